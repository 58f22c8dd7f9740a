"""monotonic_rnnt_posteriors on the host implementation (mrnnt_cpu_posteriors): the shared checks of
tests/_posterior_checks.py on CPU tensors, and the C-level argument validation. No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import _posterior_checks as P

run_cpu = P.run_cpu


def test_exported_from_the_package():
    import monotonic_rnnt_op as op
    assert "monotonic_rnnt_posteriors" in op.__all__
    src = open(op.__file__.replace("monotonic_rnnt_op.py", "__init__.py")).read()
    assert "monotonic_rnnt_posteriors" in src


def test_brute_force_on_tiny_shapes():
    P.check_brute_force_tiny(run_cpu)


def test_gradient_identity_against_the_oracle():
    P.check_gradient_identity(run_cpu)


def test_ignores_requires_grad():
    import monotonic_rnnt_op as op
    acts, labels, T, S = P.ragged(np.random.default_rng(2), [(6, 2)], 5)
    a = torch.from_numpy(acts).requires_grad_(True)
    out = op.monotonic_rnnt_posteriors(a, torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S))
    assert not any(x.requires_grad for x in out) and a.grad is None


@pytest.mark.parametrize("W", [2, 65])
def test_width_boundaries(W):
    P.check_boundary(run_cpu, W)


def test_long_thin_utterance():
    P.check_all(run_cpu, *P.long_thin_problem())


def test_restricting_alignment():
    P.check_restriction(run_cpu)


def test_value_domain():
    P.check_value_domain(run_cpu)


def test_strides():
    P.check_strides(run_cpu)


def test_padded_layout_matches_packed():
    import monotonic_rnnt_op as op
    acts, labels, T, S = P.ragged(np.random.default_rng(10), [(19, 7), (25, 11), (6, 0), (13, 13)], 16)
    res = run_cpu(acts, labels, T, S, max_input_length=27)
    off = P.offsets(T, S)
    padded = np.full((4, 27, 15, 16), 3.0, np.float32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        padded[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    out = op.monotonic_rnnt_posteriors(torch.from_numpy(padded), torch.from_numpy(labels), torch.from_numpy(T),
                                       torch.from_numpy(S))
    assert tuple(out.blank.shape) == (4, 27, 15) and tuple(out.emit.shape) == (4, 27)
    for name in ("blank", "label"):
        got, want = getattr(out, name).numpy(), np.zeros((4, 27, 15), np.float32)
        for b, (Tb, Sb) in enumerate(zip(T, S)):
            want[b, :Tb, :Sb + 1] = getattr(res, name)[off[b]:off[b + 1]].reshape(Tb, Sb + 1)
        assert got.tobytes() == want.tobytes(), name
    assert out.emit.numpy().tobytes() == res.emit.tobytes()
    assert out.label_time.numpy().tobytes() == res.label_time.tobytes()


def test_c_level_validation():
    """mrnnt_cpu_posteriors and mrnnt_posteriors reject a short emit / label_time row stride and a NULL workspace with
    a message, on the host, before any device call; any output may be NULL; the ABI is still version 13."""
    import _mrnnt_lib as L
    lib = L.load()
    assert lib.mrnnt_version() == 13
    T = np.array([4, 7], np.int32)
    S = np.array([2, 5], np.int32)
    rows = int(np.sum(T * (S + 1)))
    acts = np.random.default_rng(0).standard_normal((rows, 8)).astype(np.float32)
    labels = np.ones((2, 5), np.int32)
    p = L.MrnntProblem()
    p.B, p.V, p.blank = 2, 8, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.acts, p.labels, p.label_stride, p.num_rows = acts.ctypes.data, labels.ctypes.data, 5, rows
    n = ctypes.c_size_t(0)
    assert lib.mrnnt_cpu_workspace_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    ws = np.zeros(n.value, np.uint8)
    vp = ctypes.c_void_p
    costs = np.zeros(2, np.float32)
    assert lib.mrnnt_cpu_forward(ctypes.byref(p), vp(ws.ctypes.data), n.value, vp(costs.ctypes.data), 1,
                                 1) == L.RNNT_STATUS_SUCCESS
    blank, label = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    emit, ltime = np.zeros((2, 7), np.float32), np.zeros((2, 5), np.float32)
    for fn, tail in ((lib.mrnnt_cpu_posteriors, 1), (lib.mrnnt_posteriors, None)):
        def call(w, e, es, lt, ts):
            return fn(ctypes.byref(p), w, vp(blank.ctypes.data), vp(label.ctypes.data), e, es, lt, ts, tail)
        st = call(vp(ws.ctypes.data), vp(emit.ctypes.data), 6, vp(ltime.ctypes.data), 5)
        assert st == L.RNNT_STATUS_INVALID_VALUE and b"emit row stride" in lib.mrnnt_last_error()
        st = call(vp(ws.ctypes.data), vp(emit.ctypes.data), 7, vp(ltime.ctypes.data), 4)
        assert st == L.RNNT_STATUS_INVALID_VALUE and b"label_time row stride" in lib.mrnnt_last_error()
        st = call(None, vp(emit.ctypes.data), 7, vp(ltime.ctypes.data), 5)
        assert st == L.RNNT_STATUS_INVALID_VALUE and b"workspace is null" in lib.mrnnt_last_error()
    # a stride is only checked for an output that is given; every output may be NULL
    st = lib.mrnnt_cpu_posteriors(ctypes.byref(p), vp(ws.ctypes.data), None, vp(label.ctypes.data), None, 0, None, 0, 1)
    assert st == L.RNNT_STATUS_SUCCESS
    st = lib.mrnnt_cpu_posteriors(ctypes.byref(p), vp(ws.ctypes.data), vp(blank.ctypes.data), None,
                                  vp(emit.ctypes.data), 7, vp(ltime.ctypes.data), 5, 1)
    assert st == L.RNNT_STATUS_SUCCESS
    ref, _ = P.np_posteriors(acts, labels, T, S)
    P.compare(P.Posteriors(blank, label, emit, ltime, costs), ref, T, S)
