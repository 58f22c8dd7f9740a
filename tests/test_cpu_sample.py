"""monotonic_rnnt_sample on the host implementation (mrnnt_cpu_sample): the shared checks of tests/_sample_checks.py on
CPU tensors -- the generator's known answers, validity and path cost, exact paths against the numpy yardstick, the
distribution, determinism and indexing, sentinels and strides -- and the C-level argument validation of both
mrnnt_cpu_sample and mrnnt_sample (host checks, before any device call). No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _posterior_checks as P
import _sample_checks as C

run_cpu = C.run_cpu


def test_philox_known_answers():
    C.check_generator()


def test_exported_declared_and_bound():
    import _mrnnt_lib as L
    import monotonic_rnnt_joint as joint
    import monotonic_rnnt_op as op
    assert "monotonic_rnnt_sample" in op.__all__ and "monotonic_rnnt_joint_sample" in joint.__all__
    src = open(op.__file__.replace("monotonic_rnnt_op.py", "__init__.py")).read()
    assert "monotonic_rnnt_sample" in src and "monotonic_rnnt_joint_sample" in src
    lib = L.load()
    assert lib.mrnnt_version() == 13
    header = open(os.path.join(os.path.dirname(L.PKG_DIR), "include", "mrnnt.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in ("mrnnt_sample", "mrnnt_cpu_sample", "mrnnt_joint_sample"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert re.search(r"\sT\s" + name + r"\b", exported), name
        assert getattr(lib, name).argtypes is not None, name


def test_validity_and_path_cost():
    C.check_validity_and_cost(run_cpu)


def test_exact_paths_free_and_restricted():
    C.check_exact_paths(run_cpu)


def test_exact_paths_of_a_two_mode_posterior():
    """Samples of one call up to 100 label positions apart (the case of the GPU kernel's window fallback). Observed
    close samples of the yardstick (seed 5, K = 130, two utterances): 3 of 260, 1.2 %."""
    acts, labels, T, S = C.bimodal_problem()
    res, share = C.check_exact(run_cpu, acts, labels, T, S, 130, 5)
    ends = (res.alignments[0, :, :100] != C.BLANK).sum(axis=1)  # labels emitted in the first 100 frames
    assert (ends >= 97).sum() >= 10 and (ends <= 3).sum() >= 10  # both modes are drawn


def test_path_frequencies():
    C.check_path_frequencies(run_cpu)


def test_arc_marginals():
    C.check_arc_marginals(run_cpu, P.run_cpu)


def test_determinism_and_indexing():
    C.check_determinism(run_cpu)


def test_value_domain():
    C.check_value_domain(run_cpu)


def test_strides():
    C.check_strides(run_cpu)


def test_ignores_requires_grad_and_checks_arguments():
    import monotonic_rnnt_op as op
    acts, labels, T, S = C.ragged(np.random.default_rng(2), [(6, 2)], 5)
    a = torch.from_numpy(acts).requires_grad_(True)
    args = (torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S))
    out = op.monotonic_rnnt_sample(a, *args, 3, 1)
    assert not any(x.requires_grad for x in out) and a.grad is None
    with pytest.raises(RuntimeError, match="num_samples"):
        op.monotonic_rnnt_sample(a, *args, 0, 1)
    with pytest.raises(RuntimeError, match="first_sample"):
        op.monotonic_rnnt_sample(a, *args, 3, 1, first_sample=(1 << 32) - 2)
    neg = op.monotonic_rnnt_sample(a, *args, 3, -1)  # a negative seed is its two's complement
    same = op.monotonic_rnnt_sample(a, *args, 3, (1 << 64) - 1)
    assert torch.equal(neg.alignments, same.alignments)


def test_padded_layout_matches_packed():
    import monotonic_rnnt_op as op
    acts, labels, T, S = C.ragged(np.random.default_rng(10), [(19, 7), (25, 11), (6, 0), (13, 13)], 16)
    res = run_cpu(acts, labels, T, S, 9, 4, max_input_length=27)
    off = C.offsets(T, S)
    padded = np.full((4, 27, 15, 16), 3.0, np.float32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        padded[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    out = op.monotonic_rnnt_sample(torch.from_numpy(padded), torch.from_numpy(labels), torch.from_numpy(T),
                                   torch.from_numpy(S), 9, 4)
    assert tuple(out.alignments.shape) == (4, 9, 27)
    assert np.array_equal(out.alignments.numpy(), res.alignments)
    assert out.path_costs.numpy().tobytes() == res.path_costs.tobytes()


def test_c_level_validation():
    """mrnnt_cpu_sample and mrnnt_sample refuse a short out_stride, num_samples = 0, sample indices outside [0, 2^32]
    and a NULL output or workspace with a message, on the host, before any device call; path_costs may be NULL."""
    import _mrnnt_lib as L
    lib = L.load()
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
    C.check_host_refusals(lib.mrnnt_cpu_sample, p, vp(ws.ctypes.data), 1, 7, lib)
    C.check_host_refusals(lib.mrnnt_sample, p, vp(ws.ctypes.data), None, 7, lib)
    out = np.zeros((2, 3, 9), np.int32)
    st = lib.mrnnt_cpu_sample(ctypes.byref(p), vp(ws.ctypes.data), 3, 12, 0, vp(out.ctypes.data), 9, None, 1)
    assert st == L.RNNT_STATUS_SUCCESS
    ref = C.np_sample(acts, labels, T, S, 3, 12)
    assert not ref.close.any()
    for b in range(2):
        assert np.array_equal(out[b, :, :T[b]], ref.rows[b]) and np.all(out[b, :, T[b]:] == 0)
