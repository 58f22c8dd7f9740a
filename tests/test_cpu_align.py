"""monotonic_rnnt_align on the host implementation (mrnnt_cpu_align): the shared checks of tests/_align_checks.py
on CPU tensors, and the C-level argument validation. No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import _align_checks as A


run_cpu = A.run_cpu


def test_exported_from_the_package():
    import monotonic_rnnt_op as op
    assert "monotonic_rnnt_align" in op.__all__
    src = open(op.__file__.replace("monotonic_rnnt_op.py", "__init__.py")).read()
    assert "monotonic_rnnt_align" in src


def test_valid_and_cost_is_the_paths():
    rng = np.random.default_rng(1)
    acts, labels, T, S = A.ragged(rng, [(12, 4), (7, 0), (9, 9), (70, 64), (1, 1), (1, 0)], 8)
    al, _ = A.check_all(run_cpu, acts, labels, T, S)
    assert al.shape == (6, 70)


def test_ignores_requires_grad():
    import monotonic_rnnt_op as op
    rng = np.random.default_rng(2)
    acts, labels, T, S = A.ragged(rng, [(6, 2)], 5)
    a = torch.from_numpy(acts).requires_grad_(True)
    al, costs = op.monotonic_rnnt_align(a, torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S))
    assert not al.requires_grad and not costs.requires_grad and a.grad is None


def test_optimal_against_the_oracle_tiny():
    A.check_optimal_tiny(run_cpu)


@pytest.mark.parametrize("W", [64, 65, 129, 257, 513, 1025])
def test_optimal_at_dispatch_boundaries(W):
    A.check_boundary(run_cpu, W)


@pytest.mark.parametrize("W", [1100, 1537])
def test_optimal_at_the_gpu_paths_wider_dispatch_sizes(W):
    A.check_boundary(run_cpu, W, V=4)


@pytest.mark.parametrize("T1,S1", [(40, 20), (150, 129)])
def test_exact_planted_path(T1, S1):
    A.check_exact_path(run_cpu, T1, S1)


def test_restricting_alignment():
    A.check_restriction(run_cpu)


def test_value_domain():
    A.check_value_domain(run_cpu)


def test_strides():
    A.check_strides(run_cpu)


def test_c_level_validation():
    """mrnnt_cpu_align rejects a short row stride and a NULL output with a message; the ABI is version 13."""
    import _mrnnt_lib as L
    lib = L.load()
    assert lib.mrnnt_version() == 13
    T = np.array([4, 7], np.int32)
    S = np.array([2, 5], np.int32)
    rows = int(np.sum(T * (S + 1)))
    acts = np.zeros((rows, 8), np.float32)
    labels = np.ones((2, 5), np.int32)
    p = L.MrnntProblem()
    p.B, p.V, p.blank = 2, 8, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.acts, p.labels, p.label_stride, p.num_rows = acts.ctypes.data, labels.ctypes.data, 5, rows
    n = ctypes.c_size_t(0)
    assert lib.mrnnt_cpu_workspace_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    ws = np.zeros(n.value, np.uint8)
    out = np.zeros((2, 7), np.int32)
    costs = np.zeros(2, np.float32)
    vp = ctypes.c_void_p
    st = lib.mrnnt_cpu_align(ctypes.byref(p), vp(ws.ctypes.data), n.value, vp(out.ctypes.data), 6,
                             vp(costs.ctypes.data), 1)
    assert st == L.RNNT_STATUS_INVALID_VALUE and b"row stride" in lib.mrnnt_last_error()
    st = lib.mrnnt_cpu_align(ctypes.byref(p), vp(ws.ctypes.data), n.value, None, 7, vp(costs.ctypes.data), 1)
    assert st == L.RNNT_STATUS_INVALID_VALUE and b"null" in lib.mrnnt_last_error()
    st = lib.mrnnt_cpu_align(ctypes.byref(p), vp(ws.ctypes.data), n.value - 1, vp(out.ctypes.data), 7, None, 1)
    assert st == L.RNNT_STATUS_INVALID_VALUE and b"workspace" in lib.mrnnt_last_error()
    st = lib.mrnnt_cpu_align(ctypes.byref(p), vp(ws.ctypes.data), n.value, vp(out.ctypes.data), 7, None, 1)  # no costs
    assert st == L.RNNT_STATUS_SUCCESS
    A.check_valid(out, labels, T, S)
    # the GPU entry point validates the same arguments on the host, before any HIP call
    st = lib.mrnnt_align(ctypes.byref(p), None, 0, None, 7, None, None)
    assert st == L.RNNT_STATUS_INVALID_VALUE
