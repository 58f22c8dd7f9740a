"""Host-side tests of the fused joint's factorised-blank (HAT) entry points (no GPU needed): mrnnt_joint_hat_forward /
_backward / _align are declared, exported and bound as an addition to ABI version 13, their host checks answer with a
NULL workspace before any device call, and the Python surface exists -- with the path scores and the expected costs
still softmax-only."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "monotonic-rnnt_amd", "libmonotonic_rnnt_amd.so")
NAMES = ("mrnnt_joint_hat_forward", "mrnnt_joint_hat_backward", "mrnnt_joint_hat_align")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "monotonic-rnnt_amd")], check=True)
    import _mrnnt_lib
    return _mrnnt_lib.load()


def _joint_problem(T=(4, 7), S=(2, 5), H=256, V=64):
    """A joint problem with host lengths only: every device pointer NULL, so a call that got past the host checks
    under test would still stop at the pointer checks, never at a device call."""
    import _mrnnt_lib as L
    T, S = np.asarray(T, np.int32), np.asarray(S, np.int32)
    p = L.MrnntJointProblem()
    p.B, p.V, p.H, p.blank = len(T), V, H, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.enc_stride, p.pred_stride = int(T.max()) * H, (int(S.max()) + 1) * H
    p.label_stride = int(S.max())
    return p, (T, S)


def test_symbols_declared_exported_and_bound(lib):
    src = open(os.path.join(INC, "mrnnt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bRNNTStatus\s+" + name + r"\s*\(", src), name
        assert re.search(r"\sT\s" + name + r"\b", exported), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    # the argument lists of the softmax entry points they stand beside
    assert len(lib.mrnnt_joint_hat_forward.argtypes) == len(lib.mrnnt_joint_forward.argtypes) == 6
    assert len(lib.mrnnt_joint_hat_backward.argtypes) == len(lib.mrnnt_joint_backward.argtypes) == 9
    assert len(lib.mrnnt_joint_hat_align.argtypes) == len(lib.mrnnt_joint_align.argtypes) == 7


def test_version_stays_13(lib):
    assert lib.mrnnt_version() == 13
    assert re.search(r"#define\s+MRNNT_VERSION\s+13\b", open(os.path.join(INC, "mrnnt.h")).read())


def test_bad_H_is_refused_by_all_three(lib):
    import _mrnnt_lib as L
    p, keep = _joint_problem(H=200)
    out = (ctypes.c_int * (2 * 7))()
    calls = (lambda: lib.mrnnt_joint_hat_forward(ctypes.byref(p), None, 0, None, 1, None),
             lambda: lib.mrnnt_joint_hat_backward(ctypes.byref(p), None, 0, None, None, None, None, None, None),
             lambda: lib.mrnnt_joint_hat_align(ctypes.byref(p), None, 0, out, 7, None, None))
    for call in calls:
        assert call() == L.RNNT_STATUS_INVALID_VALUE
        assert b"joint H" in lib.mrnnt_last_error()


def test_hat_align_host_checks(lib):
    import _mrnnt_lib as L
    p, keep = _joint_problem()
    out = (ctypes.c_int * (2 * 7))()  # host memory standing in for the output: the call must fail before any use
    assert lib.mrnnt_joint_hat_align(ctypes.byref(p), None, 0, None, 7, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignment_out is null" in lib.mrnnt_last_error()
    assert lib.mrnnt_joint_hat_align(ctypes.byref(p), None, 0, out, 6, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignment_out row stride 6 < max input length 7" in lib.mrnnt_last_error()
    # a good output and stride: the next host check (the NULL inputs) answers, still without a device call
    assert lib.mrnnt_joint_hat_align(ctypes.byref(p), None, 0, out, 7, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"enc / pred / weight is null" in lib.mrnnt_last_error()


def test_hat_forward_and_backward_host_checks(lib):
    """The checks of mrnnt_joint_forward / mrnnt_joint_backward, in their order, with a NULL workspace."""
    import _mrnnt_lib as L
    p, keep = _joint_problem()
    assert lib.mrnnt_joint_hat_forward(ctypes.byref(p), None, 0, None, 1, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"enc / pred / weight is null" in lib.mrnnt_last_error()
    assert (lib.mrnnt_joint_hat_backward(ctypes.byref(p), None, 0, None, None, None, None, None, None)
            == L.RNNT_STATUS_INVALID_VALUE)
    assert b"enc / pred / weight is null" in lib.mrnnt_last_error()
    p.hact_ld = 100  # the plan's own validation comes before the pointers
    assert (lib.mrnnt_joint_hat_backward(ctypes.byref(p), None, 0, None, None, None, None, None, None)
            == L.RNNT_STATUS_INVALID_VALUE)
    assert b"hact_ld" in lib.mrnnt_last_error()


def test_python_surface():
    import torch

    import monotonic_rnnt_joint as J
    for name in ("MonotonicRNNTJointHatFunction", "monotonic_rnnt_joint_hat_loss"):
        assert name in J.__all__ and hasattr(J, name), name
    init = open(os.path.join(ROOT, "monotonic-rnnt_amd", "pytorch_binding", "__init__.py")).read()
    assert '"MonotonicRNNTJointHatFunction"' in init and '"monotonic_rnnt_joint_hat_loss"' in init
    assert (list(inspect.signature(J.monotonic_rnnt_joint_hat_loss).parameters)
            == list(inspect.signature(J.monotonic_rnnt_joint_loss).parameters))
    for fn in (J.monotonic_rnnt_joint_align, J.monotonic_rnnt_joint_posteriors, J.monotonic_rnnt_joint_sample):
        assert inspect.signature(fn).parameters["blank_factorized"].default is False, fn.__name__
    for fn in (J.monotonic_rnnt_joint_path_loss, J.monotonic_rnnt_joint_expected_cost):  # softmax-only
        assert "blank_factorized" not in inspect.signature(fn).parameters, fn.__name__
    B, T, S, H, V = 2, 5, 3, 128, 16
    enc, pred, w = torch.zeros(B, T, H), torch.zeros(B, S + 1, H), torch.zeros(V, H)
    lab = torch.ones(B, S, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="enc must be a GPU tensor"):
        J.monotonic_rnnt_joint_hat_loss(enc, pred, w, None, lab, torch.tensor([5, 4]), torch.tensor([3, 0]))
