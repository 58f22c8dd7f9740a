"""Host-side tests of the fused joint's best-path and posterior entry points (no GPU needed): mrnnt_joint_align and
mrnnt_joint_posteriors are declared, exported and bound, their host checks refuse a bad output or stride before any
device call, and the Python surface exists with the loss's own input errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "monotonic-rnnt_amd", "libmonotonic_rnnt_amd.so")
NAMES = ("mrnnt_joint_align", "mrnnt_joint_posteriors")


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
    assert len(lib.mrnnt_joint_align.argtypes) == 7 and len(lib.mrnnt_joint_posteriors.argtypes) == 11


def test_version_stays_13(lib):
    assert lib.mrnnt_version() == 13
    assert re.search(r"#define\s+MRNNT_VERSION\s+13\b", open(os.path.join(INC, "mrnnt.h")).read())


def test_joint_align_host_checks(lib):
    import _mrnnt_lib as L
    p, keep = _joint_problem()
    out = (ctypes.c_int * (2 * 7))()  # host memory standing in for the output: the call must fail before any use
    assert lib.mrnnt_joint_align(ctypes.byref(p), None, 0, None, 7, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignment_out is null" in lib.mrnnt_last_error()
    assert lib.mrnnt_joint_align(ctypes.byref(p), None, 0, out, 6, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignment_out row stride 6 < max input length 7" in lib.mrnnt_last_error()
    # a good output and stride: the next host check (the NULL inputs) answers, still without a device call
    assert lib.mrnnt_joint_align(ctypes.byref(p), None, 0, out, 7, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"enc / pred / weight is null" in lib.mrnnt_last_error()
    p.H = 200  # the plan's own validation comes first, as for the forward
    assert lib.mrnnt_joint_align(ctypes.byref(p), None, 0, out, 7, None, None) == L.RNNT_STATUS_INVALID_VALUE
    assert b"joint H" in lib.mrnnt_last_error()


def test_joint_posteriors_host_checks(lib):
    import _mrnnt_lib as L
    p, keep = _joint_problem()  # max T = 7, max S = 5
    buf = (ctypes.c_float * (2 * 7 * 6))()  # host memory standing in for the outputs, never used

    def call(grid_T=7, grid_S1=6, emit_stride=7, time_stride=5, blank=buf, label=buf, emit=buf, ltime=buf):
        return lib.mrnnt_joint_posteriors(ctypes.byref(p), None, blank, label, grid_T, grid_S1, emit, emit_stride,
                                          ltime, time_stride, None)

    for kw, msg in ((dict(grid_T=6), b"posterior grid [6, 6]"), (dict(grid_S1=5), b"posterior grid [7, 5]"),
                    (dict(emit_stride=6), b"emit row stride 6 < max input length 7"),
                    (dict(time_stride=4), b"label_time row stride 4 < max label length 5")):
        assert call(**kw) == L.RNNT_STATUS_INVALID_VALUE, kw
        assert msg in lib.mrnnt_last_error(), (kw, lib.mrnnt_last_error())
    # a stride belongs to its output: with the output NULL it is not looked at, and the NULL workspace answers
    for kw in (dict(), dict(grid_T=0, grid_S1=0, blank=None, label=None), dict(emit_stride=0, emit=None),
               dict(time_stride=0, ltime=None)):
        assert call(**kw) == L.RNNT_STATUS_INVALID_VALUE, kw
        assert b"workspace is null" in lib.mrnnt_last_error(), (kw, lib.mrnnt_last_error())


def test_python_surface():
    import torch

    import monotonic_rnnt_joint as J
    import monotonic_rnnt_op as op
    assert "monotonic_rnnt_joint_align" in J.__all__ and "monotonic_rnnt_joint_posteriors" in J.__all__
    assert J.Posteriors is op.Posteriors
    B, T, S, H, V = 2, 5, 3, 128, 16
    enc, pred, w = torch.zeros(B, T, H), torch.zeros(B, S + 1, H), torch.zeros(V, H)
    lab = torch.ones(B, S, dtype=torch.int32)
    Tl, Sl = torch.tensor([5, 4]), torch.tensor([3, 0])
    for fn in (J.monotonic_rnnt_joint_loss, J.monotonic_rnnt_joint_align, J.monotonic_rnnt_joint_posteriors):
        with pytest.raises(RuntimeError, match="enc must be a GPU tensor"):
            fn(enc, pred, w, None, lab, Tl, Sl)
        with pytest.raises(RuntimeError, match="enc must be a GPU tensor"):  # requires_grad is ignored, not an error
            fn(enc.clone().requires_grad_(True), pred, w, None, lab, Tl, Sl)
