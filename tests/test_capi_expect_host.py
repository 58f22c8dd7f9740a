"""Host checks of the expected-cost entry points (mrnnt_expect_* and the mrnnt_cpu_expect_* twins, include/mrnnt.h):
every violation is refused with RNNT_STATUS_INVALID_VALUE and a message before any device call, and the workspace-size
query covers the loss's workspace and the expectation state. No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "monotonic-rnnt_amd", "libmonotonic_rnnt_amd.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "monotonic-rnnt_amd")], check=True)
    import _mrnnt_lib
    return _mrnnt_lib.load()


def _problem(T, S, V=8):
    import _mrnnt_lib as L
    T, S = np.asarray(T, np.int32), np.asarray(S, np.int32)
    p = L.MrnntProblem()
    p.B, p.V, p.blank = len(T), V, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.label_stride = int(S.max(initial=0))
    p.num_rows = -1
    return p, (T, S)


def test_symbols_are_exported(lib):
    for name in ("mrnnt_expect_workspace_size", "mrnnt_expect_forward", "mrnnt_expect_backward",
                 "mrnnt_expect_backward_tracked", "mrnnt_cpu_expect_workspace_size", "mrnnt_cpu_expect_forward",
                 "mrnnt_cpu_expect_backward"):
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for the symbols


@pytest.mark.parametrize("cpu", [False, True])
def test_workspace_size_covers_the_loss_and_the_state(lib, cpu):
    import _mrnnt_lib as L
    p, keep = _problem([4, 70], [2, 7])
    rows = 4 * 3 + 70 * 8
    loss_size = lib.mrnnt_cpu_workspace_size if cpu else lib.mrnnt_workspace_size
    size = lib.mrnnt_cpu_expect_workspace_size if cpu else lib.mrnnt_expect_workspace_size
    n, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert loss_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    assert size(ctypes.byref(p), ctypes.byref(ne)) == L.RNNT_STATUS_SUCCESS
    assert ne.value >= n.value + 2 * 8 * rows + 8 * 2  # the loss's workspace, then A, Bk (fp64 [N]) and R (fp64 [B])
    al = np.zeros(2 * 70, np.int32)  # a restricting alignment is allowed (and its band arrays are covered)
    p.alignment, p.align_stride = al.ctypes.data, 70
    na, nea = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert loss_size(ctypes.byref(p), ctypes.byref(na)) == L.RNNT_STATUS_SUCCESS
    assert size(ctypes.byref(p), ctypes.byref(nea)) == L.RNNT_STATUS_SUCCESS
    assert nea.value >= na.value + 2 * 8 * rows + 8 * 2 and na.value > n.value
    assert size(ctypes.byref(p), None) == L.RNNT_STATUS_INVALID_VALUE
    p, keep = _problem([4], [5])  # the loss's own validation still applies
    assert size(ctypes.byref(p), ctypes.byref(ne)) == L.RNNT_STATUS_INVALID_VALUE
    assert b"invalid lengths" in lib.mrnnt_last_error()


@pytest.mark.parametrize("cpu,entry", [(False, "forward"), (False, "backward"), (False, "backward_tracked"),
                                       (True, "forward"), (True, "backward")])
def test_host_checks_refuse_before_any_device_call(lib, cpu, entry):
    """A NULL workspace with non-NULL outputs, too small a workspace, NULL grads: INVALID_VALUE, nothing written."""
    import _mrnnt_lib as L
    vp = ctypes.c_void_p
    T, S, V = [4, 7], [2, 5], 8
    p, keep = _problem(T, S, V)
    rows = 4 * 3 + 7 * 6
    acts = np.zeros((rows, V), np.float32)
    labels = np.ones((2, 5), np.int32)
    p.acts, p.labels, p.num_rows = acts.ctypes.data, labels.ctypes.data, rows
    p.T_dev, p.S_dev = p.T_host, p.S_host  # (never dereferenced: every call below fails on the host)
    out = np.zeros(max(rows * V, 2), np.float32)
    small = np.zeros(64, np.uint8)
    fn = getattr(lib, ("mrnnt_cpu_expect_" if cpu else "mrnnt_expect_") + entry)
    size = lib.mrnnt_cpu_expect_workspace_size if cpu else lib.mrnnt_expect_workspace_size
    need = ctypes.c_size_t(0)
    assert size(ctypes.byref(p), ctypes.byref(need)) == L.RNNT_STATUS_SUCCESS and need.value > small.size

    def call(ws, ws_bytes, outputs=True):
        o = vp(out.ctypes.data) if outputs else None
        args = [ctypes.byref(p), ws, ws_bytes, None, None]
        if entry == "forward":
            args += [o, o, 1]
        else:
            args += [None, None, o]
            if entry == "backward_tracked":
                args += [None, 0]
        return fn(*args, 0 if cpu else None)

    assert call(None, 0) == L.RNNT_STATUS_INVALID_VALUE and b"workspace too small" in lib.mrnnt_last_error()
    assert call(None, need.value) == L.RNNT_STATUS_INVALID_VALUE and b"workspace too small" in lib.mrnnt_last_error()
    assert call(vp(small.ctypes.data), small.size) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace too small" in lib.mrnnt_last_error()
    assert str(need.value).encode() in lib.mrnnt_last_error()
    if entry != "forward":
        big = np.zeros(need.value, np.uint8)
        assert call(vp(big.ctypes.data), big.size, outputs=False) == L.RNNT_STATUS_INVALID_VALUE
        assert b"grads is null" in lib.mrnnt_last_error()
        assert not big.any()
    assert np.all(out == 0) and not small.any()
