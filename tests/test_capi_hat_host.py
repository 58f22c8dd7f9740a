"""Host checks of the factorised-blank entry points (mrnnt_hat_* and the mrnnt_cpu_hat_* twins, include/mrnnt.h): the
symbols exist beside an unchanged version 13, and null pointers, a short workspace and a short row_state_len are each
refused with RNNT_STATUS_INVALID_VALUE before any device call. No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "monotonic-rnnt_amd", "libmonotonic_rnnt_amd.so")
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "monotonic-rnnt_amd")], check=True)
    import _mrnnt_lib
    return _mrnnt_lib.load()


class Case:
    """A valid two-utterance problem on host buffers (the device pointers are never dereferenced: every call of
    these tests fails on the host)."""

    def __init__(self):
        import _mrnnt_lib as L
        self.T, self.S = np.array([4, 7], np.int32), np.array([2, 5], np.int32)
        self.V, self.rows = 8, 4 * 3 + 7 * 6
        self.acts = np.zeros((self.rows, self.V), np.float32)
        self.labels = np.ones((2, 5), np.int32)
        p = L.MrnntProblem()
        p.B, p.V, p.blank = 2, self.V, 3
        p.T_host, p.S_host = self.T.ctypes.data, self.S.ctypes.data
        p.T_dev, p.S_dev = p.T_host, p.S_host
        p.label_stride = 5
        p.acts, p.labels, p.num_rows = self.acts.ctypes.data, self.labels.ctypes.data, self.rows
        self.p = p
        self.out = np.zeros(self.rows * self.V, np.float32)
        self.al = np.zeros((2, 7), np.int32)

    def need(self, lib, cpu):
        n = ctypes.c_size_t(0)
        size = lib.mrnnt_cpu_workspace_size if cpu else lib.mrnnt_workspace_size
        assert size(ctypes.byref(self.p), ctypes.byref(n)) == 0
        return n.value


def test_symbols_are_exported(lib):
    for name in ("mrnnt_hat_forward", "mrnnt_hat_backward", "mrnnt_hat_backward_tracked", "mrnnt_hat_align",
                 "mrnnt_cpu_hat_forward", "mrnnt_cpu_hat_backward", "mrnnt_cpu_hat_align"):
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for the symbols


def _call(lib, c, cpu, entry, ws, ws_bytes, out=True, row_state=None, row_state_len=0):
    o = vp(c.out.ctypes.data) if out else None
    fn = getattr(lib, ("mrnnt_cpu_hat_" if cpu else "mrnnt_hat_") + entry)
    tail = 0 if cpu else None  # num_threads / stream
    if entry == "forward":
        return fn(ctypes.byref(c.p), ws, ws_bytes, o, 1, tail)
    if entry == "align":
        return fn(ctypes.byref(c.p), ws, ws_bytes, vp(c.al.ctypes.data) if out else None, 7, None, tail)
    if entry == "backward_tracked":
        return fn(ctypes.byref(c.p), ws, None, o, row_state, row_state_len, tail)
    return fn(ctypes.byref(c.p), ws, None, o, tail)


ENTRIES = [(False, "forward"), (False, "backward"), (False, "backward_tracked"), (False, "align"), (True, "forward"),
           (True, "backward"), (True, "align")]


@pytest.mark.parametrize("cpu,entry", ENTRIES)
def test_null_pointers_are_refused(lib, cpu, entry):
    import _mrnnt_lib as L
    c = Case()
    big = np.zeros(c.need(lib, cpu), np.uint8)
    ws = vp(big.ctypes.data)
    # workspace
    assert _call(lib, c, cpu, entry, None, big.size) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace" in lib.mrnnt_last_error()
    # the output the entry point must write
    if entry != "forward":
        assert _call(lib, c, cpu, entry, ws, big.size, out=False) == L.RNNT_STATUS_INVALID_VALUE
        assert (b"alignment_out is null" if entry == "align" else b"grads is null") in lib.mrnnt_last_error()
    # acts
    c.p.acts = None
    assert _call(lib, c, cpu, entry, ws, big.size) == L.RNNT_STATUS_INVALID_VALUE
    assert b"acts is null" in lib.mrnnt_last_error()
    c.p.acts = c.acts.ctypes.data
    # labels (the host backward never reads them through this check: the device entries and the host forward do)
    if not (cpu and entry == "backward"):
        c.p.labels = None
        assert _call(lib, c, cpu, entry, ws, big.size) == L.RNNT_STATUS_INVALID_VALUE
        assert b"labels is null" in lib.mrnnt_last_error()
    assert not big.any() and not c.out.any() and not c.al.any()


@pytest.mark.parametrize("cpu,entry", [(False, "forward"), (False, "align"), (True, "forward"), (True, "align")])
def test_short_workspace_is_refused(lib, cpu, entry):
    import _mrnnt_lib as L
    c = Case()
    need = c.need(lib, cpu)
    small = np.zeros(need - 1, np.uint8)
    assert _call(lib, c, cpu, entry, vp(small.ctypes.data), small.size) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace too small" in lib.mrnnt_last_error() and str(need).encode() in lib.mrnnt_last_error()
    assert not small.any() and not c.out.any() and not c.al.any()


def test_short_row_state_is_refused(lib):
    import _mrnnt_lib as L
    c = Case()
    big = np.zeros(c.need(lib, False), np.uint8)
    state = np.zeros(c.rows, np.uint8)
    rc = _call(lib, c, False, "backward_tracked", vp(big.ctypes.data), big.size, row_state=vp(state.ctypes.data),
               row_state_len=c.rows - 1)
    assert rc == L.RNNT_STATUS_INVALID_VALUE
    assert b"row_state has" in lib.mrnnt_last_error()
    assert not state.any() and not c.out.any()
