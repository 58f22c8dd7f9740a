"""Host checks of the joint expected-cost entry points (mrnnt_joint_expect_*, include/mrnnt.h): the symbols, the
workspace size, and every violation refused with RNNT_STATUS_INVALID_VALUE and a message before any device call -- the
workspace is NULL or too small, and no pointer handed over is ever dereferenced. No GPU needed."""
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


def _problem(T, S, V=8, H=128, pointers=False):
    """pointers: enc / pred / weight / labels / device lengths point at (16-byte aligned) host memory, so that the
    pointer checks pass; the entry points refuse the call before anything reads them."""
    import _mrnnt_lib as L
    T, S = np.asarray(T, np.int32), np.asarray(S, np.int32)
    p = L.MrnntJointProblem()
    p.B, p.V, p.H, p.blank = len(T), V, H, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.label_stride = int(S.max(initial=0))
    p.enc_stride = int(T.max()) * H
    p.pred_stride = (int(S.max()) + 1) * H
    keep = [T, S]
    if pointers:
        raw = np.zeros(64 + 16, np.uint8)
        at = raw.ctypes.data + (-raw.ctypes.data) % 16
        p.enc = p.pred = p.weight = p.labels = p.T_dev = p.S_dev = at
        keep.append(raw)
    return p, keep


def _refused(lib, rc, *needles):
    import _mrnnt_lib as L
    msg = lib.mrnnt_last_error()
    return rc == L.RNNT_STATUS_INVALID_VALUE and len(msg) > 0 and all(s in msg for s in needles)


def test_symbols_are_exported(lib):
    for name in ("mrnnt_joint_expect_workspace_size", "mrnnt_joint_expect_forward", "mrnnt_joint_expect_rows",
                 "mrnnt_joint_expect_backward"):
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for mrnnt_joint_expect_forward


@pytest.mark.parametrize("T,S", [([4, 70], [2, 7]), ([1, 9, 130, 65], [0, 9, 40, 1]), ([5], [0])])
def test_workspace_size_covers_the_joint_and_the_expectation_state(lib, T, S):
    import _mrnnt_lib as L
    p, keep = _problem(T, S)
    n, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mrnnt_joint_workspace_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    assert lib.mrnnt_joint_expect_workspace_size(ctypes.byref(p), ctypes.byref(ne)) == L.RNNT_STATUS_SUCCESS
    N, B = sum(t * (s + 1) for t, s in zip(T, S)), len(T)
    assert ne.value >= n.value + 8 * (2 * N + B)  # A, Bk fp64 [N], R fp64 [B], then the coefficient arrays
    # with an alignment the joint's own plan grows and the extras still follow it
    al = np.zeros(len(T) * max(T), np.int32)
    p.alignment, p.align_stride = al.ctypes.data, max(T)
    assert lib.mrnnt_joint_workspace_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    assert lib.mrnnt_joint_expect_workspace_size(ctypes.byref(p), ctypes.byref(ne)) == L.RNNT_STATUS_SUCCESS
    assert ne.value >= n.value + 8 * (2 * N + B)


@pytest.mark.parametrize("entry", ["workspace_size", "forward", "rows", "backward"])
def test_everything_the_joint_forward_checks(lib, entry):
    size, out = ctypes.c_size_t(0), np.zeros(4, np.float32)
    o = vp(out.ctypes.data)

    def call(prob):
        if entry == "workspace_size":
            return lib.mrnnt_joint_expect_workspace_size(ctypes.byref(prob), ctypes.byref(size))
        if entry == "forward":
            return lib.mrnnt_joint_expect_forward(ctypes.byref(prob), None, 0, None, None, 0, 0, o, o, 1, None)
        if entry == "rows":
            return lib.mrnnt_joint_expect_rows(ctypes.byref(prob), None, 0, None, None, 0, 0, None, None, o, None)
        return lib.mrnnt_joint_expect_backward(ctypes.byref(prob), None, 0, None, None, None, None, None)

    bad_h, keep = _problem([4, 7], [2, 5], H=200, pointers=True)
    assert _refused(lib, call(bad_h), b"joint H must be")
    bad_len, keep2 = _problem([4], [5], pointers=True)  # the loss's own validation still applies
    assert _refused(lib, call(bad_len), b"invalid lengths")
    bad_stride, keep3 = _problem([4, 7], [2, 5], pointers=True)
    bad_stride.enc_stride = 6 * 128
    assert _refused(lib, call(bad_stride), b"strides")
    if entry == "workspace_size":
        assert lib.mrnnt_joint_expect_workspace_size(None, ctypes.byref(size)) != 0 and lib.mrnnt_last_error()
        good, keep4 = _problem([4, 7], [2, 5])
        assert _refused(lib, lib.mrnnt_joint_expect_workspace_size(ctypes.byref(good), None), b"null size")
        return
    null_ptrs, keep5 = _problem([4, 7], [2, 5])  # enc / pred / weight NULL
    assert _refused(lib, call(null_ptrs), b"null")
    assert np.all(out == 0)


@pytest.mark.parametrize("entry", ["forward", "rows"])
def test_grid_workspace_and_count_checks(lib, entry):
    import _mrnnt_lib as L
    out, cost = np.zeros(4, np.float32), np.zeros(2 * 8 * 8, np.float32)
    o, c = vp(out.ctypes.data), vp(cost.ctypes.data)
    p, keep = _problem([4, 7], [2, 5], pointers=True)
    need = ctypes.c_size_t(0)
    assert lib.mrnnt_joint_expect_workspace_size(ctypes.byref(p), ctypes.byref(need)) == L.RNNT_STATUS_SUCCESS
    fake = vp(keep[-1].ctypes.data)  # a non-NULL workspace that is too small: refused by its size, never touched

    def call(wb, we, gT, gS1, ws=None, ws_bytes=0, count=o):
        if entry == "forward":
            return lib.mrnnt_joint_expect_forward(ctypes.byref(p), ws, ws_bytes, wb, we, gT, gS1, o, o, 1, None)
        return lib.mrnnt_joint_expect_rows(ctypes.byref(p), ws, ws_bytes, wb, we, gT, gS1, None, None, count, None)

    # a grid smaller than [max T, max S + 1] = [7, 6] when either cost array is given
    for wb, we in ((c, None), (None, c), (c, c)):
        assert _refused(lib, call(wb, we, 6, 6), b"cost grid", b"[7, 6]")
        assert _refused(lib, call(wb, we, 7, 5), b"cost grid")
        assert _refused(lib, call(wb, we, 0, 0), b"cost grid")
    # ... and not looked at when neither is: the call gets as far as its workspace
    for args in ((None, None, 0, 0), (c, c, 7, 6), (c, None, 8, 8)):
        assert _refused(lib, call(*args), b"workspace too small")
        assert _refused(lib, call(*args, ws=fake, ws_bytes=need.value - 1), b"workspace too small")
        assert _refused(lib, call(*args, ws=None, ws_bytes=need.value), b"workspace too small")
    if entry == "rows":
        assert _refused(lib, call(None, None, 0, 0, count=None), b"count is null")
        assert _refused(lib, call(c, c, 7, 6, ws=fake, ws_bytes=need.value, count=None), b"count is null")
    assert np.all(out == 0) and np.all(keep[-1] == 0)


def test_backward_checks_its_row_count_and_takes_an_alignment(lib):
    import _mrnnt_lib as L
    p, keep = _problem([4, 7], [2, 5], pointers=True)
    assert _refused(lib, lib.mrnnt_joint_expect_backward(ctypes.byref(p), None, 0, None, None, None, None, None),
                    b"workspace is null")
    fake = vp(keep[-1].ctypes.data)
    assert _refused(lib, lib.mrnnt_joint_expect_backward(ctypes.byref(p), fake, -1, None, None, None, None, None),
                    b"n_live outside")
    inband = ctypes.c_int64(0)
    assert lib.mrnnt_joint_row_bound(ctypes.byref(p), ctypes.byref(inband)) == L.RNNT_STATUS_SUCCESS
    assert _refused(lib, lib.mrnnt_joint_expect_backward(ctypes.byref(p), fake, inband.value + 1, None, None, None,
                                                         None, None), b"n_live outside")
    assert _refused(lib, lib.mrnnt_joint_expect_backward(ctypes.byref(p), fake, 3, None, None, None, None, None),
                    b"G / Hact is null")
    # unlike the path scores, a restricting alignment is part of the problem: the same checks, no refusal of its own
    al = np.zeros(2 * 7, np.int32)
    p.alignment, p.align_stride = al.ctypes.data, 7
    assert _refused(lib, lib.mrnnt_joint_expect_backward(ctypes.byref(p), fake, 3, None, None, None, None, None),
                    b"G / Hact is null")
    assert np.all(keep[-1] == 0)
