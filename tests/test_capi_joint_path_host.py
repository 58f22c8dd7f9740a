"""Host checks of the joint path-score entry points (mrnnt_joint_path_*, include/mrnnt.h): the symbols, the workspace
size, the host-known row bound, and every violation refused with RNNT_STATUS_INVALID_VALUE and a message before any
device call -- the workspace is NULL. No GPU needed."""
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


def _problem(T, S, V=8, H=128):
    import _mrnnt_lib as L
    T, S = np.asarray(T, np.int32), np.asarray(S, np.int32)
    p = L.MrnntJointProblem()
    p.B, p.V, p.H, p.blank = len(T), V, H, 0
    p.T_host, p.S_host = T.ctypes.data, S.ctypes.data
    p.label_stride = int(S.max(initial=0))
    p.enc_stride = int(T.max()) * H
    p.pred_stride = (int(S.max()) + 1) * H
    return p, (T, S)


def _inband(T, S):
    t = np.arange(T)
    return int(np.sum(np.minimum(t, S) - np.maximum(0, t - (T - S)) + 1))


def test_symbols_are_exported(lib):
    for name in ("mrnnt_joint_path_workspace_size", "mrnnt_joint_path_row_bound", "mrnnt_joint_path_forward",
                 "mrnnt_joint_path_rows", "mrnnt_joint_path_backward"):
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for the symbols


def test_workspace_size_covers_the_joint_and_grows_with_the_paths(lib):
    import _mrnnt_lib as L
    p, keep = _problem([4, 70], [2, 7])
    n, n1, n64 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mrnnt_joint_workspace_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    assert lib.mrnnt_joint_path_workspace_size(ctypes.byref(p), 1, ctypes.byref(n1)) == L.RNNT_STATUS_SUCCESS
    assert lib.mrnnt_joint_path_workspace_size(ctypes.byref(p), 64, ctypes.byref(n64)) == L.RNNT_STATUS_SUCCESS
    assert n.value <= n1.value < n64.value
    # the joint's workspace, then the two hull arrays and at least a validity word per path
    assert n1.value >= n.value + 2 * 74 * 4
    assert n64.value >= n.value + 2 * 74 * 4 + 64 * 2 * 4


@pytest.mark.parametrize("T,S", [([4, 70], [2, 7]), ([1, 9, 130, 65], [0, 9, 40, 1]), ([5], [0]), ([6, 6], [6, 3])])
@pytest.mark.parametrize("K", [1, 3, 9, 64])
def test_row_bound_is_the_host_sum(lib, T, S, K):
    import _mrnnt_lib as L
    p, keep = _problem(T, S)
    rows = ctypes.c_int64(-1)
    assert lib.mrnnt_joint_path_row_bound(ctypes.byref(p), K, ctypes.byref(rows)) == L.RNNT_STATUS_SUCCESS
    want = sum(min(K * t, _inband(t, s)) for t, s in zip(T, S))
    assert rows.value == want
    full = ctypes.c_int64(-1)
    assert lib.mrnnt_joint_row_bound(ctypes.byref(p), ctypes.byref(full)) == L.RNNT_STATUS_SUCCESS
    assert rows.value <= full.value == sum(_inband(t, s) for t, s in zip(T, S))


@pytest.mark.parametrize("entry", ["workspace_size", "row_bound", "forward", "rows"])
def test_host_checks_refuse_before_any_device_call(lib, entry):
    """NULL workspace, no device pointers: each violation of the host-check list is INVALID_VALUE with its message."""
    import _mrnnt_lib as L
    vp = ctypes.c_void_p
    T_max, K = 7, 3
    al = np.zeros((2, K, T_max), np.int32)
    out = np.zeros((2, K), np.float32)
    size, rows = ctypes.c_size_t(0), ctypes.c_int64(0)
    sizing = entry in ("workspace_size", "row_bound")

    def call(prob, alignments, num_paths, stride):
        if entry == "workspace_size":
            return lib.mrnnt_joint_path_workspace_size(ctypes.byref(prob), num_paths, ctypes.byref(size))
        if entry == "row_bound":
            return lib.mrnnt_joint_path_row_bound(ctypes.byref(prob), num_paths, ctypes.byref(rows))
        if entry == "forward":
            return lib.mrnnt_joint_path_forward(ctypes.byref(prob), None, 0, alignments, num_paths, stride,
                                                vp(out.ctypes.data), None)
        return lib.mrnnt_joint_path_rows(ctypes.byref(prob), None, 0, alignments, num_paths, stride, None,
                                         vp(out.ctypes.data), None)

    def refused(rc, *needles):
        msg = lib.mrnnt_last_error()
        return rc == L.RNNT_STATUS_INVALID_VALUE and all(s in msg for s in needles)

    a = vp(al.ctypes.data)
    p, keep = _problem([4, 7], [2, 5])
    assert refused(call(p, a, 0, T_max), b"num_paths")
    assert refused(call(p, a, -2, T_max), b"num_paths")
    restricted, keep2 = _problem([4, 7], [2, 5])
    given = np.zeros(2 * T_max, np.int32)
    restricted.alignment, restricted.align_stride = given.ctypes.data, T_max
    assert refused(call(restricted, a, K, T_max), b"p->alignment must be NULL")
    bad_h, keep3 = _problem([4, 7], [2, 5], H=200)
    assert refused(call(bad_h, a, K, T_max), b"joint H must be")
    bad_len, keep4 = _problem([4], [5])  # the loss's own validation still applies
    assert refused(call(bad_len, a, K, T_max), b"invalid lengths")
    if sizing:
        assert call(p, a, K, T_max) == L.RNNT_STATUS_SUCCESS
        return
    assert refused(call(p, None, K, T_max), b"alignments is null")
    assert refused(call(p, a, K, T_max - 1), b"alignments row stride")
    # nothing wrong on the host-check list: the call gets as far as its pointers / workspace, and still writes nothing
    assert call(p, a, K, T_max) == L.RNNT_STATUS_INVALID_VALUE
    msg = lib.mrnnt_last_error()
    assert not any(s in msg for s in (b"num_paths", b"alignments", b"p->alignment", b"joint H")), msg
    assert np.all(out == 0)


def test_backward_refuses_a_restricting_alignment_and_a_bad_row_count(lib):
    import _mrnnt_lib as L
    p, keep = _problem([4, 7], [2, 5])
    rc = lib.mrnnt_joint_path_backward(ctypes.byref(p), None, -1, None, None, None, None, None)
    assert rc == L.RNNT_STATUS_INVALID_VALUE  # (its pointers come first: nothing is launched)
    given = np.zeros(2 * 7, np.int32)
    p.alignment, p.align_stride = given.ctypes.data, 7
    rc = lib.mrnnt_joint_path_backward(ctypes.byref(p), None, 0, None, None, None, None, None)
    assert rc == L.RNNT_STATUS_INVALID_VALUE and b"p->alignment must be NULL" in lib.mrnnt_last_error()
