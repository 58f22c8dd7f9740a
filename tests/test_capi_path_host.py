"""Host checks of the path-score entry points (mrnnt_path_* and the mrnnt_cpu_path_* twins, include/mrnnt.h): every
violation is refused with RNNT_STATUS_INVALID_VALUE and a message before any device call -- the workspace is NULL -- and
the workspace-size query covers the loss's workspace and grows with the number of paths. No GPU needed."""
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
    for name in ("mrnnt_path_workspace_size", "mrnnt_path_forward", "mrnnt_path_backward",
                 "mrnnt_cpu_path_workspace_size", "mrnnt_cpu_path_forward", "mrnnt_cpu_path_backward"):
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for the symbols


@pytest.mark.parametrize("cpu", [False, True])
def test_workspace_size_covers_the_loss_and_grows_with_the_paths(lib, cpu):
    import _mrnnt_lib as L
    p, keep = _problem([4, 70], [2, 7])
    loss_size = lib.mrnnt_cpu_workspace_size if cpu else lib.mrnnt_workspace_size
    path_size = lib.mrnnt_cpu_path_workspace_size if cpu else lib.mrnnt_path_workspace_size
    n, n1, n64 = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert loss_size(ctypes.byref(p), ctypes.byref(n)) == L.RNNT_STATUS_SUCCESS
    assert path_size(ctypes.byref(p), 1, ctypes.byref(n1)) == L.RNNT_STATUS_SUCCESS
    assert path_size(ctypes.byref(p), 64, ctypes.byref(n64)) == L.RNNT_STATUS_SUCCESS
    assert n.value <= n1.value < n64.value
    assert n64.value >= n.value + 64 * 2 * 4  # the loss's workspace and at least a validity word per path
    assert path_size(ctypes.byref(p), 0, ctypes.byref(n1)) == L.RNNT_STATUS_INVALID_VALUE
    assert b"num_paths" in lib.mrnnt_last_error()
    al = np.zeros(2 * 70, np.int32)
    p.alignment, p.align_stride = al.ctypes.data, 70
    assert path_size(ctypes.byref(p), 1, ctypes.byref(n1)) == L.RNNT_STATUS_INVALID_VALUE
    assert b"p->alignment must be NULL" in lib.mrnnt_last_error()
    p, keep = _problem([4], [5])  # the loss's own validation still applies
    assert path_size(ctypes.byref(p), 1, ctypes.byref(n1)) == L.RNNT_STATUS_INVALID_VALUE
    assert b"invalid lengths" in lib.mrnnt_last_error()


@pytest.mark.parametrize("cpu", [False, True])
@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_host_checks_refuse_before_any_device_call(lib, cpu, entry):
    """NULL workspace, no device pointers: each violation of the host-check list is INVALID_VALUE with its message."""
    import _mrnnt_lib as L
    vp = ctypes.c_void_p
    p, keep = _problem([4, 7], [2, 5])
    K, T_max = 3, 7
    al = np.zeros((2, K, T_max), np.int32)
    out = np.zeros((2, K), np.float32)
    fn = getattr(lib, ("mrnnt_cpu_path_" if cpu else "mrnnt_path_") + entry)

    def call(prob, alignments, num_paths, stride):
        args = [ctypes.byref(prob), None, 0, alignments, num_paths, stride]
        if entry == "forward":
            args += [vp(out.ctypes.data)]
        else:
            args += [None, vp(out.ctypes.data)]  # weights = NULL, grads: never written
        return fn(*args, 0 if cpu else None)

    a = vp(al.ctypes.data)
    assert call(p, a, 0, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"num_paths" in lib.mrnnt_last_error()
    assert call(p, a, -2, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"num_paths" in lib.mrnnt_last_error()
    assert call(p, None, K, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"alignments is null" in lib.mrnnt_last_error()
    assert call(p, a, K, T_max - 1) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignments row stride" in lib.mrnnt_last_error()
    restricted, keep2 = _problem([4, 7], [2, 5])
    given = np.zeros(2 * T_max, np.int32)
    restricted.alignment, restricted.align_stride = given.ctypes.data, T_max
    assert call(restricted, a, K, T_max) == L.RNNT_STATUS_INVALID_VALUE
    assert b"p->alignment must be NULL" in lib.mrnnt_last_error()
    # nothing wrong on the host-check list: the call gets as far as its pointers / workspace, and still writes nothing
    assert call(p, a, K, T_max) == L.RNNT_STATUS_INVALID_VALUE
    msg = lib.mrnnt_last_error()
    assert not any(s in msg for s in (b"num_paths", b"alignments", b"p->alignment")), msg
    assert np.all(out == 0)
