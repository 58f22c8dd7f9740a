"""Host checks of the factorised-blank path-score and expected-cost entry points (mrnnt_hat_path_* /
mrnnt_hat_expect_* and the mrnnt_cpu_ twins, include/mrnnt.h): the ten symbols exist beside an unchanged version 13;
a NULL or too small workspace, NULL grads, NULL alignments and a path stride below max T_b are each refused with
RNNT_STATUS_INVALID_VALUE before any device call; the two Python functions take blank_factorized last, default False,
and False gives the bits of a call without the keyword. No GPU needed."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "monotonic-rnnt_amd", "libmonotonic_rnnt_amd.so")
vp = ctypes.c_void_p

SYMBOLS = ["mrnnt_hat_path_forward", "mrnnt_hat_path_backward", "mrnnt_hat_path_backward_tracked",
           "mrnnt_hat_expect_forward", "mrnnt_hat_expect_backward", "mrnnt_hat_expect_backward_tracked",
           "mrnnt_cpu_hat_path_forward", "mrnnt_cpu_hat_path_backward", "mrnnt_cpu_hat_expect_forward",
           "mrnnt_cpu_hat_expect_backward"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "monotonic-rnnt_amd")], check=True)
    import _mrnnt_lib
    return _mrnnt_lib.load()


class Case:
    """A valid two-utterance problem on host buffers (the device pointers are never dereferenced: every call of
    these tests fails on the host)."""
    K, L = 2, 7

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
        self.al = np.zeros((2, self.K, self.L), np.int32)

    def need(self, lib, cpu, kind):
        n = ctypes.c_size_t(0)
        name = ("mrnnt_cpu_" if cpu else "mrnnt_") + kind + "_workspace_size"
        args = (self.K, ctypes.byref(n)) if kind == "path" else (ctypes.byref(n),)
        assert getattr(lib, name)(ctypes.byref(self.p), *args) == 0
        return n.value


def test_symbols_are_exported(lib):
    for name in SYMBOLS:
        assert getattr(lib, name, None) is not None, name
    assert lib.mrnnt_version() == 13  # an addition to version 13: callers probe for the symbols


def _call(lib, c, name, ws, ws_bytes, out=True, al=True, stride=None):
    """One of the ten entry points on Case c; out / al: pass the gradient buffer / the alignments (else NULL)."""
    fn = getattr(lib, name)
    cpu = name.startswith("mrnnt_cpu_")
    tail = 0 if cpu else None  # num_threads / stream
    o = vp(c.out.ctypes.data) if out else None
    p = ctypes.byref(c.p)
    if "_path_" in name:
        a = vp(c.al.ctypes.data) if al else None
        stride = c.L if stride is None else stride
        if name.endswith("forward"):
            return fn(p, ws, ws_bytes, a, c.K, stride, None, tail)
        if name.endswith("tracked"):
            return fn(p, ws, ws_bytes, a, c.K, stride, None, o, None, 0, tail)
        return fn(p, ws, ws_bytes, a, c.K, stride, None, o, tail)
    if name.endswith("forward"):
        return fn(p, ws, ws_bytes, None, None, None, None, 1, tail)
    if name.endswith("tracked"):
        return fn(p, ws, ws_bytes, None, None, None, None, o, None, 0, tail)
    return fn(p, ws, ws_bytes, None, None, None, None, o, tail)


def _kind(name):
    return "path" if "_path_" in name else "expect"


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_and_short_workspace_are_refused(lib, name):
    import _mrnnt_lib as L
    c = Case()
    need = c.need(lib, name.startswith("mrnnt_cpu_"), _kind(name))
    big = np.zeros(need, np.uint8)
    assert _call(lib, c, name, None, big.size) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace" in lib.mrnnt_last_error()
    assert _call(lib, c, name, vp(big.ctypes.data), need - 1) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace too small" in lib.mrnnt_last_error() and str(need).encode() in lib.mrnnt_last_error()
    assert not big.any() and not c.out.any()


@pytest.mark.parametrize("name", [s for s in SYMBOLS if "backward" in s])
def test_null_grads_are_refused(lib, name):
    import _mrnnt_lib as L
    c = Case()
    big = np.zeros(c.need(lib, name.startswith("mrnnt_cpu_"), _kind(name)), np.uint8)
    assert _call(lib, c, name, vp(big.ctypes.data), big.size, out=False) == L.RNNT_STATUS_INVALID_VALUE
    assert b"grads is null" in lib.mrnnt_last_error()
    assert not big.any()


@pytest.mark.parametrize("name", [s for s in SYMBOLS if "_path_" in s])
def test_null_alignments_and_short_path_stride_are_refused(lib, name):
    import _mrnnt_lib as L
    c = Case()
    big = np.zeros(c.need(lib, name.startswith("mrnnt_cpu_"), "path"), np.uint8)
    ws = vp(big.ctypes.data)
    assert _call(lib, c, name, ws, big.size, al=False) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignments" in lib.mrnnt_last_error()
    assert _call(lib, c, name, ws, big.size, stride=6) == L.RNNT_STATUS_INVALID_VALUE  # max T_b = 7
    assert b"stride" in lib.mrnnt_last_error()
    assert not big.any() and not c.out.any()


@pytest.mark.parametrize("fn", ["monotonic_rnnt_path_loss", "monotonic_rnnt_expected_cost"])
def test_blank_factorized_is_the_last_parameter_and_defaults_to_false(fn):
    import monotonic_rnnt_op as op
    params = list(inspect.signature(getattr(op, fn)).parameters.values())
    assert params[-1].name == "blank_factorized" and params[-1].default is False


def test_false_gives_the_bits_of_a_call_without_the_keyword():
    import monotonic_rnnt_op as op
    rng = np.random.default_rng(3)
    T, S = np.array([6, 4], np.int32), np.array([2, 4], np.int32)
    V, blank = 9, 4
    rows = int((T * (S + 1)).sum())
    acts = rng.standard_normal((rows, V)).astype(np.float32)
    labels = np.array([[1, 7, 0, 0], [2, 8, 3, 5]], np.int32)
    al = np.array([[[1, blank, 7, blank, blank, blank]], [[2, 8, 3, 5, blank, blank]]], np.int32)
    wb, we = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    t = torch.from_numpy

    def path(**kw):
        a = t(acts.copy()).requires_grad_(True)
        pc = op.monotonic_rnnt_path_loss(a, t(labels), t(T), t(S), t(al), blank_label=blank, **kw)
        pc.sum().backward()
        return pc.detach().numpy().tobytes(), a.grad.numpy().tobytes()

    def expect(**kw):
        a = t(acts.copy()).requires_grad_(True)
        e, c = op.monotonic_rnnt_expected_cost(a, t(labels), t(T), t(S), t(wb), t(we), blank_label=blank, **kw)
        (e + 0.5 * c).sum().backward()
        return e.detach().numpy().tobytes(), c.detach().numpy().tobytes(), a.grad.numpy().tobytes()

    assert path(blank_factorized=False) == path()
    assert expect(blank_factorized=False) == expect()
    assert path(blank_factorized=True)[0] != path()[0] and expect(blank_factorized=True)[0] != expect()[0]
    # the autograd functions take the flag as a trailing positional argument, default False
    a = t(acts.copy())
    old = op.MonotonicRNNTPathFunction.apply(a, t(labels), t(T), t(S), t(al), blank)
    assert old.numpy().tobytes() == path()[0]
    new = op.MonotonicRNNTPathFunction.apply(a, t(labels), t(T), t(S), t(al), blank, True)
    assert new.numpy().tobytes() == path(blank_factorized=True)[0]
