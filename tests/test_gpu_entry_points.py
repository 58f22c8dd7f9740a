"""The flat entry points called through ctypes, one problem each way: which launches each of them makes (counted
through the library's profile, so a launch that is not timed counts as none), and mrnnt_read_band with
device-resident lengths, which no other test reaches. Every entry point prepares the lattice offsets and the alignment
band in its own way -- device lengths, the setup kernel or a caller's lattice; timed or not -- and the counts pin
those ways down."""
import ctypes

import numpy as np
import pytest
import torch

import _align_checks as A
from test_gpu_chase import _launches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(23, 9), (17, 17), (12, 0)]
L_MAX = 23
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def op():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def problem(op):
    """(acts, labels, T, S) as numpy arrays and the unrestricted best path of mrnnt_align as a device tensor."""
    acts, labels, T, S = A.ragged(np.random.default_rng(21), SHAPES, 8)
    al, _ = op.monotonic_rnnt_align(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S))
    torch.cuda.synchronize()
    assert tuple(al.shape) == (3, L_MAX)
    return acts, labels, T, S, al


def _prepared(op, problem, device_lengths=False, aligned=False, dtype=None):
    acts, labels, T, S, al = problem
    a = _d(acts) if dtype is None else _d(acts).to(dtype)
    Tt, St = (_d(T), _d(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))
    prep = op._Prepared(a, _d(labels), Tt, St, al if aligned else None, 1 if aligned else 0, A.BLANK)
    prep.problem.lattice = None  # the library builds the offsets (with device lengths it always does)
    return prep


def _counts(fn):
    n = _launches(fn)
    torch.cuda.synchronize()
    return {k: v for k, v in n.items() if v}


def _forward(prep, ws, costs):
    import _mrnnt_lib as L
    st = L.load().mrnnt_forward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(costs.data_ptr()), 1,
                                prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS, L.load().mrnnt_last_error()


def _align(prep, ws, out, costs):
    import _mrnnt_lib as L
    st = L.load().mrnnt_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(out.data_ptr()), L_MAX,
                              vp(costs.data_ptr()), prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS, L.load().mrnnt_last_error()


@pytest.mark.parametrize("call,kw,expected", [
    ("forward", {}, {"setup": 1, "chase": 1}),
    ("forward", {"dtype": torch.bfloat16}, {"setup": 1, "log_softmax": 1, "alpha_beta": 1}),
    ("forward", {"device_lengths": True}, {"chase": 1}),
    ("forward", {"device_lengths": True, "aligned": True}, {"setup": 1, "band": 1, "log_softmax": 1, "alpha_beta": 1}),
    ("align", {}, {"setup": 1, "log_softmax": 1, "alpha_beta": 1}),
    ("align", {"aligned": True}, {"setup": 1, "band": 1, "log_softmax": 1, "alpha_beta": 1}),
], ids=["forward", "forward_bf16", "forward_device_lengths", "forward_device_lengths_aligned", "align",
        "align_aligned"])
def test_launches_of_forward_and_align(op, problem, call, kw, expected):
    prep = _prepared(op, problem, **kw)
    ws = prep.workspace()
    costs = torch.empty(3, dtype=torch.float32, device=DEV)
    out = torch.empty((3, L_MAX), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    if call == "forward":
        got = _counts(lambda: _forward(prep, ws, costs))
    else:
        got = _counts(lambda: _align(prep, ws, out, costs))
    assert got == expected
    assert bool(torch.isfinite(costs).all())
    op.check_lengths()


def test_launches_of_posteriors_and_read_band(op, problem):
    import _mrnnt_lib as L
    lib = L.load()
    prep = _prepared(op, problem)
    ws = prep.workspace()
    costs = torch.empty(3, dtype=torch.float32, device=DEV)
    _forward(prep, ws, costs)
    N = problem[0].shape[0]
    bp = torch.empty(N, dtype=torch.float32, device=DEV)
    lp = torch.empty(N, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()

    def posteriors():
        st = lib.mrnnt_posteriors(ctypes.byref(prep.problem), vp(ws.data_ptr()), vp(bp.data_ptr()), vp(lp.data_ptr()),
                                  None, 0, None, 0, prep.stream())
        assert st == L.RNNT_STATUS_SUCCESS, lib.mrnnt_last_error()

    assert _counts(posteriors) == {"alpha_beta": 1}
    assert bool(torch.isfinite(bp).all()) and bool(torch.isfinite(lp).all())
    for kw in ({}, {"aligned": True}, {"device_lengths": True, "aligned": True}):
        band = _prepared(op, problem, **kw)
        bws = band.workspace()
        mn = torch.empty((3, L_MAX), dtype=torch.int32, device=DEV)
        mx = torch.empty((3, L_MAX), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

        def read_band():
            st = lib.mrnnt_read_band(ctypes.byref(band.problem), vp(bws.data_ptr()), vp(mn.data_ptr()),
                                     vp(mx.data_ptr()), L_MAX, band.stream())
            assert st == L.RNNT_STATUS_SUCCESS, lib.mrnnt_last_error()

        assert _counts(read_band) == {}, kw  # its setup and band launches are not timed
    op.check_lengths()


def test_launches_of_joint_forward():
    import monotonic_rnnt_joint as J
    from test_gpu_joint import make_case
    H, V = 128, 64  # the smallest case of tests/test_gpu_joint.py
    enc, pred, w, bias, labels, T, S = make_case(H + V, 3, (1, 24), 8, H, V)
    jp = J._JointPrepared(enc.to(DEV), pred.to(DEV), w.to(DEV), bias.to(DEV), torch.from_numpy(labels).to(DEV),
                          torch.from_numpy(T), torch.from_numpy(S), 0)
    torch.cuda.synchronize()
    out = []
    got = _counts(lambda: out.append(jp.forward(False)))
    assert got == {"setup": 1, "joint_fwd": 1, "alpha_beta": 1}
    assert bool(torch.isfinite(out[0][0]).all())


def test_read_band_device_lengths_equals_host_lengths(op, problem):
    """mrnnt_read_band with lengths_on_device: the band of the alignment with max_shift = 1 is element for element the
    band the host-lengths call builds in the same workspace, and the call leaves the status word alone."""
    import _mrnnt_lib as L
    lib = L.load()
    T, S = problem[2], problem[3]
    host = _prepared(op, problem, aligned=True)
    dyn = _prepared(op, problem, device_lengths=True, aligned=True)
    assert dyn.problem.lengths_on_device == 1 and dyn.problem.status_host
    wh, wd = host.workspace(), dyn.workspace()
    ws = wh if wh.numel() >= wd.numel() else wd  # one workspace large enough for either plan
    op.check_lengths()
    status = op._status_word()
    before = int(status[0])
    res = []
    for prep in (host, dyn):
        mn = torch.full((3, L_MAX), -7, dtype=torch.int32, device=DEV)
        mx = torch.full((3, L_MAX), -7, dtype=torch.int32, device=DEV)
        st = lib.mrnnt_read_band(ctypes.byref(prep.problem), vp(ws.data_ptr()), vp(mn.data_ptr()), vp(mx.data_ptr()),
                                 L_MAX, prep.stream())
        assert st == L.RNNT_STATUS_SUCCESS, lib.mrnnt_last_error()
        torch.cuda.synchronize()
        res.append((mn.cpu().numpy(), mx.cpu().numpy()))
    assert int(status[0]) == before
    (hmn, hmx), (dmn, dmx) = res
    assert np.array_equal(dmn, hmn) and np.array_equal(dmx, hmx)
    # the band is a real one: the reference's band of the alignment, 0 / S_b past T_b
    al = problem[4].cpu().numpy()
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        lo, hi = A.band_of(al[b], int(Tb), 1)
        assert np.array_equal(hmn[b, :Tb], lo) and np.array_equal(hmx[b, :Tb], hi), b
        assert np.all(hmn[b, Tb:] == 0) and np.all(hmx[b, Tb:] == Sb), b
