"""monotonic_rnnt_joint_expected_cost (mrnnt_joint_expect_*: the joint pass, the expectation recursion, the coefficient
launch of mrnnt_expect.hip, the expect-live row list of mrnnt_joint_rows.hip and the MFMA gradient pass of
mrnnt_joint.hip) against the
yardstick of tests/_joint_expect_checks.py -- the fp64 composition the fused op replaces, from the same bf16 inputs --
and against the library's own read-outs and unfused twin.

Tolerances (tests/_joint_expect_checks.py): costs within 1e-5 max(1, |c|); each gradient tensor within
1.5e-2 max|ref| + 1e-5; expected within COST_TOL + (4e-6 + 2e-5 max(1, |cost_b|)) W_b. Where a result must not change at
all, the comparison is bitwise. Measured maxima: profiles/joint_expect/README.md.
"""
import functools

import numpy as np
import pytest
import torch

import _align_checks as A
import _expect_checks as EC
import _joint_expect_checks as JE
import _joint_path_checks as JC
from _parity import COST_TOL

pytestmark = pytest.mark.gpu

NAMES = ("d_enc", "d_pred", "d_weight", "d_bias")
# wide: S + 1 = 71 > 64 (the list and the coefficient kernel take a second 64-lane step), more than 256 live rows (the
# backward's workgroup), a T = 1 utterance, a single-path S = T utterance; t65: one frame past a 64-frame block
SHAPES = {"wide": [(130, 70), (1, 0), (33, 33)], "t65": [(65, 23), (1, 0), (40, 40)]}


@pytest.fixture(scope="module")
def jm():
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Problem:
    """Inputs, their host logits, packed cost arrays and their grid, signed upstreams: computed once per (H, V, shapes)
    and shared, unchanged, by the tests that need them."""

    def __init__(self, H, V, shapes, costs="random"):
        self.blank = V - 1 if (H, V) == (256, 100) else 0
        enc, pred, w, bias, labels, T, S = JC.make_case(H + V + len(shapes), SHAPES[shapes], H, V, self.blank)
        if (H, V) == (128, 64):
            bias = None
        self.case = (enc, pred, w, bias, labels, T, S)
        self.T, self.S = T, S
        self.logits = JC.joint_logits(enc, pred, w, bias, T, S)
        rng = np.random.default_rng(H + V)
        self.wb, self.we = JE.random_costs(rng, T, S) if costs == "random" else EC.latency_costs(T, S)
        self.ge, self.gc = EC.upstreams(rng, len(T))
        # the grid of the enc / pred slots; strictly larger than that at (640, 130)
        extra = 2 if (H, V) == (640, 130) else 0
        self.grid_shape = (enc.size(1) + extra, pred.size(1) + extra)
        assert self.grid_shape[0] > int(T.max()) and self.grid_shape[1] > int(S.max()) + 1
        self.wbg, self.weg = JE.grid(self.wb, self.we, T, S, *self.grid_shape)
        self.W = EC.cost_bound(self.wb, self.we, T, S)

    def yardstick(self, ge, gc, bands=None):
        enc, pred, w, bias, labels, T, S = self.case
        return JE.yardstick(enc, pred, w, bias, labels, T, S, self.wb, self.we, ge, gc, self.blank, self.logits, bands)


@functools.lru_cache(maxsize=None)
def problem(H, V, shapes, costs="random"):
    return Problem(H, V, shapes, costs)


@functools.lru_cache(maxsize=None)
def parity_reference(H, V, shapes):
    p = problem(H, V, shapes)
    return p.yardstick(p.ge, p.gc)


def _d(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def on(dev, enc, pred, w, bias, labels, T, S):
    return (enc.to(dev), pred.to(dev), w.to(dev), None if bias is None else bias.to(dev),
            torch.from_numpy(labels).to(dev), torch.from_numpy(T), torch.from_numpy(S))


def run(jm, dev, case, wbg, weg, ge=None, gc=None, blank=0, alignment=None, k=0, capturable=None):
    """(expected fp32 numpy [B], costs fp32 numpy [B], d_enc, d_pred, d_weight, d_bias or None) of one forward and ONE
    backward of sum_b ge[b] expected[b] + gc[b] costs[b] (None: ones)."""
    enc, pred, w, bias, lab, T, S = on(dev, *case)
    B = len(T)
    leaves = [x.requires_grad_(True) for x in (enc, pred, w)] + ([] if bias is None else [bias.requires_grad_(True)])
    e, c = jm.monotonic_rnnt_joint_expected_cost(enc, pred, w, bias, lab, T, S, _d(wbg, dev), _d(weg, dev), blank,
                                                 _d(alignment, dev), k, capturable)
    for x in (e, c):
        assert x.dtype == torch.float32 and tuple(x.shape) == (B,) and x.requires_grad
    one = np.ones(B, np.float32)
    torch.autograd.backward((e, c), (_d(np.asarray(one if ge is None else ge, np.float32), dev),
                                     _d(np.asarray(one if gc is None else gc, np.float32), dev)))
    torch.cuda.synchronize()
    grads = [x.grad for x in leaves] + ([None] if bias is None else [])
    for x, like in zip(grads, (enc, pred, w, bias)):
        assert x is None or (x.dtype == like.dtype and x.shape == like.shape)
    return (e.detach().cpu().numpy(), c.detach().cpu().numpy()) + tuple(grads)


def check_vs_yardstick(got, ref, p, need_grads=True):
    JC.assert_costs(got[1], ref[1])
    JE.assert_expected(got[0], ref[0], ref[1], p.W)
    for x, r, name in zip(got[2:], ref[2:], NAMES):
        if x is not None:
            if need_grads:
                assert float(r.abs().max()) > 1e-3, name  # something is compared
            JC.close(x, r, name)
    de, dp = got[2], got[3]
    for b in range(len(p.T)):  # padding frames / label slots: exactly zero
        assert torch.all(de[b, p.T[b]:] == 0) and torch.all(dp[b, p.S[b] + 1:] == 0)


def same_bits(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for x, y, name in zip(a[2:], b[2:], NAMES):
        assert (x is None and y is None) or torch.equal(x, y), name


# 1. parity: both MFMA tiles (H <= 512 / H = 640), V % 4 != 0, blank = V - 1 at (256, 100), no bias at (128, 64), the
# grid strictly larger than the enc / pred slots at (640, 130)
@pytest.mark.parametrize("shapes", ["wide", "t65"])
@pytest.mark.parametrize("H,V", [(128, 64), (256, 100), (512, 256), (640, 130)])
def test_parity_vs_yardstick(jm, dev, H, V, shapes):
    p = problem(H, V, shapes)
    got = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank)
    check_vs_yardstick(got, parity_reference(H, V, shapes), p)


# 2. g_c = 0 with latency costs (integers: every sum of the single-path utterances is exact)
def test_single_path_utterances_get_exactly_nothing(jm, dev):
    p = problem(256, 128, "wide", costs="latency")
    B = len(p.T)
    ge, zero = np.array([1.0, -2.0, 0.5], np.float32), np.zeros(B, np.float32)
    got = run(jm, dev, p.case, p.wbg, p.weg, ge, zero)
    check_vs_yardstick(got, p.yardstick(ge, zero), p)
    assert float(got[2][0].abs().max()) > 0  # (utterance 0 has paths to tell apart)
    for b in (1, 2):  # S = 0, S = T: one path, no deviation from the mean
        assert torch.all(got[2][b] == 0) and torch.all(got[3][b] == 0), b
    # only such utterances: the row list is empty, and every gradient is exactly zero
    enc, pred, w, bias, labels, T, S = p.case
    only = (enc[1:], pred[1:], w, bias, labels[1:], T[1:], S[1:])
    assert p.wbg is None  # (latency: no blank costs)
    got = run(jm, dev, only, None, p.weg[1:], ge[1:], zero[1:])
    want = np.array([0.0, float(sum(range(33)))], np.float32)  # label s is emitted at frame s
    assert np.array_equal(got[0], want), got[0]
    for x, name in zip(got[2:], NAMES):
        assert torch.all(x == 0), name
    prep = jm._JointPrepared(*on(dev, *only), 0)
    wb, we, gT, gS1 = prep.cost_grid(None, _d(p.weg[1:], dev))
    _, _, ws = prep.expect_forward(wb, we, gT, gS1, True)
    assert int(prep.expect_rows(ws, wb, we, gT, gS1, _d(ge[1:], dev), None).item()) == 0
    assert int(prep.expect_rows(ws, wb, we, gT, gS1, _d(ge[1:], dev), _d(ge[1:], dev)).item()) == 1 + 33


# 3. a constant cost on both arcs: every path costs c T_b
def test_constant_costs(jm, dev):
    p = problem(256, 128, "wide", costs="latency")
    cval = np.array([0.375, -2.5, 3.0], np.float32)
    g = np.broadcast_to(cval[:, None, None], (len(p.T),) + p.grid_shape).astype(np.float32)
    e = run(jm, dev, p.case, g, g, None, np.zeros(len(p.T), np.float32))[0]
    want = (cval.astype(np.float64) * p.T).astype(np.float32)
    print("constant costs:", e, want)
    assert np.all(np.abs(e.astype(np.float64) - want) <= np.spacing(np.abs(want))), (e, want)


# 4. consistency with the library's own read-outs and the unfused twin
def test_consistent_with_loss_posteriors_and_unfused_twin(jm, dev):
    import monotonic_rnnt_op as op
    p = problem(256, 100, "wide")
    enc, pred, w, bias, labels, T, S = p.case
    args = on(dev, *p.case)
    assert p.grid_shape == (enc.size(1), pred.size(1))  # the posteriors' grid
    wbg, weg = _d(p.wbg, dev), _d(p.weg, dev)
    e, c = jm.monotonic_rnnt_joint_expected_cost(*args, wbg, weg, blank_label=p.blank)
    assert not e.requires_grad and not c.requires_grad  # (no gradient asked for: the A direction alone)
    loss = jm.monotonic_rnnt_joint_loss(*args, blank_label=p.blank)
    assert torch.equal(c, loss)
    got = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank)
    assert got[1].tobytes() == loss.cpu().numpy().tobytes()
    assert np.all(np.abs(got[0].astype(np.float64) - e.cpu().numpy()) <= COST_TOL + 4e-6 * p.W)
    post = jm.monotonic_rnnt_joint_posteriors(*args, blank_label=p.blank)
    pb, pe = post.blank.double(), post.label.double()
    z = torch.zeros_like(pb)
    rows = torch.where(pb != 0, pb * wbg.double(), z) + torch.where(pe != 0, pe * weg.double(), z)
    ref = rows.sum((1, 2)).cpu().numpy()
    err = np.abs(e.cpu().numpy().astype(np.float64) - ref)
    print("expected vs posteriors: max err / tol", float((err / (4e-6 * p.W + COST_TOL)).max()))
    assert np.all(err <= 4e-6 * p.W + COST_TOL), (err, p.W)
    acts = torch.from_numpy(p.logits[1]).to(dev)
    te, tc = op.monotonic_rnnt_expected_cost(acts, args[4], args[5], args[6], _d(p.wb, dev), _d(p.we, dev),
                                             blank_label=p.blank)
    JE.assert_expected(e.cpu().numpy(), te.cpu().numpy().astype(np.float64), tc.cpu().numpy().astype(np.float64), p.W,
                       "expected vs unfused twin")
    JC.assert_costs(c.cpu().numpy(), tc.cpu().numpy().astype(np.float64))


# 5. g_e = 0: the loss's own backward
def test_zero_expected_upstream_is_the_loss_backward(jm, dev):
    p = problem(512, 256, "t65")
    zero = np.zeros(len(p.T), np.float32)
    got = run(jm, dev, p.case, p.wbg, p.weg, zero, p.gc, p.blank)
    leaves = [x.requires_grad_(True) for x in on(dev, *p.case)[:4]]
    loss = jm.monotonic_rnnt_joint_loss(*leaves, *on(dev, *p.case)[4:], blank_label=p.blank)
    loss.backward(_d(p.gc, dev))
    torch.cuda.synchronize()
    assert got[1].tobytes() == loss.detach().cpu().numpy().tobytes()
    for x, leaf, name in zip(got[2:], leaves, NAMES):
        assert float(leaf.grad.abs().max()) > 1e-3, name
        JC.close(x, leaf.grad.double().cpu(), name)


# 6. restricting alignment: the expectation under the restricted distribution
@pytest.mark.parametrize("shapes", ["wide", "t65"])
def test_restricting_alignment(jm, dev, shapes):
    p = problem(256, 100, shapes)
    args = on(dev, *p.case)
    al, _ = jm.monotonic_rnnt_joint_align(*args, blank_label=p.blank)
    al = al.cpu().numpy()
    k = 2
    bands = [A.band_of(al[b], int(p.T[b]), k, p.blank) for b in range(len(p.T))]
    ref = p.yardstick(p.ge, p.gc, bands)
    free = parity_reference(256, 100, shapes)
    assert ref[1][0] > free[1][0] + 1e-3  # (the band removed paths of utterance 0)
    got = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank, alignment=al, k=k)
    check_vs_yardstick(got, ref, p)
    loss = jm.monotonic_rnnt_joint_loss(*args, blank_label=p.blank, alignment=_d(al, dev),
                                        max_distance_from_alignment=k)
    assert got[1].tobytes() == loss.cpu().numpy().tobytes()


# 7. bitwise behaviour
@pytest.mark.parametrize("H,V", [(256, 100), (640, 130)])
def test_bitwise_reproducible_batch_independent(jm, dev, H, V):
    p = problem(H, V, "wide")
    first = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank)
    same_bits(first, run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank))
    enc, pred, w, bias, labels, T, S = p.case
    # utterance 0 without a finite cost: its own values NaN, the others' untouched
    bad = enc.clone()
    bad[0] = float("nan")
    got = run(jm, dev, (bad, pred, w, bias, labels, T, S), p.wbg, p.weg, p.ge, p.gc, p.blank)
    assert np.isnan(got[0][0]) and np.isnan(got[1][0])
    assert got[0][1:].tobytes() == first[0][1:].tobytes() and got[1][1:].tobytes() == first[1][1:].tobytes()
    assert torch.isnan(got[2][0, : T[0]]).all() and torch.isfinite(got[2][1:]).all()  # its rows are listed, as NaN
    # a permuted batch: the permuted values
    perm = np.array([2, 0, 1])
    case = (enc[perm], pred[perm], w, bias, labels[perm], T[perm], S[perm])
    got = run(jm, dev, case, p.wbg[perm], p.weg[perm], p.ge[perm], p.gc[perm], p.blank)
    assert got[0].tobytes() == first[0][perm].tobytes() and got[1].tobytes() == first[1][perm].tobytes()


# 8. capturable
def _step(jm, leaves, lab, T, S, wbg, weg, ups, capturable):
    for x in leaves:
        x.grad = None
    e, c = jm.monotonic_rnnt_joint_expected_cost(*leaves, lab, T, S, wbg, weg, capturable=capturable)
    torch.autograd.backward((e, c), ups)
    return (e.detach().clone(), c.detach().clone()) + tuple(x.grad.clone() for x in leaves)


@pytest.mark.parametrize("H,V", [(256, 128), (640, 130)])
def test_capturable_and_graph_capture_replay(jm, dev, H, V):
    p = problem(H, V, "t65")
    assert p.blank == 0 and p.case[3] is not None
    got = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, capturable=True)
    check_vs_yardstick(got, parity_reference(H, V, "t65"), p)
    enc, pred, w, bias, lab, T, S = on(dev, *p.case)
    wbg, weg, ups = _d(p.wbg, dev), _d(p.weg, dev), (_d(p.ge, dev), _d(p.gc, dev))
    leaves = [x.requires_grad_(True) for x in (enc, pred, w, bias)]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any device-to-host read in the capturable step raises
    try:
        _step(jm, leaves, lab, T, S, wbg, weg, ups, True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    # capture (warm-up on a side stream first, as torch.cuda.graph asks), then replay on new inputs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _step(jm, leaves, lab, T, S, wbg, weg, ups, None)
    torch.cuda.current_stream().wait_stream(s)
    for x in leaves:
        x.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e, c = jm.monotonic_rnnt_joint_expected_cost(*leaves, lab, T, S, wbg, weg)  # capturable inside capture
        torch.autograd.backward((e, c), ups)
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(2):
        with torch.no_grad():
            leaves[0].copy_(torch.randn(enc.shape, device=dev, generator=gen).to(enc.dtype))
            leaves[1].copy_(torch.randn(pred.shape, device=dev, generator=gen).to(pred.dtype))
        g.replay()
        torch.cuda.synchronize()
        got = (e.detach().clone(), c.detach().clone()) + tuple(x.grad.clone() for x in leaves)
        fresh = [x.detach().clone().requires_grad_(True) for x in leaves]
        ref = _step(jm, fresh, lab, T, S, wbg, weg, ups, True)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


# 9. cost-array edge cases
def test_absent_cost_arrays_and_never_read_slots(jm, dev):
    p = problem(256, 100, "t65")
    ref = run(jm, dev, p.case, p.wbg, p.weg, p.ge, p.gc, p.blank)
    # other garbage (NaN, -inf, huge of the other sign) where the contract says nothing is read
    for garbage in (np.nan, -np.inf, -3e38):
        wbg, weg = JE.grid(p.wb, p.we, p.T, p.S, *p.grid_shape, garbage=garbage)
        same_bits(ref, run(jm, dev, p.case, wbg, weg, p.ge, p.gc, p.blank))
    # None is an array of zeros (in the read slots; garbage elsewhere), bit for bit
    zb, ze = JE.grid(0 * p.wb, 0 * p.we, p.T, p.S, *p.grid_shape)
    for x, y, xz, yz in ((None, p.weg, zb, p.weg), (p.wbg, None, p.wbg, ze), (None, None, zb, ze)):
        got = run(jm, dev, p.case, x, y, p.ge, p.gc, p.blank)
        same_bits(got, run(jm, dev, p.case, xz, yz, p.ge, p.gc, p.blank))
    assert np.all(got[0] == 0.0)
    # the shapes the surface refuses
    args = on(dev, *p.case)
    small = torch.zeros(len(p.T), int(p.T.max()) - 1, p.grid_shape[1], device=dev)
    with pytest.raises(RuntimeError, match="grid_T"):
        jm.monotonic_rnnt_joint_expected_cost(*args, small, None, p.blank)
    wider = torch.zeros(len(p.T), p.grid_shape[0], p.grid_shape[1] + 1, device=dev)
    with pytest.raises(RuntimeError, match="same shape"):
        jm.monotonic_rnnt_joint_expected_cost(*args, _d(p.wbg, dev), wider, p.blank)
