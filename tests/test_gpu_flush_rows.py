"""The flush-dead rows of the loss gradient on the MI355X (mrnnt_host.h kFlushLog2): a row whose every exp2 argument
is below -126 - 2^-6 and whose two corrections are 0 is stored as zero_row_value without reading acts, because the raw
v_exp_f32 returns +0 there. Tuning occ_skip: 0 no skip, 2 the occupancy threshold alone (e^-110), 1 both (the product).

  test_exp2_probe        the hardware fact everything else rests on (devtools mrnnt_exp2_probe)
  test_bit_identity      gradients and costs across occ_skip 0 / 2 / 1, bit for bit, and against the oracle
  test_live_row_count    mrnnt_grad_live_rows pinned from both sides by the oracle's fp64 occupancies
  test_den_bound_*       max_v z + den, the eps of the proof, for every log-softmax form, at the offset 1e4 (<= 1e-6)
                         and across a binade of max * kLog2e (the rule's slack); test_bit_identity_at_large_offsets
  test_non_finite        NaN logit, ll = -inf, NaN grad_output: the full path, bit-identical
  test_row_state         flush-dead rows are zero rows of the row state (mrnnt_backward_tracked) and are not rewritten

Shapes: seeded normal logits x scale, each scaled utterance with rows of log-occupancy in [-110, -87.6) -- counted per
case from the oracle's fp64 alpha / beta and required to be >= 100, so no case can pass without rows the rule decides
-- and an S = 0 utterance, which has none. V = 64 (4 rows per wave), 1024 (1 row per wave), 1001 (the scalar kernel)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
from _flush_rows import log_occupancy, window_rows
from _parity import GRAD_TOL, assert_costs, assert_grads, band_mask, knobs

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# the oracle runs on the upcast inputs; what is left is the rounding of the stored gradient: relative, on top of the
# absolute tolerance of _parity (bf16 as tests/test_gpu_parity.py has it; fp16: half an ulp, 2^-11)
GRAD_REL = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# name: V, [(T, S, logit scale)]; grad_output = SCALE per utterance, and SCALE[1] alone in the stride-0 form
BATCHES = {
    "v64": (64, [(400, 80, 3.0)] * 4 + [(23, 0, 3.0)]),
    "v1024": (1024, [(200, 60, 1.0)] + [(120, 30, 3.0)] * 3 + [(9, 0, 1.0)]),
    "v1001": (1001, [(120, 30, 3.0)] * 4 + [(9, 0, 3.0)]),
}
SCALE = [1.0, -0.5, 2.0, 0.0, 1.0]
_CACHE = {}


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


@pytest.fixture(scope="module")
def L():
    import _mrnnt_lib
    return _mrnnt_lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Data:
    """One batch in one element type: the inputs on the device and, computed once, the oracle's costs, gradient and
    occupancy counts on the inputs as the device holds them (upcast)."""

    def __init__(self, dev, batch, dtype, seed=606, utts=None, V=None, edit=None):
        if utts is None:
            V, utts = BATCHES[batch]
        rng = np.random.default_rng(seed)
        self.T = np.array([u[0] for u in utts], np.int32)
        self.S = np.array([u[1] for u in utts], np.int32)
        self.V, self.dtype, self.dev = V, dtype, dev
        n = self.T * (self.S + 1)
        mul = np.repeat(np.array([u[2] for u in utts], np.float32), n)[:, None]
        acts = rng.standard_normal((int(n.sum()), V)).astype(np.float32) * mul
        self.labels_np = rng.integers(1, V, (len(utts), max(1, int(self.S.max())))).astype(np.int32)
        self.utt = np.repeat(np.arange(len(utts)), n)
        if edit is not None:
            edit(self, acts)
        self.acts = torch.from_numpy(acts).to(dev).to(dtype)
        self.up = self.acts.float().cpu().numpy()
        self.labels = torch.from_numpy(self.labels_np).to(dev)
        self.cr, self.gr, _, self.al, self.be = O.oracle_rnnt(self.up, self.labels_np, self.T, self.S, num_threads=8,
                                                              debug=True)
        self.win = window_rows(self.al, self.be, self.cr, self.T, self.S)
        self.above = sum(window_rows(self.al, self.be, self.cr, self.T, self.S, lo=-87.0, hi=np.inf))
        self.band = int(band_mask(self.T, self.S).sum())

    def prepared(self, op):
        return op._Prepared(self.acts, self.labels, torch.from_numpy(self.T), torch.from_numpy(self.S), None, 0, 0)


def data(dev, batch, name):
    key = (batch, name)
    if key not in _CACHE:
        d = _CACHE[key] = Data(dev, batch, DTYPES[name])
        print(f"{batch} {name}: rows in [-110, -87.6) per utterance {d.win}, >= -87.0: {d.above}, band {d.band}")
    d = _CACHE[key]
    # the guard: the case has rows the flush rule decides, in every scaled utterance; the S = 0 utterance has none
    assert sum(d.win) >= 100 and min(d.win[:-1]) >= 50 and d.win[-1] == 0, d.win
    return d


def backward(L, prep, ws, scale, broadcast=False, state=None, grads=None):
    """mrnnt_backward (mrnnt_backward_tracked with a state) of the current library into a NaN-filled buffer."""
    if grads is None:
        grads = torch.full_like(prep.acts, float("nan"))
    prep.problem.grad_scale_broadcast = 1 if broadcast else 0
    lib, p = L.load(), ctypes.byref(prep.problem)
    if state is None:
        L.check(lib.mrnnt_backward(p, vp(ws), vp(scale), vp(grads), prep.stream()), "backward")
    else:
        L.check(lib.mrnnt_backward_tracked(p, vp(ws), vp(scale), vp(grads), vp(state), state.numel(), prep.stream()),
                "backward_tracked")
    torch.cuda.synchronize()
    return grads


def live_rows(L, prep, ws):
    cnt = torch.zeros(1, dtype=torch.int64, device=prep.device)
    L.check(L.load().mrnnt_grad_live_rows(ctypes.byref(prep.problem), vp(ws), vp(cnt), prep.stream()), "grad_live_rows")
    return int(cnt.item())


# ---------------------------------------------------------------------------------------------------------------------

def exp2_probe(L, dev, x_np):
    x = torch.from_numpy(x_np).to(dev)
    y = torch.full_like(x, float("nan"))
    rc = L.devtools().mrnnt_exp2_probe(vp(x), vp(y), x.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_exp2_probe(L, dev):
    """Every fp32 in [-150, -126] (1,703,937 values; the bit patterns of negative floats ascend with the magnitude):
    the raw v_exp_f32 returns exactly +0 for x <= -126 - 2^-6 and a normal positive number for x >= -126. Arguments
    further down, which a dead row also produces, return +0 as well."""
    lo, hi = np.float32(-126.0).view(np.uint32), np.float32(-150.0).view(np.uint32)
    x = np.arange(int(lo), int(hi) + 1, dtype=np.uint32).view(np.float32)
    assert x.size == 1703937 and x[0] == -126.0 and x[-1] == -150.0
    y = exp2_probe(L, dev, x)
    bits = y.view(np.uint32)
    flush = x <= np.float32(-126.0 - 2.0 ** -6)
    tiny = np.finfo(np.float32).tiny
    top = x >= np.float32(-126.0)
    print(f"x <= -126 - 2^-6: {int(flush.sum())} inputs, {int((bits[flush] != 0).sum())} outputs not +0; "
          f"exp2(-126) = {y[0]!r}; between: {int((bits[~flush & ~top] != 0).sum())} of {int((~flush & ~top).sum())} "
          f"outputs not +0")
    assert np.all(bits[flush] == 0), (x[flush][bits[flush] != 0][:8], bits[flush][bits[flush] != 0][:8])
    assert np.all(y[top] >= tiny) and np.all(np.isfinite(y[top]))
    far = np.array([-150.5, -151.0, -160.0, -200.0, -300.0, -1000.0, -1e4, -1e10, -3e38, -np.inf], np.float32)
    assert np.all(exp2_probe(L, dev, far).view(np.uint32) == 0)
    # the rows just above the edge are not flushed: normal numbers from -126 up
    near = np.linspace(-126.0, -125.0, 1025).astype(np.float32)
    assert np.all(exp2_probe(L, dev, near) >= tiny)


@pytest.mark.parametrize("grad_variant", [0, 2, 3, 5, 6])
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("batch", list(BATCHES))
def test_bit_identity(op, L, dev, batch, name, grad_variant):
    """Costs and gradients across occ_skip 0 / 2 / 1, signed zeros included, with grad_output (1, -0.5, 2, 0, 1) per
    utterance and -0.5 in the stride-0 broadcast form; the product's result against the oracle."""
    d = data(dev, batch, name)
    vec = torch.tensor(SCALE, dtype=torch.float32, device=dev)
    one = torch.tensor(SCALE[1:2], dtype=torch.float32, device=dev)
    out = {}
    with knobs(grad_variant=grad_variant):
        for skip in (0, 2, 1):
            with knobs(occ_skip=skip):
                prep = d.prepared(op)
                costs, ws = op._forward(prep, with_beta=True)
                out[skip] = (costs.view(torch.int32).clone(), backward(L, prep, ws, vec).view(INT[d.dtype]),
                             backward(L, prep, ws, one, broadcast=True).view(INT[d.dtype]))
    for skip in (2, 1):
        for i, what in enumerate(("costs", "grads", "grads, broadcast grad_output")):
            assert torch.equal(out[0][i], out[skip][i]), (what, skip)
    assert_costs(out[1][0].view(torch.float32).cpu().numpy(), d.cr)
    g = out[1][1].view(d.dtype).float().cpu().numpy()
    ref = d.gr * np.asarray(SCALE)[d.utt][:, None]
    assert np.isfinite(g).all()
    err = float((np.abs(g - ref) - GRAD_REL[d.dtype] * np.abs(ref)).max())
    assert err <= GRAD_TOL, err
    if d.dtype == torch.float32:  # row (t, s) = (0, 1) of utterance 0 is out of band: -0 under -0.5, +0 under 1
        assert bool((out[1][2][1] == torch.iinfo(torch.int32).min).all()) and bool((out[1][1][1] == 0).all())


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("batch", list(BATCHES))
def test_live_row_count(op, L, dev, batch, name):
    """live(occ_skip = 2) - live(1) >= the rows with -110 <= log-occupancy < -87.6 (a quarter nat inside the true edge
    -126.015625 ln 2 = -87.35), and live(1) >= the rows at or above -87.0: the count is pinned from both sides without
    leaning on rows within rounding of the edge. live(0) is the band."""
    d = data(dev, batch, name)
    live = {}
    for skip in (0, 2, 1):
        with knobs(occ_skip=skip):
            prep = d.prepared(op)
            _, ws = op._forward(prep, with_beta=True)
            live[skip] = live_rows(L, prep, ws)
    print(f"{batch} {name}: live rows {live}, window {sum(d.win)}, >= -87.0: {d.above}")
    assert live[0] == d.band
    assert live[2] - live[1] >= sum(d.win), (live, d.win)
    assert live[1] >= d.above, (live, d.above)
    prep = d.prepared(op)  # the product library counts as occ_skip = 1
    _, ws = op._forward(prep, with_beta=True)
    assert live_rows(L, prep, ws) == live[1]


# ---------------------------------------------------------------------------------------------------------------------
# the eps of the proof: z <= -den + eps for every element of a reduced row

def _den_inputs(dev, V, dtype, lengths, seed, offset=1.0e4):
    """Normal logits x 3 with rows offset by `offset`, rows with one dominant logit (the sum is exactly 1) and both."""
    T, S = (np.asarray(x, np.int32) for x in lengths)
    g = torch.Generator().manual_seed(seed)
    n = int(np.sum(T * (S + 1)))
    acts = torch.randn(n, V, generator=g) * 3.0
    acts[1::5] += offset
    acts[2::7] = -60.0 + torch.randn(acts[2::7].shape, generator=g)
    acts[2::7, 3] = 60.0  # every other term is below e^-110: sum = 1 exactly
    acts[3::11, V - 1] += offset
    labels = torch.randint(1, V, (T.size, max(1, int(S.max()))), generator=g, dtype=torch.int32)
    return acts.to(dev).to(dtype), labels.to(dev), T, S


def _assert_den_bound(op, L, acts, labels, T, S, what, flat=True):
    """eps = max_v z + den on every in-band row. Always: eps log2(e) <= half of flush_eps_log2(den, V), the slack the
    rule adds (mrnnt_host.h). flat: eps <= 1e-6 as well, which holds where the rounding error of max * kLog2e, times
    ln 2 and the row's chunks, stays under half an ulp of max: single-chunk rows at offsets up to 1e4."""
    prep = op._Prepared(acts, labels, torch.from_numpy(T), torch.from_numpy(S), None, 0, 0)
    _, ws = op._forward(prep, with_beta=True)
    den = torch.empty(acts.size(0), dtype=torch.float32, device=acts.device)
    L.check(L.load().mrnnt_read_denoms(ctypes.byref(prep.problem), vp(ws), vp(den), prep.stream()), "read_denoms")
    torch.cuda.synchronize()
    band = torch.from_numpy(band_mask(T, S)).to(acts.device)
    V = acts.size(1)
    eps = (acts.float().amax(dim=1).double() + den.double())[band]
    half = 0.5 * (den.double().abs()[band] + 32.0) * (V // 256 + 2) * 2.0 ** -22
    worst = float(eps.max())
    ratio = float((eps * 1.4426950408889634 / half).max())
    print(f"{what}: max_v z + den over {int(band.sum())} in-band rows: {worst:.3e}; eps log2(e) over half the rule's "
          f"slack: {ratio:.3f}")
    assert bool(torch.isfinite(eps).all()) and ratio <= 1.0, (what, worst, ratio)
    if flat:
        assert worst <= 1e-6, (what, worst)


SOFTMAX_VARIANTS = [13, 21, 22, 23, 16, 14, 15, 0, 2]
# rows of one full chunk (1024: 4 loads per lane, 256: 16-lane rows / one load, 64), the scalar form (1001), partial
# chunks (800: 4 loads, 400: 2 loads), a full chunk of 2 loads (512), three chunks with a partial last one (2052)
DEN_V = (1024, 256, 64, 1001, 800, 512, 400, 2052)


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("softmax_variant", SOFTMAX_VARIANTS)
def test_den_bound_softmax_variants(op, L, dev, softmax_variant, name):
    """Every softmax_variant x element type x row form at the offset 1e4: eps <= 1e-6 on the single-chunk rows, the
    rule's slack on all of them."""
    lengths = ((14, 9, 11), (5, 9, 0))
    for V in DEN_V:
        a, lab, T, S = _den_inputs(dev, V, DTYPES[name], lengths, seed=V)
        with knobs(softmax_variant=softmax_variant, chase=0):
            _assert_den_bound(op, L, a, lab, T, S, f"softmax_variant {softmax_variant} {name} V={V}",
                              flat=V * a.element_size() <= 4096)


@pytest.mark.parametrize("offset", [1.2e4, 5.0e4, 2.0e5, -2.0e5])
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("softmax_variant", SOFTMAX_VARIANTS)
def test_den_bound_across_a_binade(op, L, dev, softmax_variant, name, offset):
    """Offsets whose max * kLog2e lies in the binade above max (1.2e4 -> 17,312 >= 16,384; 5e4 -> 72,135 >= 65,536;
    2e5 -> 288,539 >= 262,144; 1.5e5 -> 216,404 would not: eps = 0 there, like 1e4): the maximum's own term of the fmaf forms is 2^d with d up to an ulp of max, a dominant row's -den rounds to max - ulp(max), and
    eps is 1e-3 .. 1.6e-2, not 1e-6. The rule's slack covers it on every form. (fp16 holds nothing above 65,504: its
    offsets stop at 3e4, whose max * kLog2e = 43,281 is in the binade above as well.)"""
    if name == "fp16":  # (a row may carry the offset twice: 2 x 3e4 still fits)
        offset = float(np.clip(offset, -3.0e4, 3.0e4))
    lengths = ((14, 9, 11), (5, 9, 0))
    for V in DEN_V:
        a, lab, T, S = _den_inputs(dev, V, DTYPES[name], lengths, seed=V + 7, offset=offset)
        with knobs(softmax_variant=softmax_variant, chase=0):
            _assert_den_bound(op, L, a, lab, T, S, f"softmax_variant {softmax_variant} {name} V={V} offset {offset:g}",
                              flat=False)


@pytest.mark.parametrize("offset", [1.0e4, 1.2e4, 2.0e5])
@pytest.mark.parametrize("self_help", [0, 1])
@pytest.mark.parametrize("V,B,T,S", [(256, 8, 200, 40), (400, 4, 300, 60), (512, 4, 300, 60), (800, 4, 300, 60),
                                     (1024, 4, 300, 60)])
def test_den_bound_chase(op, L, dev, V, B, T, S, self_help, offset):
    """The chase launch at shapes where it pays, one per body (f32: 16-lane rows; 2 loads per lane, partial and full; 4
    loads, partial and full): its producers, and with a wait budget of 0 the recursion waves' own column body (the
    columns were helped)."""
    a, lab, Tn, Sn = _den_inputs(dev, V, torch.float32, ([T] * B, [S] * B), seed=V + 1, offset=offset)
    kn = dict(chase=1, chase_pair=1)
    if self_help:
        kn.update(chase_wait_us=0, chase_delay_us=200)
    with knobs(**kn):
        L.profile_enable(True)
        try:
            L.load_dev().mrnnt_chase_helped(1)
            _assert_den_bound(op, L, a, lab, Tn, Sn, f"chase V={V} self_help={self_help} offset {offset:g}",
                              flat=offset == 1.0e4)
            helped = int(L.load_dev().mrnnt_chase_helped(1))
            prof = {k: n for k, (_, n) in L.profile_read().items()}
        finally:
            L.profile_enable(False)
    assert prof["chase"] == 1, prof
    assert not self_help or helped > 0


@pytest.mark.parametrize("grad_variant", [5, 0, 3])
def test_bit_identity_at_large_offsets(op, L, dev, grad_variant):
    """Rows shifted by 0, 1.2e4, 1.5e5, 2e5 and -2e5 in turn (the softmax does not change, eps does: up to 1.6e-2 nats at
    2e5, more than 2^-6 in the exponent): gradients and costs bit-identical across occ_skip 0 / 2 / 1, the rule still
    decides rows."""
    offs = np.array([0.0, 1.2e4, 1.5e5, 2.0e5, -2.0e5], np.float32)

    def edit(d, acts):
        acts += offs[np.arange(acts.shape[0]) % offs.size][:, None]

    key = ("offsets", "f32")
    if key not in _CACHE:
        _CACHE[key] = Data(dev, None, torch.float32, seed=21, utts=[(120, 30, 3.0)] * 4 + [(9, 0, 3.0)], V=1024, edit=edit)
    d = _CACHE[key]
    assert sum(d.win) >= 100, d.win
    vec = torch.tensor(SCALE, dtype=torch.float32, device=dev)
    out, live = {}, {}
    with knobs(grad_variant=grad_variant):
        for skip in (0, 2, 1):
            with knobs(occ_skip=skip):
                prep = d.prepared(op)
                costs, ws = op._forward(prep, with_beta=True)
                out[skip] = (costs.view(torch.int32).clone(), backward(L, prep, ws, vec).view(torch.int32))
                live[skip] = live_rows(L, prep, ws)
    print(f"offsets: window {d.win}, live rows {live}")
    for skip in (2, 1):
        assert torch.equal(out[0][0], out[skip][0]) and torch.equal(out[0][1], out[skip][1]), skip
    assert live[2] - live[1] >= 50, live


# ---------------------------------------------------------------------------------------------------------------------

def test_non_finite(op, L, dev):
    """A NaN logit in a window row (the utterance's ll is NaN), ll = -inf (every blank logit -inf with T > S: no path)
    and a NaN grad_output over a clean utterance with window rows: every row takes the full path, and the result is
    bit-identical across occ_skip 0 / 2 / 1."""
    utts = [(120, 30, 3.0)] * 4
    clean = Data(dev, None, torch.float32, seed=11, utts=utts, V=1024)
    assert min(clean.win) >= 50, clean.win
    occ = log_occupancy(clean.al, clean.be, clean.cr, clean.T, clean.S)
    hit = int(np.flatnonzero((occ >= -105.0) & (occ < -90.0))[0])  # a window row of utterance 0
    assert clean.utt[hit] == 0

    def edit(d, acts):
        acts[hit, 17] = np.nan
        acts[d.utt == 1, 0] = -np.inf

    d = Data(dev, None, torch.float32, seed=11, utts=utts, V=1024, edit=edit)
    assert np.isnan(d.cr[0]) and d.cr[1] == np.inf and np.isfinite(d.cr[2:]).all(), d.cr
    scale = torch.tensor([1.0, -0.5, float("nan"), 2.0], dtype=torch.float32, device=dev)
    out = {}
    for skip in (0, 2, 1):
        with knobs(occ_skip=skip):
            prep = d.prepared(op)
            costs, ws = op._forward(prep, with_beta=True)
            out[skip] = (costs.view(torch.int32).clone(), backward(L, prep, ws, scale).view(torch.int32))
    for skip in (2, 1):
        assert torch.equal(out[0][0], out[skip][0]) and torch.equal(out[0][1], out[skip][1]), skip
    g = out[1][1].view(torch.float32).cpu().numpy()
    for b in (0, 1, 2):
        assert np.isnan(g[d.utt == b]).all(), b
    assert_grads(g[d.utt == 3], 2.0 * clean.gr[clean.utt == 3])


@pytest.mark.parametrize("grad_variant", [5, 0])
def test_infeasible_alignment_band(op, L, dev, grad_variant):
    """ll = -inf through the alignment band: utterance 0's alignment holds no label, so with max_shift 2 no path
    reaches s = S and its every row is NaN; utterances 1 and 2 follow real alignments. The forward reduces only the
    rows of each column's window, so the rows outside it keep whatever den the workspace held -- here the state of a
    forward over other logits, on purpose -- and are dead before the flush rule looks at them. Bit-identical across
    occ_skip 0 / 2 / 1, and equal to the oracle."""
    rng = np.random.default_rng(31)
    T, S, V, k = np.array([120, 120, 90], np.int32), np.array([30, 30, 20], np.int32), 1024, 2
    n = T * (S + 1)
    utt = np.repeat(np.arange(3), n)
    acts = (3.0 * rng.standard_normal((int(n.sum()), V))).astype(np.float32)
    labels = rng.integers(1, V, (3, 30)).astype(np.int32)
    al = np.zeros((3, 120), np.int32)
    for b in (1, 2):
        al[b, np.sort(rng.choice(T[b], S[b], replace=False))] = labels[b, :S[b]]
    cr, gr = O.oracle_rnnt(acts, labels, T, S, alignment=al, max_shift=k, num_threads=8)
    assert cr[0] == np.inf and np.isfinite(cr[1:]).all(), cr
    scale = np.array([1.0, -0.5, 2.0], np.float32)
    a, stale = torch.from_numpy(acts).to(dev), torch.from_numpy(acts[::-1].copy() * 40.0).to(dev)
    lab, ald, vec = torch.from_numpy(labels).to(dev), torch.from_numpy(al).to(dev), torch.from_numpy(scale).to(dev)
    out = {}
    with knobs(grad_variant=grad_variant):
        for skip in (0, 2, 1):
            with knobs(occ_skip=skip):
                # the workspace first takes an unrestricted forward over other logits: every den is written, and stale
                free = op._Prepared(stale, lab, torch.from_numpy(T), torch.from_numpy(S), None, 0, 0)
                prep = op._Prepared(a, lab, torch.from_numpy(T), torch.from_numpy(S), ald, k, 0)
                ws, wf = prep.workspace(), free.workspace()
                big = ws if ws.numel() >= wf.numel() else wf
                costs = torch.empty(3, dtype=torch.float32, device=dev)
                op._call(free, "forward", vp(big), big.numel(), vp(costs), 1)
                op._call(prep, "forward", vp(big), big.numel(), vp(costs), 1)
                out[skip] = (costs.view(torch.int32).clone(), backward(L, prep, big, vec).view(torch.int32))
    for skip in (2, 1):
        assert torch.equal(out[0][0], out[skip][0]) and torch.equal(out[0][1], out[skip][1]), skip
    g = out[1][1].view(torch.float32).cpu().numpy()
    assert np.isnan(g[utt == 0]).all()
    assert_costs(out[1][0].view(torch.float32).cpu().numpy(), cr)
    fin = utt != 0
    assert_grads(g[fin], (gr * scale.astype(np.float64)[utt][:, None])[fin])


def test_row_state(op, L, dev):
    """Two tracked steps on one buffer (the product library). After the first, every row of the window [-110, -87.6)
    has state 1 or 2 like any other zero row; those rows are overwritten with a sentinel, the state kept, as a caller
    that wrote them would not be allowed to; the second step does not store them again, and everywhere else the
    buffer equals an untracked launch."""
    d = data(dev, "v1024", "f32")
    sent = 0x7FC0BEEF
    vec = torch.tensor(SCALE, dtype=torch.float32, device=dev)
    prep = d.prepared(op)
    _, ws = op._forward(prep, with_beta=True)
    plain = backward(L, prep, ws, vec).view(torch.int32)
    rows = plain.size(0)
    ibuf = torch.full((rows, d.V), sent, dtype=torch.int32, device=dev)
    state = torch.zeros(rows, dtype=torch.uint8, device=dev)
    backward(L, prep, ws, vec, state=state, grads=ibuf)
    assert torch.equal(ibuf, plain)
    occ = log_occupancy(d.al, d.be, d.cr, d.T, d.S)
    win = (occ >= -110.0) & (occ < -87.6)  # the window rows, in the packed row order
    st = state.cpu().numpy()
    assert int(win.sum()) == sum(d.win) and np.all(st[win] != 0) and np.all(st <= 2)
    want = np.where(np.signbit(np.asarray(SCALE, np.float32) * 0.0)[d.utt], 2, 1)
    assert np.array_equal(st[win], want[win]) and (st[win] == 2).any() and (st[win] == 1).any()
    zero = torch.from_numpy(st != 0).to(dev)
    ibuf[zero] = sent
    backward(L, prep, ws, vec, state=state, grads=ibuf)
    assert np.array_equal(state.cpu().numpy(), st)
    assert bool((ibuf[zero] == sent).all()), "a row the state vouched for was stored again"
    assert torch.equal(ibuf[~zero], plain[~zero])
    assert bool(((plain[zero] & 0x7FFFFFFF) == 0).all())  # what the skipped rows hold in the untracked launch: +0 or -0
