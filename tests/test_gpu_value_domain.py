"""The HIP path on logits outside N(0,1) -- the value-domain cases and bounds of _value_domain.py (large offsets, peaked
and constant rows, -inf masks, NaN / +inf poison) -- against the fp64 oracle on the exact upcast values the kernels
read, at the smallest shapes that reach each code path:

    16-lane rows (partial / full)            V = 100, 256    f32        B = 3, T in [6, 40], S <= 12
    single chunk (partial / full)            V = 1000, 1024  f32        same
    multi-chunk running max                  V = 2052        f32        B = 2, T <= 20, S <= 6
    odd V (scalar kernels)                   V = 257         f32        same
    reduced precision                        V = 512         bf16, f16  B = 3, T <= 40, S <= 12
    halo recursion                           V = 16          f32        B = 2, S = 100, T = 130
    per-step-barrier recursion               V = 16          f32        B = 1, S = 460, T = 480

Paths: the product library (`product`, and `devlen`: device-resident lengths), and the development build with the chase
launch on (`chase`: knobs(chase=1, chase_pair=1)) and off (`nochase`: knobs(chase=0)), the launch confirmed from the
profile counters (a shape the chase does not take skips its `chase` leg).

The rule the poison tests pin is the one of test_cpu_value_domain.py: NaN in, NaN out -- never +inf ("no path"),
never a finite cost -- and the other utterances of the batch untouched, bit for bit.
"""
import contextlib

import numpy as np
import pytest
import torch

import oracle as O
import _value_domain as D
from _parity import COST_TOL, GRAD_TOL, knobs
from test_gpu_chase import _launches
from test_gpu_fuzz import pad, unpad

pytestmark = pytest.mark.gpu

ROWS = {
    # name: (V, dtype, B, T range, S max, force)
    "row16_partial": (100, "f32", 3, (6, 40), 12, {0: (40, 12), 1: (9, 0), 2: (7, 7)}),
    "row16_full": (256, "f32", 3, (6, 40), 12, {0: (33, 11), 2: (12, 12)}),
    "one_partial": (1000, "f32", 3, (6, 40), 12, {0: (37, 12), 1: (6, 0)}),
    "one_full": (1024, "f32", 3, (6, 40), 12, {0: (40, 9), 2: (8, 8)}),
    "multi_chunk": (2052, "f32", 2, (6, 20), 6, {0: (20, 6)}),
    "odd_v": (257, "f32", 2, (6, 20), 6, {0: (19, 5)}),
    "bf16": (512, "bf16", 3, (6, 40), 12, {0: (40, 12), 1: (11, 0)}),
    "f16": (512, "f16", 3, (6, 40), 12, {0: (40, 12), 1: (11, 0)}),
    "halo": (16, "f32", 2, (130, 130), 100, {0: (130, 100), 1: (130, 100)}),
    "barrier": (16, "f32", 1, (480, 480), 460, {0: (480, 460)}),
}
F32_SMALL_V = [r for r, c in ROWS.items() if c[1] == "f32" and c[0] <= 1024]
LEGS = [(r, "product") for r in ROWS] + [(r, p) for r in F32_SMALL_V for p in ("chase", "nochase")] + \
       [(r, "devlen") for r in ("row16_partial", "row16_full", "one_partial", "one_full")]
# rows the chase launch takes (development build, chase = 1): their `chase` legs must run, not skip. The others'
# (the scalar log-softmax of odd V, the per-step-barrier recursion) skip.
CHASE_TAKES = ("row16_partial", "row16_full", "one_partial", "one_full", "halo")
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_BASE = {}


def base(row):
    if row not in _BASE:
        V, dtype, B, Tr, Smax, force = ROWS[row]
        _BASE[row] = D.base_problem(sum(map(ord, row)), B, Tr, Smax, V, force=force)
    return _BASE[row]


def upcast(acts, dtype):
    """The values the kernels read: acts rounded to the element type, as fp32."""
    return torch.from_numpy(acts).to(TORCH_DT[dtype]).float().numpy()


def run(op, dev, host, labels, T, S, dtype="f32", dev_lengths=False, padded=False, alignment=None, k=0):
    """costs [B] f64 and gradients [rows, V] f32 (as fp32 of the element type) of the op on the upcast values."""
    a = torch.from_numpy(pad(host, T, S, int(T.max()) + 2, int(S.max()) + 3) if padded else host).to(TORCH_DT[dtype])
    a = a.to(dev).requires_grad_(True)
    Tt, St = torch.from_numpy(T), torch.from_numpy(S)
    if dev_lengths:
        Tt, St = Tt.to(dev), St.to(dev)
    al = None if alignment is None else torch.from_numpy(alignment).to(dev)
    costs = op.monotonic_rnnt_loss(a, torch.from_numpy(labels).to(dev), Tt, St, al, k)
    costs.sum().backward()
    torch.cuda.synchronize()
    g = a.grad.float().cpu().numpy()
    if padded:
        pad_rows = np.ones(g.shape[:3], bool)
        for b in range(len(T)):
            pad_rows[b, : T[b], : S[b] + 1] = False
        assert np.all(g[pad_rows] == 0.0), "padding rows of the gradient are zero"
        g = unpad(g, T, S)
    return costs.detach().float().cpu().numpy().astype(np.float64), g


@contextlib.contextmanager
def leg(op, dev, row, path):
    """The library and knobs of a path; yields the run keyword arguments. The chase legs check, on the row's base
    problem, that the chase launch did (did not) run."""
    dtype = ROWS[row][1]
    kw = dict(dtype=dtype, dev_lengths=(path == "devlen"))
    if path in ("product", "devlen"):
        yield kw
        return
    acts, labels, T, S = base(row)
    with knobs(chase=1, chase_pair=1) if path == "chase" else knobs(chase=0):
        n = _launches(lambda: run(op, dev, acts, labels, T, S, **kw))
        if path == "chase":
            if n["chase"] == 0:
                # the chase-path coverage of these tests rests on the rows below: they may not skip
                assert row not in CHASE_TAKES, f"the chase launch no longer takes {row}: {n}"
                pytest.skip(f"the chase launch does not take {row}")
            assert n["log_softmax"] == 0 and n["alpha_beta"] == 0, n
        else:
            assert n["chase"] == 0 and n["log_softmax"] >= 1, n
        yield kw


def check_vs_oracle(name, got, host, labels, T, S, dtype):
    """None, or what missed: costs classed and within cost_tol, gradients non-finite in the oracle's places and within
    grad_tol. Prints the figures first."""
    c, g = got
    cr, gr = O.oracle_rnnt(host, labels, T, S, num_threads=8)
    tol_c, (tol_g, rel_g) = D.cost_tol(cr, T, host), D.grad_tol(host, dtype)
    fin = np.isfinite(gr)
    cerr = np.abs(c - D.as_f32_costs(cr))
    gerr = float(np.abs(g[fin] - gr[fin]).max()) if fin.any() and np.array_equal(np.isfinite(g), fin) else float("nan")
    print(f"{name}: cost err / tol {np.nanmax(cerr / tol_c):.3f} (err {np.nanmax(cerr):.3e}), "
          f"grad err {gerr:.3e} (tol {tol_g:.3e} + {rel_g:.1e} |g|)")
    try:
        D.assert_costs_classed(c, cr, tol_c)
        D.assert_grads_tol(g, gr, tol_g, rel_g)
    except AssertionError as e:
        return f"{name}: {str(e)[:300]}"
    return None


# (fp16: 1e4 + N(0,1) and 1000 N(0,1) stay below 65504)
FINITE = [D.offset(100.0), D.offset(-100.0), D.offset(1e3), D.offset(1e4), D.offset(-1e4), D.row_offsets(1e3),
          D.scale(30.0), D.scale(1000.0), D.constant(0.0), D.constant(-1e4), D.mask_unused(0.5)]


@pytest.mark.parametrize("row,path", LEGS, ids=[f"{r}-{p}" for r, p in LEGS])
def test_finite_transforms_vs_oracle(op, dev, row, path):
    """offset(+-100, 1e3, +-1e4), row_offsets(1e3), scale(30, 1000), constant(0, -1e4), mask_unused against the oracle
    at the bounds of _value_domain (the plain 1e-4 up to |z| = 128). At offset 1e4 the bf16 values collapse into exact
    ties: intended."""
    acts, labels, T, S = base(row)
    dtype = ROWS[row][1]
    bad = []
    with leg(op, dev, row, path) as kw:
        for tf in FINITE:
            host = upcast(tf(acts, labels, T, S), dtype)
            assert np.all(np.isfinite(host) | np.isneginf(host)), tf.__name__
            bad.append(check_vs_oracle(tf.__name__, run(op, dev, host, labels, T, S, **kw), host, labels, T, S, dtype))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("row", list(ROWS))
def test_peaked_rows_occupancy_skip_bit_identical(op, dev, row):
    """scale(1000) leaves most rows dead (occupancy < e^-110): with the skip off (development build, occ_skip = 0) the
    costs and gradients are the same bits as with it on."""
    acts, labels, T, S = base(row)
    dtype = ROWS[row][1]
    host = upcast(D.scale(1000.0)(acts, labels, T, S), dtype)
    out = {}
    for skip in (1, 0):
        with knobs(occ_skip=skip):
            out[skip] = run(op, dev, host, labels, T, S, dtype=dtype)
    assert D.same_bits(out[0][0], out[1][0]) and D.same_bits(out[0][1], out[1][1])
    assert check_vs_oracle("scale(1000), occ_skip=0", out[0], host, labels, T, S, dtype) is None


@pytest.mark.parametrize("row", ["row16_partial", "one_partial", "multi_chunk", "odd_v", "halo"])
@pytest.mark.parametrize("M", [64.0, -64.0])
def test_shift_invariance_exact_inputs(op, dev, row, M):
    """Logits quantised to multiples of 2^-10 with |z| <= 8 shift by +-64 exactly in fp32, and log-softmax is shift
    invariant: the shifted costs equal the unshifted ones within COST_TOL and the gradients within GRAD_TOL -- no
    oracle, no widened bound."""
    acts, labels, T, S = base(row)
    q = np.clip(np.round(acts * 1024.0) / 1024.0, -8.0, 8.0).astype(np.float32)
    sh = D.offset(M)(q, labels, T, S)
    assert np.array_equal(sh.astype(np.float64), q.astype(np.float64) + M)
    c0, g0 = run(op, dev, q, labels, T, S)
    c1, g1 = run(op, dev, sh, labels, T, S)
    print(f"shift {M:g}: cost diff {np.abs(c1 - c0).max():.3e}, grad diff {np.abs(g1 - g0).max():.3e}")
    assert np.all(np.isfinite(c0)) and np.all(np.abs(c1 - c0) <= COST_TOL * np.maximum(1.0, np.abs(c0))), (c0, c1)
    assert np.all(np.isfinite(g1)) and float(np.abs(g1 - g0).max()) <= GRAD_TOL


def test_padded_layout_masked_logits_nan_padding(op, dev):
    """The padded [B, pad_T, pad_S1, V] layout with -inf masked columns in the lattice rows and NaN in every padding
    row: the padding does not leak (costs and gradients on the oracle, padding gradients exactly 0)."""
    row = "row16_partial"
    acts, labels, T, S = base(row)
    host = D.mask_unused(0.5)(acts, labels, T, S)
    got = run(op, dev, host, labels, T, S, padded=True)
    assert check_vs_oracle("mask_unused, padded", got, host, labels, T, S, "f32") is None
    packed = run(op, dev, host, labels, T, S)
    assert D.same_bits(got[0], packed[0]) and D.same_bits(got[1], packed[1])


def others_untouched(b, T, S, got, ref):
    (c, g), (c0, g0) = got, ref
    for o in range(len(T)):
        if o != b:
            assert D.same_bits(c[o:o + 1], c0[o:o + 1]), (o, c, c0)
            assert D.same_bits(g[D.utt_rows(T, S, o)], g0[D.utt_rows(T, S, o)]), o


MASK_LEGS = [(r, p) for r in ("row16_partial", "row16_full", "one_partial", "one_full", "halo")
             for p in ("product", "chase", "nochase")]


@pytest.mark.parametrize("row,path", MASK_LEGS, ids=[f"{r}-{p}" for r, p in MASK_LEGS])
def test_masked_label_and_blank_are_inf_others_untouched(op, dev, row, path):
    """-inf on utterance 0's first label column / on its blank column, in its rows: its cost is +inf (no path), its
    gradient non-finite where the oracle's is, and every other utterance the same bits as on the clean logits."""
    acts, labels, T, S = base(row)
    with leg(op, dev, row, path) as kw:
        x, lab = D.mask_label(0)(acts, labels, T, S)
        for name, x, lab in (("mask_label", x, lab), ("mask_blank_rows", D.mask_blank_rows(0)(acts, labels, T, S), labels)):
            got = run(op, dev, x, lab, T, S, **kw)
            cr, gr = O.oracle_rnnt(x, lab, T, S, num_threads=8)
            assert D.cost_class(cr)[0] == "+inf" and D.cost_class(got[0])[0] == "+inf", (name, got[0], cr)
            D.assert_costs_classed(got[0], cr)
            D.assert_grads_tol(got[1], gr, GRAD_TOL)
            others_untouched(0, T, S, got, run(op, dev, acts, lab, T, S, **kw))


# rows of the multi-wave recursions beyond band_positions' picks: a wave other than wave 0, and the wave boundaries
# (the per-step-barrier kernel: 64 cells per wave; the halo recursion: 56 own cells per wave)
EXTRA_POSITIONS = {
    "halo": [(60, 55), (60, 56), (70, 63), (70, 64), (100, 90)],
    "barrier": [(60, 55), (60, 56), (70, 63), (70, 64), (310, 300), (479, 459)],
}
POISON_LEGS = [(r, p) for r in ("row16_partial", "row16_full", "one_partial", "one_full", "halo", "barrier")
               for p in ("product", "chase", "nochase")]


@pytest.mark.parametrize("row,path", POISON_LEGS, ids=[f"{r}-{p}" for r, p in POISON_LEGS])
def test_poison_is_nan_and_others_untouched(op, dev, row, path):
    """One NaN or +inf logit at every first / last row, up to 3 rows of each other kind and the wave-boundary rows of
    utterance 0, a whole row of -inf at an interior row, and (B > 1) one NaN at the first and the last row of utterance
    1 -- the rows that follow utterance 0's in the workspace, where a recursion lane past S_0 would read them. The
    oracle calls the poisoned utterance NaN (asserted first: the condition the inputs are chosen for); the library
    must too, with no finite garbage in its gradient, and every other utterance the same bits as on the clean
    logits."""
    acts, labels, T, S = base(row)
    pos = [p[:2] for p in D.pick_positions(T[0], S[0])] + EXTRA_POSITIONS.get(row, [])
    inband = {p[:2] for p in D.band_positions(T[0], S[0])}
    assert all(p in inband for p in pos)
    tfs = [(0, D.poison(0, t, s, v)) for t, s in pos for v in (D.NAN, D.INF)]
    inner = next(p for p in D.pick_positions(T[0], S[0]) if p[2] == "interior")
    tfs.append((0, D.all_neg_inf_row(0, inner[0], inner[1])))
    if len(T) > 1:
        tfs += [(1, D.poison(1, 0, 0, D.NAN)), (1, D.poison(1, T[1] - 1, S[1], D.NAN))]
    bad = []
    with leg(op, dev, row, path) as kw:
        ref = run(op, dev, acts, labels, T, S, **kw)
        assert np.all(np.isfinite(ref[0]))
        for b, tf in tfs:
            x = tf(acts, labels, T, S)
            cr, gr = O.oracle_rnnt(x, labels, T, S, num_threads=8)
            assert D.cost_class(cr)[b] == "nan", (tf.__name__, cr)
            c, g = run(op, dev, x, labels, T, S, **kw)
            if D.cost_class(c)[b] != "nan":
                bad.append(f"{tf.__name__}: cost {c[b]} (class {D.cost_class(c)[b]}), oracle nan")
                continue
            try:
                others_untouched(b, T, S, (c, g), ref)
                rows = D.utt_rows(T, S, b)
                D.assert_poisoned_grads(g[rows], gr[rows], D.grad_tol(x)[0])
            except AssertionError as e:
                bad.append(f"{tf.__name__}: {str(e)[:200]}")
    assert not bad, f"{len(bad)} of {len(tfs)} cases:\n" + "\n".join(bad)


CROSS = {
    # name: (force, alignment shift k or None): a short utterance in front of the one whose recursion shape is meant
    "barrier": ({0: (12, 4), 1: (480, 460)}, None),        # per-step-barrier recursion (S + 1 > 448)
    "halo": ({0: (12, 4), 1: (130, 100)}, None),           # lean halo recursion
    "halo_aligned": ({0: (12, 4), 1: (130, 100)}, 2),      # alignment-restricted: the masked halo step
    "one_wave": ({0: (40, 12), 1: (9, 0)}, None),          # one wave, 50 lanes past S_0
    "one_wave_aligned": ({0: (40, 12), 1: (9, 3)}, 1),
}


@pytest.mark.parametrize("path", ["product", "nochase"])
@pytest.mark.parametrize("name", list(CROSS))
def test_poison_does_not_cross_utterances(op, dev, name, path):
    """The lp rows of the utterances of a batch lie back to back in the workspace, and recursion lanes at the ends of
    a frame (the cell below s = 0, the lanes past S) read the neighbouring rows for terms that are -inf whatever they
    hold -- unless they hold a NaN. A NaN in the last row of utterance 0 / the first row of utterance 1 makes that
    utterance NaN (the oracle's answer, asserted first) and leaves the other one the same bits as on clean logits."""
    force, k = CROSS[name]
    acts, labels, T, S = D.base_problem(sum(map(ord, name)), 2, (6, 6), 4, 16, force=force)
    al = None
    if k is not None:
        rng = np.random.default_rng(k)
        al = np.zeros((2, int(T.max())), np.int32)
        for b in range(2):
            al[b, np.sort(rng.choice(T[b], S[b], replace=False))] = labels[b, : S[b]]
    kw = dict(alignment=al, k=k or 0)
    with knobs(chase=0) if path == "nochase" else contextlib.nullcontext():
        ref = run(op, dev, acts, labels, T, S, **kw)
        assert np.all(np.isfinite(ref[0]))
        for b, tf in ((0, D.poison(0, T[0] - 1, S[0], D.NAN)), (1, D.poison(1, 0, 0, D.NAN))):
            x = tf(acts, labels, T, S)
            cr, _ = O.oracle_rnnt(x, labels, T, S, alignment=al, max_shift=k or 0, grads=False, num_threads=8)
            assert D.cost_class(cr)[b] == "nan" and D.cost_class(cr)[1 - b] == "finite", (tf.__name__, cr)
            c, g = run(op, dev, x, labels, T, S, **kw)
            assert D.cost_class(c)[b] == "nan", (tf.__name__, c)
            others_untouched(b, T, S, (c, g), ref)
            assert np.isnan(g[D.utt_rows(T, S, b)]).all(), tf.__name__
