"""Checks of monotonic_rnnt_expected_cost shared by tests/test_cpu_expect.py and tests/test_gpu_expect.py (only the
device differs).

`run(acts, labels, T, S, wb, we, ge=None, gc=None, alignment=None, k=0, **kw)` -> (expected fp32 [B], costs fp32 [B],
grads fp32 in the shape of acts) as numpy arrays: expected_cost with the per-row cost arrays wb / we (None: absent),
then ONE backward of sum_b ge[b] expected[b] + gc[b] costs[b] (None: ones).

Yardsticks (independent of the library): torch on the CPU in float64 over lsm = log_softmax(acts.double()), gradients
torch.autograd's of the same objective.
  (a) brute: every one of the C(T, S) paths of an utterance enumerated, T <= 7;
  (b) dp: a log-domain recursion over frames, vectorised over s, carrying ll and the mean prefix cost.
For bf16 / fp16 the yardstick runs on the upcast values the kernel reads, plus one rounding of the output type.

Tolerances. W_b = sum_t max_s max(|wb|, |we|) bounds |f(path)| of utterance b.
  expected: COST_TOL + 4e-6 W_b (absolute).            costs: assert_costs.
  gradient, per utterance: GRAD_TOL |g_c| (the loss's, scaled by its upstream) + |g_e| (GRAD_TOL + 4e-6 W_b).
The 4e-6 W_b: a coefficient is a posterior with relative error ~1e-6 (the fp32 exp of the gradient's row coefficients)
times a deviation of at most 2 W_b; twice that bound. fp32 storage adds 6e-8 relative.
"""
import itertools
import math

import numpy as np
import torch

import _align_checks as A
from _align_checks import BLANK, offsets, ragged  # noqa: F401  (re-exported)
from _parity import COST_TOL, GRAD_TOL, assert_costs
from _path_checks import pack_to_padded, padded_to_packed

NI = -math.inf


# ---- problems ---------------------------------------------------------------------------------------------------------

def frame_of_row(T, S):
    """t of every packed lattice row."""
    return np.concatenate([np.repeat(np.arange(Tb), Sb + 1) for Tb, Sb in zip(T, S)]).astype(np.float32)


def utt_of_row(T, S):
    return np.concatenate([np.full(int(Tb) * (int(Sb) + 1), b) for b, (Tb, Sb) in enumerate(zip(T, S))])


def random_costs(rng, T, S):
    """N(0, 1) on both arcs, plus the emission time on the label arc."""
    n = int(offsets(T, S)[-1])
    wb = rng.standard_normal(n).astype(np.float32)
    we = (rng.standard_normal(n) + frame_of_row(T, S)).astype(np.float32)
    return wb, we


def latency_costs(T, S):
    return None, frame_of_row(T, S)


def cost_bound(wb, we, T, S):
    """W_b [B]."""
    off = offsets(T, S)
    out = np.zeros(len(T))
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        m = np.zeros((Tb, Sb + 1))
        for x in (wb, we):
            if x is not None:
                m = np.maximum(m, np.abs(np.asarray(x[off[b]:off[b + 1]], np.float64)).reshape(Tb, Sb + 1))
        out[b] = m.max(axis=1).sum()
    return out


def upstreams(rng, B):
    """Signed per-utterance upstream gradients of expected and costs."""
    return rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)


# ---- yardsticks -------------------------------------------------------------------------------------------------------

def _brute_utt(z, lab, Tb, Sb, wb, we):
    logps, fs = [], []
    for emit in itertools.combinations(range(Tb), Sb):
        s, lp, f = 0, 0.0, 0.0
        for t in range(Tb):
            if t in emit:
                lp = lp + z[t, s, int(lab[s])]
                f += float(we[t, s])
                s += 1
            else:
                lp = lp + z[t, s, BLANK]
                f += float(wb[t, s])
        logps.append(lp)
        fs.append(f)
    logps = torch.stack(logps)
    ll = torch.logsumexp(logps, 0)
    return ll, (torch.exp(logps - ll) * torch.tensor(fs, dtype=torch.float64)).sum()


def _dp_utt(z, lab, Tb, Sb, wb, we):
    W = Sb + 1
    lpb = z[:, :, BLANK]
    lpe = torch.cat([z[:, torch.arange(Sb), torch.as_tensor(np.asarray(lab[:Sb], np.int64))],
                     torch.zeros(Tb, 1, dtype=torch.float64)], 1) if Sb else torch.zeros(Tb, 1, dtype=torch.float64)
    wb, we = torch.from_numpy(wb), torch.from_numpy(we)
    al = torch.full((W,), NI, dtype=torch.float64)
    al[0] = 0.0
    Am = torch.zeros(W, dtype=torch.float64)
    s = torch.arange(W)
    ninf, zero1 = torch.full((1,), NI, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    for t in range(Tb):
        x = al + lpb[t]
        y = torch.cat([ninf, (al + lpe[t])[:-1]])
        xa = Am + wb[t]
        ya = torch.cat([zero1, (Am + we[t])[:-1]])
        ok = (s <= t + 1) & (Sb - s <= Tb - 1 - t)
        x = torch.where(ok, x, torch.full_like(x, NI))
        y = torch.where(ok, y, torch.full_like(y, NI))
        m = torch.maximum(x, y)
        live = m > NI
        ms = torch.where(live, m, torch.zeros_like(m))
        ex, ey = torch.exp(x - ms), torch.exp(y - ms)
        den = torch.where(live, ex + ey, torch.ones_like(ex))
        al = torch.where(live, ms + torch.log(den), torch.full_like(m, NI))
        Am = torch.where(live, (ex * xa + ey * ya) / den, torch.zeros_like(Am))
    return al[Sb], Am[Sb]


def yardstick(acts, labels, T, S, wb, we, ge=None, gc=None, brute=False):
    """expected fp64 [B], costs fp64 [B], grads fp64 [N, V] of sum_b ge[b] expected[b] + gc[b] costs[b]."""
    B = len(T)
    ge = np.ones(B) if ge is None else np.asarray(ge, np.float64)
    gc = np.ones(B) if gc is None else np.asarray(gc, np.float64)
    n = int(offsets(T, S)[-1])
    wb = np.zeros(n) if wb is None else np.asarray(wb, np.float64)
    we = np.zeros(n) if we is None else np.asarray(we, np.float64)
    a = torch.tensor(np.asarray(acts, np.float64), requires_grad=True)
    lsm = torch.log_softmax(a, dim=1)
    off = offsets(T, S)
    exp_, cst, total = np.zeros(B), np.zeros(B), 0.0
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        sl = slice(int(off[b]), int(off[b + 1]))
        z = lsm[sl].view(Tb, Sb + 1, -1)
        fn = _brute_utt if brute else _dp_utt
        ll, R = fn(z, labels[b], Tb, Sb, wb[sl].reshape(Tb, Sb + 1), we[sl].reshape(Tb, Sb + 1))
        exp_[b], cst[b] = float(R.detach()), float(-ll.detach())
        total = total + float(ge[b]) * R - float(gc[b]) * ll
    total.backward()
    return exp_, cst, a.grad.numpy()


# ---- comparisons ------------------------------------------------------------------------------------------------------

def assert_expected(e, ref, Wb):
    e = np.asarray(e, np.float64)
    assert e.shape == ref.shape and np.all(np.isfinite(e)), e
    err, tol = np.abs(e - ref), COST_TOL + 4e-6 * Wb
    print("expected: max err / tol =", float((err / tol).max()))
    assert np.all(err <= tol), (err, tol)


def grad_tol(T, S, Wb, ge, gc):
    """Per row: GRAD_TOL |g_c| + |g_e| (GRAD_TOL + 4e-6 W_b) of the row's utterance."""
    B = len(T)
    ge = np.ones(B) if ge is None else np.abs(np.asarray(ge, np.float64))
    gc = np.ones(B) if gc is None else np.abs(np.asarray(gc, np.float64))
    return (GRAD_TOL * gc + ge * (GRAD_TOL + 4e-6 * Wb))[utt_of_row(T, S)][:, None]


def assert_grads(g, ref, tol, eps=0.0):
    g = np.asarray(g, np.float64)
    assert g.shape == ref.shape and np.all(np.isfinite(g))
    err = np.abs(g - ref) - eps * np.abs(ref)
    print("grads: max err / tol =", float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())


def check_against_yardstick(run, acts, labels, T, S, wb, we, ge, gc, brute=False, eps=0.0, yard_acts=None, **kw):
    e, c, g = run(acts, labels, T, S, wb, we, ge, gc, **kw)
    assert e.dtype == np.float32 and c.dtype == np.float32 and e.shape == (len(T),) and c.shape == (len(T),)
    ref_e, ref_c, ref_g = yardstick(acts if yard_acts is None else yard_acts, labels, T, S, wb, we, ge, gc, brute)
    Wb = cost_bound(wb, we, T, S)
    assert_expected(e, ref_e, Wb)
    assert_costs(c, ref_c)
    assert_grads(g, ref_g, grad_tol(T, S, Wb, ge, gc), eps)
    return e, c, g


# ---- 1. brute force ---------------------------------------------------------------------------------------------------

BRUTE_SHAPES = [(1, 0), (1, 1), (4, 0), (3, 3), (5, 2), (7, 3)]


def brute_problem(V):
    rng = np.random.default_rng(40 + V)
    acts, labels, T, S = ragged(rng, BRUTE_SHAPES, V)
    wb, we = random_costs(rng, T, S)
    ge, gc = upstreams(rng, len(T))
    return acts, labels, T, S, wb, we, ge, gc


def check_brute(run, V, **kw):
    """Ragged batch of tiny lattices against path enumeration; single-path utterances (S = 0, S = T) have an
    expected-gradient within tolerance of 0."""
    acts, labels, T, S, wb, we, ge, gc = brute_problem(V)
    check_against_yardstick(run, acts, labels, T, S, wb, we, ge, gc, brute=True, **kw)
    one = np.ones(len(T), np.float32)
    _, _, g = run(acts, labels, T, S, wb, we, one, 0 * one, **kw)
    tol = grad_tol(T, S, cost_bound(wb, we, T, S), one, 0 * one)
    single = np.isin(utt_of_row(T, S), [b for b, (t, s) in enumerate(BRUTE_SHAPES) if s == 0 or s == t])
    assert single.any() and np.all(np.abs(g[single]) <= tol[single])


# ---- 2. DP yardstick edges --------------------------------------------------------------------------------------------

# (name, V, [(T, S)]). T in {63, 64, 65, 130}, S + 1 in {56, 57, 64, 65, 113}: the wave boundaries of the recursion (and
# the 56-cell halo boundaries of the forward's); (305, 299) crosses the gradient's 256-row segment; S + 1 = 531 / 1031:
# two / three cells per lane of the recursion; V = 1024 with T <= 40; V = 32; V = 5: the scalar kernels.
EDGE_CASES = [
    ("waves_v8", 8, [(63, 55), (64, 56), (65, 63), (130, 64), (130, 112)]),
    ("segment_v8", 8, [(305, 299), (5, 2)]),
    ("cells2_v8", 8, [(560, 530), (9, 9)]),
    ("cells3_v8", 8, [(1040, 1030)]),
    ("v1024", 1024, [(40, 12), (20, 3), (1, 0), (12, 12)]),
    ("v32", 32, [(130, 40), (17, 0), (9, 9), (64, 1)]),
    ("scalar_v5", 5, [(65, 1), (33, 5), (1, 1), (64, 64)]),
]


def edge_problem(name):
    i = [c[0] for c in EDGE_CASES].index(name)
    _, V, shapes = EDGE_CASES[i]
    rng = np.random.default_rng(200 + i)
    acts, labels, T, S = ragged(rng, shapes, V)
    wb, we = random_costs(rng, T, S)
    ge, gc = upstreams(rng, len(T))
    return acts, labels, T, S, wb, we, ge, gc


def check_edge_case(run, name, **kw):
    return check_against_yardstick(run, *edge_problem(name), **kw)


def small_problem(seed=51, V=12, shapes=((23, 9), (17, 17), (12, 0), (30, 4))):
    rng = np.random.default_rng(seed)
    acts, labels, T, S = ragged(rng, list(shapes), V)
    wb, we = random_costs(rng, T, S)
    return acts, labels, T, S, wb, we


# ---- 3. identities ----------------------------------------------------------------------------------------------------

def check_posteriors_identity(run, run_posteriors, alignment=None, k=0):
    """expected = sum_rows blank_post wb + label_post we, the posteriors those of the same inputs."""
    acts, labels, T, S, wb, we = small_problem(seed=52)
    e, _, _ = run(acts, labels, T, S, wb, we, alignment=alignment, k=k)
    post = run_posteriors(acts, labels, T, S, alignment, k)
    rows = np.asarray(post.blank, np.float64) * wb + np.asarray(post.label, np.float64) * we
    ref = np.array([rows[utt_of_row(T, S) == b].sum() for b in range(len(T))])
    assert_expected(e, ref, cost_bound(wb, we, T, S))


def check_costs_identity(run, run_loss):
    """The costs output is monotonic_rnnt_loss's, bit for bit, and at g_e = 0 the gradient is the loss's within
    GRAD_TOL. run_loss(acts, labels, T, S, gc) -> (costs, grads)."""
    acts, labels, T, S, wb, we = small_problem(seed=53)
    gc = np.array([1.0, -0.5, 2.0, 0.25], np.float32)
    _, c, g = run(acts, labels, T, S, wb, we, 0 * gc, gc)
    lc, lg = run_loss(acts, labels, T, S, gc)
    assert c.tobytes() == lc.tobytes()
    tol = GRAD_TOL * np.abs(gc)[utt_of_row(T, S)][:, None]
    assert np.all(np.abs(g.astype(np.float64) - lg) <= tol), float(np.abs(g - lg).max())


def check_constant_costs(run):
    """wb = we = c_b: every path costs c_b T_b -- expected = c_b T_b and its gradient is within tolerance of 0."""
    acts, labels, T, S, _, _ = small_problem(seed=54)
    cval = np.array([1.0, -2.5, 0.375, 3.0])
    w = cval[utt_of_row(T, S)].astype(np.float32)
    one = np.ones(len(T), np.float32)
    e, _, g = run(acts, labels, T, S, w, w, one, 0 * one)
    Wb = cost_bound(w, w, T, S)
    assert_expected(e, cval * T, Wb)
    assert np.all(np.abs(g) <= grad_tol(T, S, Wb, one, 0 * one))


def check_negation(run):
    """Costs scaled by -1 negate expected and its gradient."""
    acts, labels, T, S, wb, we = small_problem(seed=55)
    one = np.ones(len(T), np.float32)
    e, _, g = run(acts, labels, T, S, wb, we, one, 0 * one)
    en, _, gn = run(acts, labels, T, S, -wb, -we, one, 0 * one)
    Wb = cost_bound(wb, we, T, S)
    assert np.all(np.abs(e.astype(np.float64) + en) <= COST_TOL + 4e-6 * Wb)
    assert np.all(np.abs(g.astype(np.float64) + gn) <= grad_tol(T, S, Wb, one, 0 * one))
    assert np.any(np.abs(g) > 1e-3)  # (there is something to negate)


# ---- 4. two upstreams in one pass -------------------------------------------------------------------------------------

def check_two_upstreams(run, **kw):
    """Signed per-utterance a, b together (the edge cases do that too), then b = 0 and a = 0 each alone."""
    acts, labels, T, S, wb, we = small_problem(seed=56)
    rng = np.random.default_rng(57)
    a, b = upstreams(rng, len(T))
    for ge, gc in ((a, b), (a, 0 * b), (0 * a, b)):
        check_against_yardstick(run, acts, labels, T, S, wb, we, ge, gc, **kw)
    # neither: every gradient row is exactly zero
    _, _, g = run(acts, labels, T, S, wb, we, 0 * a, 0 * b, **kw)
    assert np.all(g == 0.0)


# ---- 5. restriction ---------------------------------------------------------------------------------------------------

def path_cost(al_row, lab, Tb, Sb, wb, we):
    s, f = 0, 0.0
    for t in range(Tb):
        if al_row[t] == BLANK:
            f += float(wb[t, s])
        else:
            f += float(we[t, s])
            s += 1
    assert s == Sb
    return f


def check_restriction(run, run_posteriors):
    acts, labels, T, S, wb, we = small_problem(seed=58)
    off = offsets(T, S)
    al, _ = A.run_cpu(acts, labels, T, S)  # a valid alignment: the best path
    one = np.ones(len(T), np.float32)
    Wb = cost_bound(wb, we, T, S)
    # k = 0: a point mass on that path
    e, _, g = run(acts, labels, T, S, wb, we, one, 0 * one, alignment=al, k=0)
    ref = np.array([path_cost(al[b], labels[b], int(T[b]), int(S[b]),
                              wb[off[b]:off[b + 1]].reshape(T[b], S[b] + 1), we[off[b]:off[b + 1]].reshape(T[b], S[b] + 1))
                    for b in range(len(T))])
    assert_expected(e, ref, Wb)
    assert np.all(np.abs(g) <= grad_tol(T, S, Wb, one, 0 * one))
    # k >= T: the unrestricted call
    ge, gc = upstreams(np.random.default_rng(59), len(T))
    eu, cu, gu = run(acts, labels, T, S, wb, we, ge, gc)
    ek, ck, gk = run(acts, labels, T, S, wb, we, ge, gc, alignment=al, k=int(T.max()))
    assert np.all(np.abs(ek.astype(np.float64) - eu) <= COST_TOL + 4e-6 * Wb)
    assert_costs(ck, cu.astype(np.float64))
    assert np.all(np.abs(gk.astype(np.float64) - gu) <= grad_tol(T, S, Wb, ge, gc))
    # k = 1: the posteriors identity under the restricted distribution
    check_posteriors_identity(run, run_posteriors, alignment=al, k=1)


# ---- 6. non-finite ----------------------------------------------------------------------------------------------------

def _without(b, acts, labels, T, S, wb, we):
    off = offsets(T, S)
    keep = np.ones(len(acts), bool)
    keep[off[b]:off[b + 1]] = False
    kb = [i for i in range(len(T)) if i != b]
    return acts[keep], labels[kb], T[kb], S[kb], wb[keep], we[keep], keep


def check_non_finite(run):
    acts, labels, T, S, wb, we = small_problem(seed=60)
    off = offsets(T, S)
    e0, c0, g0 = run(acts, labels, T, S, wb, we)
    for how in ("nan_logit", "masked_label"):
        bad = acts.copy()
        if how == "nan_logit":  # row (3, 2) of utterance 0 (T = 23, S = 9) is inside its band
            bad[off[0] + 3 * (S[0] + 1) + 2, 5] = np.nan
        else:                    # label 0 of utterance 0 masked in every row (t, 0): no path survives
            bad[off[0]:off[1]].reshape(T[0], S[0] + 1, -1)[:, 0, labels[0, 0]] = -np.inf
        e, c, g = run(bad, labels, T, S, wb, we)
        assert np.isnan(e[0]) and np.all(np.isnan(g[off[0]:off[1]])), how
        # the others: bit-identical to a call without that utterance
        a1, l1, T1, S1, wb1, we1, keep = _without(0, acts, labels, T, S, wb, we)
        e1, c1, g1 = run(a1, l1, T1, S1, wb1, we1)
        assert e[1:].tobytes() == e1.tobytes() and c[1:].tobytes() == c1.tobytes(), how
        assert g[keep].tobytes() == g1.tobytes(), how
        assert e[1:].tobytes() == e0[1:].tobytes() and g[keep].tobytes() == g0[keep].tobytes()
    # -inf logits off every path's arcs (the rows outside the band) change nothing
    from _parity import band_mask
    out = ~band_mask(T, S)
    assert out.any()
    off_band = acts.copy()
    off_band[out] = -np.inf
    e, c, g = run(off_band, labels, T, S, wb, we)
    assert e.tobytes() == e0.tobytes() and c.tobytes() == c0.tobytes() and g.tobytes() == g0.tobytes()
    assert np.all(g[out] == 0.0)


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------

def check_reproducible(run):
    """Two runs are bitwise equal; an utterance alone equals itself inside a batch."""
    acts, labels, T, S, wb, we = small_problem(seed=61)
    ge, gc = upstreams(np.random.default_rng(62), len(T))
    r1 = run(acts, labels, T, S, wb, we, ge, gc)
    r2 = run(acts, labels, T, S, wb, we, ge, gc)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r1, r2))
    off = offsets(T, S)
    for b in range(len(T)):
        sl = slice(int(off[b]), int(off[b + 1]))
        e, c, g = run(acts[sl], labels[b:b + 1, :max(1, int(S[b]))], T[b:b + 1], S[b:b + 1], wb[sl], we[sl],
                      ge[b:b + 1], gc[b:b + 1])
        assert e.tobytes() == r1[0][b:b + 1].tobytes() and c.tobytes() == r1[1][b:b + 1].tobytes(), b
        assert g.tobytes() == r1[2][sl].tobytes(), b
    return acts, labels, T, S, wb, we, ge, gc, r1


def check_padded(run, V):
    """The padded 4-D layout (NaN in the padding rows of acts and of the cost arrays) equals the packed result bit for
    bit; the gradient's padding rows are 0."""
    acts, labels, T, S, wb, we = small_problem(seed=63, V=V)
    ge, gc = upstreams(np.random.default_rng(64), len(T))
    e, c, g = run(acts, labels, T, S, wb, we, ge, gc)
    pad_T, pad_S1 = int(T.max()) + 2, int(S.max()) + 3
    pad = lambda x: pack_to_padded(x, T, S, pad_T, pad_S1, np.nan)  # noqa: E731
    ep, cp, gp = run(pad(acts), labels, T, S, pad(wb[:, None])[..., 0], pad(we[:, None])[..., 0], ge, gc)
    assert gp.shape == (len(T), pad_T, pad_S1, V)
    assert ep.tobytes() == e.tobytes() and cp.tobytes() == c.tobytes()
    assert padded_to_packed(gp, T, S).tobytes() == g.tobytes()
    mask = np.ones(gp.shape[:3], bool)
    for b in range(len(T)):
        mask[b, : T[b], : S[b] + 1] = False
    assert np.all(gp[mask] == 0.0)


# ---- the host implementation ------------------------------------------------------------------------------------------

def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def run_cpu(acts, labels, T, S, wb, we, ge=None, gc=None, alignment=None, k=0):
    """`run` on the host implementation (CPU tensors; 2-D packed or 4-D padded acts)."""
    import monotonic_rnnt_op as op
    a = _t(acts).requires_grad_(True)
    e, c = op.monotonic_rnnt_expected_cost(a, _t(labels), _t(T), _t(S), _t(wb), _t(we), _t(alignment), k, BLANK)
    B = len(T)
    assert e.dtype == torch.float32 and c.dtype == torch.float32 and e.shape == (B,) and c.shape == (B,)
    assert e.requires_grad and c.requires_grad
    one = torch.ones(B)
    torch.autograd.backward((e, c), (one if ge is None else _t(np.asarray(ge, np.float32)),
                                     one if gc is None else _t(np.asarray(gc, np.float32))))
    return e.detach().numpy(), c.detach().numpy(), a.grad.numpy()


def posteriors_cpu(acts, labels, T, S, alignment=None, k=0):
    import monotonic_rnnt_op as op
    return op.monotonic_rnnt_posteriors(_t(acts), _t(labels), _t(T), _t(S), _t(alignment), k, BLANK)


def loss_cpu(acts, labels, T, S, gc):
    import monotonic_rnnt_op as op
    a = _t(acts).requires_grad_(True)
    c = op.monotonic_rnnt_loss(a, _t(labels), _t(T), _t(S), None, 0, BLANK)
    c.backward(_t(np.asarray(gc, np.float32)))
    return c.detach().numpy(), a.grad.numpy().astype(np.float64)
