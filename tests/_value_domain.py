"""Shared case builders and bounds of the value-domain tests (test_cpu_value_domain.py, test_gpu_value_domain.py):
logits outside the N(0,1) range every other parity test draws from -- large common offsets, sharply peaked and
constant rows, denormals, -inf masks, and NaN / +inf poison.

A problem is (acts, labels, T, S) as _parity.random_problem makes it: packed fp32 acts [sum_b T_b (S_b + 1), V],
labels != blank (= 0). A transform is a function (acts, labels, T, S) -> acts that returns a new array and leaves its
input alone (mask_label alone returns (acts, labels): it redraws labels).

Bounds (derived here, not fitted to any implementation's output):

grad_tol   The gradient is g[v] = e^(z[v] + den + alpha + beta - ll) - corrections, an exp term <= 1 whose exponent
           an implementation with fp32 per-row state forms from terms of size |z|: the row's denominator stored as
           fp32 contributes 2^-24 |z| to the exponent, the per-row coefficient (den + alpha + beta - ll) rounded to
           fp32 another 2^-24 |z|, and a float log2(e) against a double one (1.3e-8 relative) 0.22 * 2^-24 |z| --
           2.22 * 2^-24 |z| in all, rounded up to 2^-22 max|z|, on a term <= 1: absolute.
           For max|z| <= 128 this is <= 3.1e-5 and is NOT granted: those cases hold the project's plain 1e-4. (The
           issue draws the line at |z| <= 100 and means offset(+-100) by it; N(0,1) + 100 reaches ~104, so the line
           is put at 128 on purpose -- stricter, never looser. scale(30) reaches ~135 and gets a term of ~3e-5.)
cost_tol   A log-softmax that folds the row maximum into the exponent as one rounded fp32 offset (-M log2 e) puts a
           common error of 2^-24 |M| log2(e) ln(2) = 2^-24 |M| on every term of the row, i.e. on the row's
           denominator; a path crosses T_b rows, so with no cancellation assumed, and doubled, T_b 2^-23 max|z|,
           granted above max|z| = 128 only, on top of the standing 1e-4 max(1, |c|).
"""
import math

import numpy as np

from _parity import COST_TOL, GRAD_TOL, assert_costs, random_problem

NAN = float("nan")
INF = float("inf")
WIDE_ABOVE = 128.0  # max|z| up to which the plain project tolerances hold: offsets of +-100 on N(0,1) stay below it


# ---- problems -------------------------------------------------------------------------------------------------------

def base_problem(seed, B, Trange, Smax, V, force=None):
    """N(0,1) fp32 acts, ragged T and S, labels in [1, V - 1) (never the blank 0; column V - 1 stays free of labels so
    that mask_unused can always mask it, V >= 3)."""
    rng = np.random.default_rng(seed)
    acts, labels, T, S = random_problem(rng, B, Trange, Smax, V, force=force)
    if V >= 3:
        labels = np.where(labels == V - 1, 1 + (labels + np.arange(labels.shape[1])[None, :]) % (V - 2), labels)
    return acts, labels.astype(np.int32), T, S


def row_offsets_of(T, S):
    """First packed row of every utterance (and the total), int64 [B + 1]."""
    n = np.asarray(T, np.int64) * (np.asarray(S, np.int64) + 1)
    return np.concatenate([[0], np.cumsum(n)])


def utt_rows(T, S, b):
    off = row_offsets_of(T, S)
    return slice(int(off[b]), int(off[b + 1]))


def row_of(T, S, b, t, s):
    return int(row_offsets_of(T, S)[b]) + int(t) * (int(S[b]) + 1) + int(s)


def band_positions(T, S):
    """In-band rows (t, s) of one utterance -- max(0, t - (T - S)) <= s <= min(t, S), the rows a log-softmax must
    reduce -- as [(t, s, kind)]: `first` (0, 0), `last` (T - 1, S), `lower_edge` (s = lo), `upper_edge` (s = hi),
    `interior`. A row that is both edges (lo == hi) is listed as lower_edge."""
    out = []
    for t in range(int(T)):
        lo, hi = max(0, t - (int(T) - int(S))), min(t, int(S))
        for s in range(lo, hi + 1):
            if (t, s) == (0, 0):
                kind = "first"
            elif (t, s) == (int(T) - 1, int(S)):
                kind = "last"
            elif s == lo:
                kind = "lower_edge"
            elif s == hi:
                kind = "upper_edge"
            else:
                kind = "interior"
            out.append((t, s, kind))
    return out


def pick_positions(T, S, per_kind=3):
    """Every first and last row and up to per_kind rows of each other kind, spread over the kind's rows (the first,
    the last and the ones between, evenly)."""
    pos = band_positions(T, S)
    out = [p for p in pos if p[2] in ("first", "last")]
    for kind in ("lower_edge", "upper_edge", "interior"):
        rows = [p for p in pos if p[2] == kind]
        if len(rows) > per_kind:
            idx = sorted({round(i * (len(rows) - 1) / (per_kind - 1)) for i in range(per_kind)}) if per_kind > 1 else [0]
            rows = [rows[i] for i in idx]
        out += rows
    return out


# ---- transforms -----------------------------------------------------------------------------------------------------

def offset(M):
    def f(acts, labels, T, S):
        return (acts + np.float32(M)).astype(np.float32)
    f.__name__ = f"offset({M:g})"
    return f


def row_offsets(M, seed=0):
    def f(acts, labels, T, S):
        off = np.random.default_rng(seed).uniform(-M, M, acts.shape[0]).astype(np.float32)
        return (acts + off[:, None]).astype(np.float32)
    f.__name__ = f"row_offsets({M:g})"
    return f


def scale(k):
    def f(acts, labels, T, S):
        return (acts * np.float32(k)).astype(np.float32)
    f.__name__ = f"scale({k:g})"
    return f


def constant(c):
    def f(acts, labels, T, S):
        return np.full_like(acts, np.float32(c))
    f.__name__ = f"constant({c:g})"
    return f


def denormal(acts, labels, T, S):
    return (acts.astype(np.float64) * 1e-40).astype(np.float32)


def unused_columns(labels, V, blank=0):
    used = set(np.asarray(labels).reshape(-1).tolist()) | {blank}
    return np.array([v for v in range(V) if v not in used], np.int64)


def mask_unused(frac=0.5, seed=0):
    """-inf on a random `frac` of the columns that are neither the blank nor any label of the batch, column V - 1 --
    the last element of the last 16-byte vector of a row, whatever the element type -- always among them."""
    def f(acts, labels, T, S):
        V = acts.shape[1]
        free = unused_columns(labels, V)
        assert V - 1 in free, "base_problem keeps column V - 1 free of labels"
        rest = free[free != V - 1]
        n = max(0, int(round(frac * len(free))) - 1)
        cols = np.concatenate([[V - 1], np.random.default_rng(seed).choice(rest, n, replace=False)]).astype(np.int64)
        out = acts.copy()
        out[:, cols] = -INF
        return out
    f.__name__ = f"mask_unused({frac:g})"
    return f


def mask_label(b, seed=0):
    """-inf on the column of utterance b's first label, in the rows of utterance b (so every other utterance's logits
    are the base acts', bit for bit); the other utterances' labels are redrawn to avoid that column. Returns
    (acts, labels): compare against the base acts with the returned labels."""
    def f(acts, labels, T, S):
        assert S[b] >= 1
        V = acts.shape[1]
        col = int(labels[b, 0])
        rng = np.random.default_rng(seed)
        lab = labels.copy()
        for o in range(len(T)):
            if o == b:
                continue
            hit = lab[o] == col
            if hit.any() and V > 3:
                lab[o, hit] = rng.choice([v for v in range(1, V - 1) if v != col], int(hit.sum()))
        out = acts.copy()
        out[utt_rows(T, S, b), col] = -INF
        return out, lab
    f.__name__ = f"mask_label({b})"
    return f


def mask_blank_rows(b, blank=0):
    """-inf on the blank column in the rows of utterance b only (T_b > S_b: every path takes a blank)."""
    def f(acts, labels, T, S):
        assert T[b] > S[b]
        out = acts.copy()
        out[utt_rows(T, S, b), blank] = -INF
        return out
    f.__name__ = f"mask_blank_rows({b})"
    return f


def poison(b, t, s, value, v=None):
    """One element (column v, default V - 1) of in-band row (t, s) of utterance b set to `value` (NaN or +inf)."""
    def f(acts, labels, T, S):
        out = acts.copy()
        out[row_of(T, S, b, t, s), acts.shape[1] - 1 if v is None else v] = value
        return out
    f.__name__ = f"poison({b},{t},{s},{value})"
    return f


def all_neg_inf_row(b, t, s):
    def f(acts, labels, T, S):
        out = acts.copy()
        out[row_of(T, S, b, t, s), :] = -INF
        return out
    f.__name__ = f"all_neg_inf_row({b},{t},{s})"
    return f


OFFSETS = [100.0, -100.0, 1e3, 1e4, -1e4]
ROW_OFFSETS = [100.0, 1e3]
SCALES = [10.0, 30.0, 100.0, 1000.0]
CONSTANTS = [0.0, 3.5, -1e4]


# ---- classes and bounds ---------------------------------------------------------------------------------------------

def cost_class(c):
    """Per utterance: 'finite', '+inf', '-inf' or 'nan'."""
    c = np.atleast_1d(np.asarray(c, np.float64))
    out = np.full(c.shape, "finite", dtype=object)
    out[np.isposinf(c)] = "+inf"
    out[np.isneginf(c)] = "-inf"
    out[np.isnan(c)] = "nan"
    return out


def as_f32_costs(ref):
    """The reference costs as the op can return them: fp32."""
    with np.errstate(over="ignore"):
        return np.asarray(ref, np.float64).astype(np.float32).astype(np.float64)


def assert_costs_classed(c, ref, tol=None):
    """_parity.assert_costs plus the class of every non-finite cost: +inf (no alignment path) and NaN (bad input) are
    different answers. tol: per-utterance absolute bounds (cost_tol) in place of the standing 1e-4 max(1, |c|)."""
    c = np.asarray(c, np.float64)
    ref = as_f32_costs(ref)
    got, want = cost_class(c), cost_class(ref)
    assert np.array_equal(got, want), (list(got), list(want), c, ref)
    if tol is None:
        assert_costs(c, ref)
        return
    fin = np.isfinite(ref)
    if fin.any():
        err = np.abs(c[fin] - ref[fin])
        assert np.all(err <= np.asarray(tol, np.float64)[fin]), (err, np.asarray(tol)[fin], c, ref)


def max_abs_finite(acts):
    a = np.abs(np.asarray(acts, np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def grad_tol(acts_f32, dtype="f32"):
    """(absolute, relative) gradient bound for these logits: |g - ref| <= absolute + relative |ref|. See the module
    docstring. relative is the one rounding of the gradient to the acts type (as test_gpu_fuzz.check_case)."""
    z = max_abs_finite(acts_f32)
    extra = 2.0 ** -22 * z if z > WIDE_ABOVE else 0.0
    return GRAD_TOL + extra, {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}[dtype]


def cost_tol(c_ref, T, acts):
    """Per-utterance absolute cost bound [B]. See the module docstring."""
    c = np.abs(as_f32_costs(c_ref))
    c = np.where(np.isfinite(c), c, 1.0)
    z = max_abs_finite(acts)
    extra = np.asarray(T, np.float64) * 2.0 ** -23 * z if z > WIDE_ABOVE else 0.0
    return COST_TOL * np.maximum(1.0, c) + extra


def assert_grads_tol(g, ref, absolute, relative=0.0):
    """_parity.assert_grads with a relative term: the same non-finite places, |g - ref| <= absolute + relative |ref|."""
    assert g.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(g), fin), np.argwhere(np.isfinite(g) != fin)[:8]
    if fin.any():
        err = np.abs(g[fin] - ref[fin])
        assert np.all(err <= absolute + relative * np.abs(ref[fin])), (err.max(), absolute)


def closed_form_cost(T, S, V):
    """Every logit of every row equal: each transition has probability 1 / V and there are C(T, S) monotonic paths
    (which S of the T frames emit), so the cost is T ln V - ln C(T, S)."""
    return int(T) * math.log(V) - math.log(math.comb(int(T), int(S)))


def assert_poisoned_grads(g, ref, absolute):
    """The gradient rows of an utterance whose cost is NaN: no finite garbage -- every element is NaN, or equals the
    reference where the reference is finite."""
    ok = np.isnan(g) | (np.isfinite(ref) & (np.abs(g - np.where(np.isfinite(ref), ref, 0.0)) <= absolute))
    assert ok.all(), (np.argwhere(~ok)[:8], g[~ok][:8])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
