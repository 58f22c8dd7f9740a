"""Checks of monotonic_rnnt_posteriors shared by tests/test_cpu_posteriors.py and tests/test_gpu_posteriors.py (only
the device differs): a numpy fp64 forward-backward yardstick over log_softmax of the acts upcast to fp64, and the
property checks built on it and on the CPU oracle.

`run(acts, labels, T, S, alignment=None, k=0, max_input_length=None)` -> Posteriors(blank [N], label [N],
emit [B, L], label_time [B, labels.shape[1]], costs [B]) as numpy arrays; the inputs are numpy arrays.

Tolerances (absolute). blank / label / emit: GRAD_TOL, the project's gradient tolerance -- the gradient's per-row
coefficients are these very numbers. label_time: GRAD_TOL * max(1, T_b), a sum with weights up to T_b - 1. costs:
assert_costs. Non-finite entries must sit in the same places. The invariants take the bounds these imply: a sum of n
values, each within GRAD_TOL of numbers that sum exactly to the target, is within n * GRAD_TOL of it.
"""
import collections
import itertools

import numpy as np

import oracle
from _align_checks import BLANK, band_of, boundary_problem, offsets, ragged  # noqa: F401  (re-exported)
from _parity import GRAD_TOL, assert_costs

Posteriors = collections.namedtuple("Posteriors", ["blank", "label", "emit", "label_time", "costs"])
NEG = -np.inf


def run_cpu(acts, labels, T, S, alignment=None, k=0, max_input_length=None):
    """`run` on the host implementation (CPU tensors)."""
    import torch

    import monotonic_rnnt_op as op
    out = op.monotonic_rnnt_posteriors(
        torch.from_numpy(acts), torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S),
        alignment=None if alignment is None else torch.from_numpy(alignment), max_distance_from_alignment=k,
        blank_label=BLANK, max_input_length=max_input_length)
    assert out._fields == Posteriors._fields
    assert all(x.dtype == torch.float32 and not x.requires_grad for x in out)
    assert out.blank.shape == acts.shape[:-1] and out.label.shape == acts.shape[:-1]
    return Posteriors(*(x.numpy() for x in out))


def np_posteriors(acts, labels, T, S, blank=BLANK, bands=None):
    """The yardstick: fp64 forward-backward per utterance, vectorised over s. bands[b] = (min_s [T_b], max_s [T_b]),
    the band of the state after frame t (band_of). Returns Posteriors with emit / label_time as lists of per-utterance
    arrays ([T_b] / [S_b]) and costs fp64, plus `reach` [N]: the rows with alpha(t-1, s) and beta(t, s) above -inf."""
    off = offsets(T, S)
    N = int(off[-1])
    out_b, out_l, reach_all = np.zeros(N), np.zeros(N), np.zeros(N, bool)
    emit, ltime, costs = [], [], np.zeros(len(T))
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        Tb, Sb = int(Tb), int(Sb)
        W = Sb + 1
        z = np.asarray(acts[off[b]:off[b + 1]], np.float64)
        s = np.arange(W)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mx = z.max(axis=1)
            den = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
            lab = np.concatenate([np.asarray(labels[b, :Sb], np.int64), [blank]])
            lpb = (z[:, blank] - den).reshape(Tb, W)
            lpe = (z[np.arange(Tb * W), np.tile(lab, Tb)] - den).reshape(Tb, W)
            lpe[:, Sb] = NEG  # no label arc out of s = S
            A = np.full((Tb + 1, W), NEG)  # A[t + 1] = alpha(t, .), A[0] = alpha(-1, .)
            A[0, 0] = 0.0
            for t in range(Tb):
                a = np.logaddexp(A[t] + lpb[t], np.concatenate([[NEG], A[t, :-1] + lpe[t, :-1]]))
                if bands is not None:
                    a = np.where((s >= int(bands[b][0][t])) & (s <= int(bands[b][1][t])), a, NEG)
                A[t + 1] = a
            Bt = np.full((Tb + 1, W), NEG)  # Bt[t] = beta(t, .): the state before frame t, i.e. after frame t - 1
            Bt[Tb, Sb] = 0.0
            for t in range(Tb - 1, -1, -1):
                v = np.logaddexp(Bt[t + 1] + lpb[t], np.concatenate([Bt[t + 1, 1:], [NEG]]) + lpe[t])
                if t == 0:
                    v = np.where(s == 0, v, NEG)
                elif bands is not None:
                    v = np.where((s >= int(bands[b][0][t - 1])) & (s <= int(bands[b][1][t - 1])), v, NEG)
                Bt[t] = v
            ll = A[Tb, Sb]
            costs[b] = -ll
            reach = (A[:Tb] != NEG) & (Bt[:Tb] != NEG)
            bp = np.where(reach, np.exp(A[:Tb] + lpb + Bt[1:] - ll), 0.0)
            nxt = np.concatenate([Bt[1:, 1:], np.full((Tb, 1), NEG)], axis=1)
            ep = np.where(reach, np.exp(A[:Tb] + lpe + nxt - ll), 0.0)
        if not np.isfinite(ll):
            bp, ep = np.full((Tb, W), np.nan), np.full((Tb, W), np.nan)
        out_b[off[b]:off[b + 1]] = bp.reshape(-1)
        out_l[off[b]:off[b + 1]] = ep.reshape(-1)
        reach_all[off[b]:off[b + 1]] = reach.reshape(-1)
        emit.append(ep.sum(axis=1))
        ltime.append((np.arange(Tb)[:, None] * ep).sum(axis=0)[:Sb])
    out = Posteriors(out_b, out_l, emit, ltime, costs)
    return out, reach_all


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, np.argwhere(np.isfinite(got) != fin)[:5])
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    assert err <= tol, (what, err, tol)
    return err


def compare(res, ref, T, S, what=""):
    """res (the library, padded emit / label_time) against ref (np_posteriors / brute force, per-utterance lists)."""
    _close(res.blank.reshape(-1), ref.blank, GRAD_TOL, what + " blank")
    _close(res.label.reshape(-1), ref.label, GRAD_TOL, what + " label")
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        Tb, Sb = int(Tb), int(Sb)
        _close(res.emit[b, :Tb], ref.emit[b], GRAD_TOL, f"{what} emit[{b}]")
        assert np.all(res.emit[b, Tb:] == 0.0), (what, b)
        _close(res.label_time[b, :Sb], ref.label_time[b], GRAD_TOL * max(1, Tb), f"{what} label_time[{b}]")
        assert np.all(res.label_time[b, Sb:] == -1.0), (what, b)
    assert_costs(res.costs, np.asarray(ref.costs, np.float64))


def check_invariants(res, T, S):
    """3. Per-frame sum 1, per-label sum 1, sum_t emit = S_b, label_time increasing by at least one frame per label
    (label s + 1 is emitted strictly after label s on every path) -- for the utterances with a finite cost."""
    off = offsets(T, S)
    blank, label = res.blank.reshape(-1).astype(np.float64), res.label.reshape(-1).astype(np.float64)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        Tb, Sb = int(Tb), int(Sb)
        if not np.isfinite(res.costs[b]):
            continue
        bp = blank[off[b]:off[b + 1]].reshape(Tb, Sb + 1)
        ep = label[off[b]:off[b + 1]].reshape(Tb, Sb + 1)
        assert np.all(ep[:, Sb] == 0.0)
        n_band = min(Sb, Tb - Sb) + 1  # in-band rows of a frame, at most; two arcs each
        assert np.abs((bp + ep).sum(axis=1) - 1.0).max() <= 2 * n_band * GRAD_TOL, b
        if Sb:
            assert np.abs(ep[:, :Sb].sum(axis=0) - 1.0).max() <= (Tb - Sb + 1) * GRAD_TOL, b
            lt = res.label_time[b, :Sb].astype(np.float64)
            assert np.all(np.diff(lt) >= 1.0 - 2 * GRAD_TOL * Tb), (b, lt)
            assert lt[0] >= -GRAD_TOL * Tb and lt[-1] <= Tb - 1 + GRAD_TOL * Tb
        assert abs(res.emit[b, :Tb].astype(np.float64).sum() - Sb) <= Tb * GRAD_TOL, b


def check_all(run, acts, labels, T, S, alignment=None, k=0, **kw):
    """The library against the yardstick (banded when an alignment is given), plus the invariants."""
    res = run(acts, labels, T, S, alignment=alignment, k=k, **kw)
    bands = None if alignment is None else [band_of(alignment[b], int(T[b]), k) for b in range(len(T))]
    ref, reach = np_posteriors(acts, labels, T, S, bands=bands)
    compare(res, ref, T, S)
    fin = np.repeat(np.isfinite(ref.costs), np.asarray(T, np.int64) * (np.asarray(S, np.int64) + 1))
    dead = ~reach & fin  # unreachable rows of utterances with a path: exactly 0
    assert np.all(res.blank.reshape(-1)[dead] == 0.0) and np.all(res.label.reshape(-1)[dead] == 0.0)
    check_invariants(res, T, S)
    return res, ref


def check_brute_force_tiny(run):
    """1. Every one of the C(T, S) alignments priced by the oracle at k = 0; the arc posteriors are the normalised sums
    of the path probabilities through each arc. Rests on the oracle alone: the library must match it, and so must the
    yardstick."""
    rng = np.random.default_rng(3)
    shapes = [(1, 0), (1, 1), (5, 2), (6, 6), (7, 0), (9, 4)]
    acts, labels, T, S = ragged(rng, shapes, 6)
    off = offsets(T, S)
    every = []
    for b, (Tb, Sb) in enumerate(shapes):
        every.append([frames for frames in itertools.combinations(range(Tb), Sb)])
    n = max(len(r) for r in every)
    assert n <= 126
    bp, ep, tot = np.zeros(int(off[-1])), np.zeros(int(off[-1])), np.zeros(len(shapes))
    for i in range(n):  # call i prices alignment i (mod its count) of every utterance
        cand = np.full((len(shapes), int(T.max())), BLANK, np.int32)
        for b, rows in enumerate(every):
            cand[b, list(rows[i % len(rows)])] = labels[b, :shapes[b][1]]
        c, _ = oracle.oracle_rnnt(acts, labels, T, S, alignment=cand, max_shift=0, grads=False)
        for b, rows in enumerate(every):
            if i >= len(rows):
                continue
            p = np.exp(-c[b])
            tot[b] += p
            s, Tb, Sb = 0, *shapes[b]
            for t in range(Tb):
                r = off[b] + t * (Sb + 1) + s
                if t in rows[i]:
                    ep[r] += p
                    s += 1
                else:
                    bp[r] += p
    scale = np.repeat(tot, T.astype(np.int64) * (S + 1))
    bp, ep = bp / scale, ep / scale
    emit, ltime = [], []
    for b, (Tb, Sb) in enumerate(shapes):
        e = ep[off[b]:off[b + 1]].reshape(Tb, Sb + 1)
        emit.append(e.sum(axis=1))
        ltime.append((np.arange(Tb)[:, None] * e).sum(axis=0)[:Sb])
    brute = Posteriors(bp, ep, emit, ltime, -np.log(tot))
    yard, _ = np_posteriors(acts, labels, T, S)
    assert np.abs(yard.blank - bp).max() <= 1e-12 and np.abs(yard.label - ep).max() <= 1e-12  # yardstick vs oracle
    res = run(acts, labels, T, S)
    compare(res, brute, T, S, "brute force")
    check_invariants(res, T, S)


def check_gradient_identity(run):
    """2. g = (bp + ep) softmax - onehot_blank bp - onehot_label ep reproduces the oracle's fp64 gradient, every row
    within GRAD_TOL."""
    rng = np.random.default_rng(21)
    shapes = [(12, 4), (7, 0), (9, 9), (70, 64), (1, 1), (1, 0), (33, 5)]
    acts, labels, T, S = ragged(rng, shapes, 8)
    res, _ = check_all(run, acts, labels, T, S)
    _, g = oracle.oracle_rnnt(acts, labels, T, S, grads=True)
    z = acts.astype(np.float64)
    sm = np.exp(z - z.max(axis=1, keepdims=True))
    sm /= sm.sum(axis=1, keepdims=True)
    bp, ep = res.blank.astype(np.float64), res.label.astype(np.float64)
    pred = (bp + ep)[:, None] * sm
    pred[:, BLANK] -= bp
    off = offsets(T, S)
    for b, (Tb, Sb) in enumerate(shapes):
        for s in range(Sb):
            rows = off[b] + np.arange(Tb) * (Sb + 1) + s
            pred[rows, labels[b, s]] -= ep[rows]
    err = np.abs(pred - g).max(axis=1)
    assert err.max() <= GRAD_TOL, (err.max(), int(err.argmax()))


def check_restriction(run):
    """4. A random given alignment: k = 0 leaves its 0/1 indicators, k in {1, 3} the banded yardstick with exact zeros
    outside the band, k >= T the unrestricted result bit for bit."""
    rng = np.random.default_rng(6)
    shapes = [(23, 9), (17, 17), (12, 0), (30, 4)]
    acts, labels, T, S = ragged(rng, shapes, 8)
    off = offsets(T, S)
    given = np.full((len(shapes), int(T.max())), BLANK, np.int32)
    frames = []
    for b, (Tb, Sb) in enumerate(shapes):
        frames.append(np.sort(rng.choice(Tb, Sb, replace=False)))
        given[b, frames[b]] = labels[b, :Sb]
    free = run(acts, labels, T, S)
    res, _ = check_all(run, acts, labels, T, S, alignment=given, k=0)
    ind_b, ind_l = np.zeros(int(off[-1]), np.float32), np.zeros(int(off[-1]), np.float32)
    for b, (Tb, Sb) in enumerate(shapes):
        s = 0
        for t in range(Tb):
            r = off[b] + t * (Sb + 1) + s
            if given[b, t] != BLANK:
                ind_l[r] = 1.0
                s += 1
            else:
                ind_b[r] = 1.0
        assert np.array_equal(res.label_time[b, :Sb], frames[b].astype(np.float32)), b
        assert np.array_equal(res.emit[b, :Tb], (given[b, :Tb] != BLANK).astype(np.float32)), b
    assert np.array_equal(res.blank.reshape(-1), ind_b) and np.array_equal(res.label.reshape(-1), ind_l)
    for k in (1, 3):
        check_all(run, acts, labels, T, S, alignment=given, k=k)  # (asserts the exact zeros outside the band)
    wide = run(acts, labels, T, S, alignment=given, k=int(T.max()))
    for x, y in zip(wide, free):
        assert x.tobytes() == y.tobytes()


def check_value_domain(run):
    """5. -inf and NaN logits: all NaN for their utterances, the clean one bit-identical to the clean run."""
    rng = np.random.default_rng(7)
    acts, labels, T, S = ragged(rng, [(11, 4), (9, 3), (8, 2)], 8)
    off = offsets(T, S)
    clean = run(acts, labels, T, S)
    bad = acts.copy()
    rows1 = off[1] + np.arange(int(T[1])) * (int(S[1]) + 1)  # rows (t, 0) of utterance 1: where label 0 is emitted
    bad[rows1, labels[1, 0]] = -np.inf
    bad[off[2], 3] = np.nan                                   # row (0, 0) of utterance 2: in every band
    res, ref = check_all(run, bad, labels, T, S)
    assert res.costs[1] == np.inf and np.isnan(res.costs[2])
    for b in (1, 2):
        Tb, Sb = int(T[b]), int(S[b])
        assert np.all(np.isnan(res.blank.reshape(-1)[off[b]:off[b + 1]]))
        assert np.all(np.isnan(res.label.reshape(-1)[off[b]:off[b + 1]]))
        assert np.all(np.isnan(res.emit[b, :Tb])) and np.all(res.emit[b, Tb:] == 0.0)
        assert np.all(np.isnan(res.label_time[b, :Sb])) and np.all(res.label_time[b, Sb:] == -1.0)
    assert res.blank.reshape(-1)[:off[1]].tobytes() == clean.blank.reshape(-1)[:off[1]].tobytes()
    assert res.label.reshape(-1)[:off[1]].tobytes() == clean.label.reshape(-1)[:off[1]].tobytes()
    assert res.emit[0].tobytes() == clean.emit[0].tobytes()
    assert res.label_time[0].tobytes() == clean.label_time[0].tobytes()
    assert res.costs[0].tobytes() == clean.costs[0].tobytes()


def check_strides(run):
    """6. labels wider than max S and max_input_length wider than max T: the same values, 0 / -1 in the padding."""
    rng = np.random.default_rng(8)
    acts, labels, T, S = ragged(rng, [(9, 4), (14, 6), (5, 0)], 8, label_width=11)
    res, _ = check_all(run, acts, labels, T, S)
    assert res.emit.shape == (3, 14) and res.label_time.shape == (3, 11)
    tight = run(acts, np.ascontiguousarray(labels[:, :6]), T, S)
    assert tight.label_time.shape == (3, 6)
    assert np.array_equal(res.label_time[:, :6], tight.label_time) and np.all(res.label_time[:, 6:] == -1.0)
    assert np.array_equal(res.blank, tight.blank) and np.array_equal(res.label, tight.label)
    assert np.array_equal(res.emit, tight.emit) and np.array_equal(res.costs, tight.costs)
    wide = run(acts, labels, T, S, max_input_length=21)
    assert wide.emit.shape == (3, 21)
    assert np.array_equal(wide.emit[:, :14], res.emit) and np.all(wide.emit[:, 14:] == 0.0)
    assert np.array_equal(wide.label_time, res.label_time) and np.array_equal(wide.blank, res.blank)


def check_boundary(run, W, V=8):
    """Width boundaries: a ragged batch whose longest S + 1 is W, T = S + 3 (boundary_problem)."""
    acts, labels, T, S = boundary_problem(W, V)
    return check_all(run, acts, labels, T, S)


def long_thin_problem():
    """Many frames per label sum: (T, S) = (300, 5) mixed with (1, 0) and (1, 1)."""
    return ragged(np.random.default_rng(17), [(300, 5), (1, 0), (1, 1)], 8)
