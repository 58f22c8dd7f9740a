"""Checks of monotonic_rnnt_align shared by tests/test_cpu_align.py and tests/test_gpu_align.py (only the device
differs): a numpy fp64 Viterbi yardstick over log_softmax of the acts upcast to fp64, with the library's tie rule
(label arc only when strictly greater), and the property checks built on it and on the CPU oracle.

`run(acts, labels, T, S, alignment=None, k=0, max_input_length=None)` -> (alignment int32 [B, L], costs fp32 [B]) as
numpy arrays; acts / labels / T / S / alignment are numpy arrays.
"""
import itertools

import numpy as np

import oracle
from _parity import assert_costs

BLANK = 0


def run_cpu(acts, labels, T, S, alignment=None, k=0, max_input_length=None):
    """`run` on the host implementation (CPU tensors)."""
    import torch

    import monotonic_rnnt_op as op
    al, costs = op.monotonic_rnnt_align(
        torch.from_numpy(acts), torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S),
        alignment=None if alignment is None else torch.from_numpy(alignment), max_distance_from_alignment=k,
        blank_label=BLANK, max_input_length=max_input_length)
    assert al.dtype == torch.int32 and costs.dtype == torch.float32 and not al.requires_grad
    return al.numpy(), costs.numpy()


def offsets(T, S):
    return np.concatenate([[0], np.cumsum(np.asarray(T, np.int64) * (np.asarray(S, np.int64) + 1))])


def band_of(al_row, T, k, blank=BLANK):
    """The reference's band (restrict_to_alignment): m(t) = labels among the first t frames, s_index_mapping at
    t+1-k / t+1+k, indices clamped to [0, T]."""
    m = np.concatenate([[0], np.cumsum(np.asarray(al_row[:T]) != blank)])
    t = np.arange(T)
    return m[np.clip(t + 1 - k, 0, T)], m[np.clip(t + 1 + k, 0, T)]


def np_viterbi(acts, labels, T, S, blank=BLANK, bands=None):
    """fp64 Viterbi per utterance, vectorised over s. Returns (costs [B] fp64, paths: list of int arrays [T_b] in the
    alignment format, or None where no finite path exists)."""
    off = offsets(T, S)
    costs, paths = np.zeros(len(T)), []
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        Tb, Sb = int(Tb), int(Sb)
        W = Sb + 1
        z = np.asarray(acts[off[b]:off[b + 1]], np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            mx = z.max(axis=1)
            den = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
            lab = np.concatenate([np.asarray(labels[b, :Sb], np.int64), [blank]])  # (column S: unused filler)
            r = np.arange(Tb * W)
            lpb = (z[:, blank] - den).reshape(Tb, W)
            lpe = (z[r, np.tile(lab, Tb)] - den).reshape(Tb, W)
        v = np.full(W, -np.inf)
        v[0] = 0.0
        took = np.zeros((Tb, W), bool)
        s = np.arange(W)
        for t in range(Tb):
            lo, hi = max(0, t - (Tb - 1 - Sb)), min(Sb, t + 1)
            if bands is not None:
                lo, hi = max(lo, int(bands[b][0][t])), min(hi, int(bands[b][1][t]))
            with np.errstate(invalid="ignore"):
                x = v + lpb[t]
                y = np.concatenate([[-np.inf], v[:-1] + lpe[t, :-1]])  # the frame-t label arc from row (t, s-1)
                take = (y > x) | np.isnan(y)
            nv = np.where(take, y, x)
            inb = (s >= lo) & (s <= hi)
            v = np.where(inb, nv, -np.inf)
            took[t] = take & inb
        costs[b] = -v[Sb]
        if not np.isfinite(v[Sb]):
            paths.append(None)
            continue
        path, sc = np.zeros(Tb, np.int32), Sb
        for t in range(Tb - 1, -1, -1):
            if sc > 0 and took[t, sc]:
                path[t] = labels[b, sc - 1]
                sc -= 1
            else:
                path[t] = blank
        paths.append(path)
    return costs, paths


def ragged(rng, shapes, V, label_width=None):
    T = np.array([t for t, _ in shapes], np.int32)
    S = np.array([s for _, s in shapes], np.int32)
    acts = rng.standard_normal((int(offsets(T, S)[-1]), V)).astype(np.float32)
    labels = rng.integers(1, V, (len(T), label_width or max(1, int(S.max())))).astype(np.int32)
    return acts, labels, T, S


def check_valid(al, labels, T, S, blank=BLANK):
    """1. Validity: the non-blank entries of row b before T_b are labels[b, :S_b] in order; blank from T_b on."""
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        row = al[b, :Tb]
        assert np.array_equal(row[row != blank], labels[b, :Sb]), (b, row, labels[b, :Sb])
        assert np.all(al[b, Tb:] == blank), (b, al[b, Tb:])


def check_cost_is_the_paths(al, costs, acts, labels, T, S):
    """2. The returned cost is the oracle's cost of the returned path alone (k = 0 leaves exactly that path)."""
    ref, _ = oracle.oracle_rnnt(acts, labels, T, S, alignment=al, max_shift=0, grads=False)
    assert_costs(costs, ref)


def check_all(run, acts, labels, T, S, **kw):
    al, costs = run(acts, labels, T, S, **kw)
    check_valid(al, labels, T, S)
    check_cost_is_the_paths(al, costs, acts, labels, T, S)
    return al, costs


def check_optimal_tiny(run):
    """3. Optimality against the reference-shaped oracle alone: the minimum of its k = 0 cost over every one of the
    C(T, S) alignments is the returned cost, and its unrestricted cost is no larger."""
    rng = np.random.default_rng(3)
    shapes = [(1, 0), (1, 1), (5, 2), (6, 6), (7, 0), (9, 4)]
    acts, labels, T, S = ragged(rng, shapes, 6)
    al, costs = check_all(run, acts, labels, T, S)
    every = []
    for b, (Tb, Sb) in enumerate(shapes):
        rows = []
        for frames in itertools.combinations(range(Tb), Sb):
            row = np.full(int(T.max()), BLANK, np.int32)
            row[list(frames)] = labels[b, :Sb]
            rows.append(row)
        every.append(rows)
    n = max(len(r) for r in every)
    assert n <= 126
    best = np.full(len(shapes), np.inf)
    for i in range(n):  # call i prices alignment i (mod its count) of every utterance
        cand = np.stack([rows[i % len(rows)] for rows in every])
        c, _ = oracle.oracle_rnnt(acts, labels, T, S, alignment=cand, max_shift=0, grads=False)
        best = np.minimum(best, c)
    assert_costs(costs, best)
    full, _ = oracle.oracle_rnnt(acts, labels, T, S, grads=False)
    assert np.all(full <= costs.astype(np.float64) + 1e-4 * np.maximum(1.0, np.abs(full))), (full, costs)


def boundary_problem(W, V=8, seed=4):
    """4. A ragged batch whose longest S + 1 is W, T = S + 3, with shorter utterances mixed in (S = 0 and S = T)."""
    S0 = W - 1
    shapes = [(S0 + 3, S0), (5, 0), (7, 7), (S0 // 2 + 3, S0 // 2), (S0 + 3, max(1, S0 - 1))]
    return ragged(np.random.default_rng(seed + W), shapes, V)


def check_boundary(run, W, V=8):
    acts, labels, T, S = boundary_problem(W, V)
    al, costs = run(acts, labels, T, S)
    check_valid(al, labels, T, S)
    ref, _ = np_viterbi(acts, labels, T, S)
    assert_costs(costs, ref)  # |dc| <= COST_TOL * max(1, |c|), both sides: compare costs, not paths
    return al, costs


def planted_problem(T1, S1, V=8, seed=5):
    """5. One utterance with a random valid alignment planted: +12 on the planted symbol's logit at each of its T
    cells, row (t, s_before), column label or blank."""
    rng = np.random.default_rng(seed + S1)
    acts, labels, T, S = ragged(rng, [(T1, S1)], V)
    frames = np.sort(rng.choice(T1, S1, replace=False))
    al = np.full((1, T1), BLANK, np.int32)
    al[0, frames] = labels[0, :S1]
    s = 0
    for t in range(T1):
        acts[t * (S1 + 1) + s, al[0, t]] += 12.0
        s += int(al[0, t] != BLANK)
    return acts, labels, T, S, al


def check_exact_path(run, T1, S1):
    acts, labels, T, S, planted = planted_problem(T1, S1)
    _, paths = np_viterbi(acts, labels, T, S)
    assert np.array_equal(paths[0], planted[0])  # the yardstick recovers the planted path ...
    al, costs = run(acts, labels, T, S)
    assert np.array_equal(al, planted)           # ... and the library returns it element for element
    return al, costs


def check_restriction(run):
    """6. A restricting alignment with k in {0, 1, 3}; k >= T; an alignment with the wrong number of labels."""
    rng = np.random.default_rng(6)
    shapes = [(23, 9), (17, 17), (12, 0), (30, 4)]
    acts, labels, T, S = ragged(rng, shapes, 8)
    given = np.full((len(shapes), int(T.max())), BLANK, np.int32)
    for b, (Tb, Sb) in enumerate(shapes):
        given[b, np.sort(rng.choice(Tb, Sb, replace=False))] = labels[b, :Sb]
    free_al, free_c = run(acts, labels, T, S)
    for k in (0, 1, 3):
        al, costs = check_all(run, acts, labels, T, S, alignment=given, k=k)
        bands = [band_of(given[b], int(T[b]), k) for b in range(len(T))]
        for b, Tb in enumerate(T):
            after = np.cumsum(al[b, :Tb] != BLANK)  # label position after frame t
            assert np.all(after >= bands[b][0]) and np.all(after <= bands[b][1]), (k, b)
        ref, _ = np_viterbi(acts, labels, T, S, bands=bands)
        assert_costs(costs, ref)
        if k == 0:
            assert np.array_equal(al, given)
    al, costs = run(acts, labels, T, S, alignment=given, k=int(T.max()))
    assert np.array_equal(al, free_al) and np.array_equal(costs, free_c)
    wrong = given.copy()
    wrong[0, np.flatnonzero(wrong[0] != BLANK)[0]] = BLANK  # utterance 0: one label short
    al, costs = run(acts, labels, T, S, alignment=wrong, k=0)
    assert costs[0] == np.inf and np.all(al[0] == -1)
    assert np.array_equal(al[1:], given[1:]) and np.all(np.isfinite(costs[1:]))


def check_value_domain(run):
    """7. -inf and NaN logits: +inf / NaN costs and -1 rows for their utterances, the clean one bit-identical."""
    rng = np.random.default_rng(7)
    acts, labels, T, S = ragged(rng, [(11, 4), (9, 3), (8, 2)], 8)
    off = offsets(T, S)
    al0, c0 = run(acts, labels, T, S)
    bad = acts.copy()
    rows1 = off[1] + np.arange(int(T[1])) * (int(S[1]) + 1)  # rows (t, 0) of utterance 1: where label 0 is emitted
    bad[rows1, labels[1, 0]] = -np.inf
    bad[off[2], 3] = np.nan                                   # row (0, 0) of utterance 2: in every band
    al, costs = run(bad, labels, T, S)
    assert costs[1] == np.inf and np.all(al[1] == -1)
    assert np.isnan(costs[2]) and np.all(al[2] == -1)
    assert np.array_equal(al[0], al0[0]) and costs[0].tobytes() == c0[0].tobytes()


def check_strides(run):
    """8. labels wider than S_max and an output wider than T_max: same result, blank padding columns."""
    rng = np.random.default_rng(8)
    acts, labels, T, S = ragged(rng, [(9, 4), (14, 6), (5, 0)], 8, label_width=11)
    al, costs = check_all(run, acts, labels, T, S)
    assert al.shape == (3, 14)
    tight_al, tight_c = run(acts, np.ascontiguousarray(labels[:, :6]), T, S)
    assert np.array_equal(al, tight_al) and np.array_equal(costs, tight_c)
    wide_al, wide_c = run(acts, labels, T, S, max_input_length=21)
    assert wide_al.shape == (3, 21)
    assert np.array_equal(wide_al[:, :14], al) and np.all(wide_al[:, 14:] == BLANK) and np.array_equal(wide_c, costs)
