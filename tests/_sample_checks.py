"""Checks of monotonic_rnnt_sample shared by tests/test_cpu_sample.py, tests/test_gpu_sample.py and
tests/test_gpu_joint_sample.py (only the device / the source of the logits differs): a numpy Philox4x32-10, a numpy
fp64 yardstick that applies the library's decision rule to its own backward pass, and the property checks built on
them and on the CPU oracle.

`run(acts, labels, T, S, K, seed, first_sample=0, alignment=None, k=0, max_input_length=None)` ->
Samples(alignments int32 [B, K, L], path_costs fp32 [B, K], costs fp32 [B]) as numpy arrays; the inputs are numpy.

Exactness. The library and the yardstick draw the same u(b, k, t) (integer code) and compare it with p_label formed
from states that agree to GRAD_TOL (the project's tolerance on exactly these coefficients). A sample is *close* when
on the yardstick's walk some frame has |u - p_label| <= GRAD_TOL; every other sample must equal the yardstick's row
element for element, and close samples may be at most CLOSE_CAP of a case's samples (a condition on the case, met by
the yardstick alone: each frame is close with probability <= 2 GRAD_TOL, so a T <= 40 sample with probability <= 0.8 %).
"""
import collections
import itertools

import numpy as np

import oracle
from _align_checks import BLANK, band_of, boundary_problem, check_valid, offsets, ragged  # noqa: F401  (re-exported)
from _parity import GRAD_TOL, assert_costs

Samples = collections.namedtuple("Samples", ["alignments", "path_costs", "costs"])
NEG = -np.inf
CLOSE_CAP = 0.03

# counter, key -> output (Random123's known answers for philox4x32-10)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
_M32 = np.uint64(0xffffffff)


def philox4x32_10(ctr, key):
    """ctr: four arrays (broadcastable) of 32-bit words, key: two. Returns the four output words as uint64 arrays."""
    c = [np.asarray(x, np.uint64) & _M32 for x in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def check_generator():
    """1. The numpy generator reproduces the three known answers."""
    for ctr, key, want in PHILOX_KAT:
        got = philox4x32_10(ctr, key)
        assert tuple(int(x) for x in got) == want, (ctr, key, [hex(int(x)) for x in got])


def uniforms(seed, b, first, K, Tb):
    """u(b, k, t) [K, Tb]: key (seed low, seed high), counter (t >> 2, first + k, b, 0x4D524E54), word t & 3,
    u = (word + 0.5) 2^-32."""
    seed = int(seed) & ((1 << 64) - 1)
    nq = (Tb + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, :]
    smp = (np.uint64(first) + np.arange(K, dtype=np.uint64))[:, None]
    w = philox4x32_10((q, smp, np.uint64(b), np.uint64(0x4D524E54)), (seed & 0xffffffff, seed >> 32))
    words = np.stack([np.broadcast_to(x, (K, nq)) for x in w], axis=2).reshape(K, nq * 4)[:, :Tb]
    return (words.astype(np.float64) + 0.5) * 2.0 ** -32


def np_state(acts, labels, T, S, blank=BLANK, bands=None):
    """fp64 lpb / lpe [T_b, S_b + 1] (lpe -inf at s = S) and beta [T_b + 1, S_b + 1] (beta[T_b] = [s == S_b]) per
    utterance: the backward pass of _posterior_checks.np_posteriors."""
    off = offsets(T, S)
    out = []
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
            lpe[:, Sb] = NEG
            Bt = np.full((Tb + 1, W), NEG)
            Bt[Tb, Sb] = 0.0
            for t in range(Tb - 1, -1, -1):
                v = np.logaddexp(Bt[t + 1] + lpb[t], np.concatenate([Bt[t + 1, 1:], [NEG]]) + lpe[t])
                if t == 0:
                    v = np.where(s == 0, v, NEG)
                elif bands is not None:
                    v = np.where((s >= int(bands[b][0][t - 1])) & (s <= int(bands[b][1][t - 1])), v, NEG)
                Bt[t] = v
        out.append((lpb, lpe, Bt))
    return out


YardSamples = collections.namedtuple("YardSamples", ["rows", "path_costs", "close", "costs"])


def np_sample(acts, labels, T, S, K, seed, first=0, bands=None, tol=GRAD_TOL, blank=BLANK):
    """The yardstick: the library's walk and decision rule on np_state, the same Philox stream. rows[b]: int32
    [K, T_b] (None when the utterance has no finite log-likelihood), path_costs [B, K] fp64, close [B, K] (some frame
    of the walk has |u - p_label| <= tol), costs [B] fp64."""
    rows, close, pcost, costs = [], np.zeros((len(T), K), bool), np.zeros((len(T), K)), np.zeros(len(T))
    for b, (lpb, lpe, Bt) in enumerate(np_state(acts, labels, T, S, blank, bands)):
        Tb, Sb = int(T[b]), int(S[b])
        costs[b] = -Bt[0, 0]
        if not np.isfinite(Bt[0, 0]):
            rows.append(None)
            pcost[b] = np.inf if Bt[0, 0] == NEG else np.nan
            continue
        u = uniforms(seed, b, first, K, Tb)
        s = np.zeros(K, np.int64)
        out = np.full((K, Tb), blank, np.int32)
        for t in range(Tb):
            with np.errstate(invalid="ignore", over="ignore"):
                x = np.where(Tb - 1 - t >= Sb - s, lpb[t, s] + Bt[t + 1, s], NEG)
                y = np.where(s < Sb, lpe[t, s] + Bt[t + 1, np.minimum(s + 1, Sb)], NEG)
                p = np.where(y == NEG, 0.0, np.where(x == NEG, 1.0, 1.0 / (1.0 + np.exp(x - y))))
                take = (u[:, t] < p) & (s < Sb)
                close[b] |= np.abs(u[:, t] - p) <= np.broadcast_to(tol, (len(T),))[b]  # (tol: one value, or [B])
            pcost[b] -= np.where(take, lpe[t, s], lpb[t, s])
            out[take, t] = labels[b, s[take]]
            s = s + take
        rows.append(out)
    return YardSamples(rows, pcost, close, costs)


def run_cpu(acts, labels, T, S, K, seed, first_sample=0, alignment=None, k=0, max_input_length=None):
    """`run` on the host implementation (CPU tensors)."""
    import torch

    import monotonic_rnnt_op as op
    out = op.monotonic_rnnt_sample(
        torch.from_numpy(acts), torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S), K, seed,
        first_sample=first_sample, alignment=None if alignment is None else torch.from_numpy(alignment),
        max_distance_from_alignment=k, blank_label=BLANK, max_input_length=max_input_length)
    check_types(out, len(T), K)
    return Samples(*(x.numpy() for x in out))


def check_types(out, B, K):
    import torch
    assert out._fields == Samples._fields
    assert out.alignments.dtype == torch.int32 and out.path_costs.dtype == torch.float32
    assert out.costs.dtype == torch.float32 and not any(x.requires_grad for x in out)
    assert out.alignments.dim() == 3 and tuple(out.alignments.shape[:2]) == (B, K)
    assert tuple(out.path_costs.shape) == (B, K) and tuple(out.costs.shape) == (B,)


def check_valid_all(res, labels, T, S):
    for k in range(res.alignments.shape[1]):
        check_valid(res.alignments[:, k, :], labels, T, S)


def check_path_costs(res, acts, labels, T, S):
    """path_costs[b, k] is the oracle's k = 0 cost of row (b, k) alone."""
    for k in range(res.alignments.shape[1]):
        ref, _ = oracle.oracle_rnnt(acts, labels, T, S, alignment=np.ascontiguousarray(res.alignments[:, k, :]),
                                    max_shift=0, grads=False)
        assert_costs(res.path_costs[:, k], ref)


def check_validity_and_cost(run):
    """2. Every sample is a valid alignment, its path cost is the oracle's cost of that alignment, costs is the loss;
    T = S and S = 0 have a single path."""
    shapes = [(1, 0), (1, 1), (5, 2), (6, 6), (7, 0), (9, 4)]
    acts, labels, T, S = ragged(np.random.default_rng(3), shapes, 6)
    res = run(acts, labels, T, S, 5, 2024)
    assert res.alignments.shape == (len(shapes), 5, 9)
    check_valid_all(res, labels, T, S)  # (the single path of T = S / S = 0 is the only valid row)
    check_path_costs(res, acts, labels, T, S)
    full, _ = oracle.oracle_rnnt(acts, labels, T, S, grads=False)
    assert_costs(res.costs, full)
    for b, (Tb, Sb) in enumerate(shapes):
        if Sb in (0, Tb):
            want = labels[b, :Tb] if Sb else np.full(Tb, BLANK, np.int32)
            assert np.all(res.alignments[b, :, :Tb] == want[None, :]), b
            assert_costs(res.path_costs[b], np.full(5, full[b]))
    return res


def check_exact(run, acts, labels, T, S, K, seed, alignment=None, k=0, tol=GRAD_TOL, cap=CLOSE_CAP, state_acts=None,
                **kw):
    """3. Every sample that is not close equals the yardstick's row element for element; close samples are at most
    `cap` of the case. Also validity, and the band under a restricting alignment. state_acts: the logits the yardstick
    sees when they are not `acts` (the values a half-precision or fused-joint call computes on). Returns (res, share of
    close samples)."""
    res = run(acts, labels, T, S, K, seed, alignment=alignment, k=k, **kw)
    bands = None if alignment is None else [band_of(alignment[b], int(T[b]), k) for b in range(len(T))]
    ref = np_sample(acts if state_acts is None else state_acts, labels, T, S, K, seed, kw.get("first_sample", 0), bands,
                    tol)
    share = float(ref.close.mean())
    assert share <= cap, ("the case itself has too many close samples", share)
    check_valid_all(res, labels, T, S)
    for b, Tb in enumerate(T):
        Tb = int(Tb)
        assert ref.rows[b] is not None
        exact = ~ref.close[b]
        assert np.array_equal(res.alignments[b, exact, :Tb], ref.rows[b][exact]), (b, np.flatnonzero(
            np.any(res.alignments[b, :, :Tb] != ref.rows[b], axis=1) & exact)[:5])
        assert np.all(res.alignments[b, :, Tb:] == BLANK)
        assert_costs(res.path_costs[b][exact], ref.path_costs[b][exact])
        if bands is not None:
            after = np.cumsum(res.alignments[b, :, :Tb] != BLANK, axis=1)  # label position after frame t
            assert np.all(after >= bands[b][0][None, :]) and np.all(after <= bands[b][1][None, :]), (k, b)
    assert_costs(res.costs, ref.costs)
    return res, share


def random_alignment(rng, labels, T, S):
    given = np.full((len(T), int(T.max())), BLANK, np.int32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        given[b, np.sort(rng.choice(int(Tb), int(Sb), replace=False))] = labels[b, :Sb]
    return given


def check_exact_paths(run, W=33, seed=5):
    """3. boundary_problem(W): a ragged batch with longest S + 1 = W, T = S + 3 (<= 40 frames at the default), K = 64,
    free and restricted by a random alignment at k in {0, 1, 3}; k = 0 returns the given alignment for every sample.
    Observed close samples of the yardstick (seed 5; free, k = 0, 1, 3), of 320 each: W = 33: 1, 0, 1, 1; W = 96: 2, 2,
    2, 2; W = 97: 4, 2, 2, 4 -- at most 1.25 %."""
    acts, labels, T, S = boundary_problem(W)
    check_exact(run, acts, labels, T, S, 64, seed)
    given = random_alignment(np.random.default_rng(9), labels, T, S)
    for k in (0, 1, 3):
        res, _ = check_exact(run, acts, labels, T, S, 64, seed, alignment=given, k=k)
        if k == 0:
            assert np.all(res.alignments == given[:, None, :])


def bimodal_problem(T1=200, S1=100, V=6, seed=23):
    """One utterance whose posterior has two far-apart modes -- every label as early as possible, or every label as
    late as possible (+9 on those arcs' logits) -- so that samples of one call stand up to S1 label positions apart."""
    rng = np.random.default_rng(seed)
    acts, labels, T, S = ragged(rng, [(T1, S1), (3, 1)], V)
    W = S1 + 1
    for t in range(T1):
        if t < S1:
            acts[t * W + t, labels[0, t]] += 9.0       # early mode: label t at frame t
        else:
            acts[t * W + S1, BLANK] += 9.0             # ... then blanks
        if t < T1 - S1:
            acts[t * W + 0, BLANK] += 9.0              # late mode: blanks first
        else:
            s = t - (T1 - S1)
            acts[t * W + s, labels[0, s]] += 9.0       # ... then label s at frame T - S + s
    return acts, labels, T, S


def _bound(p, K, close):
    return 5.0 * np.sqrt(p * (1.0 - p) / K) + (1.0 + close) / K


def check_path_frequencies(run, seed=77, K=4096):
    """4a. (T, S) = (6, 3), V = 5: the frequency of each of the 20 paths against p(path) = exp(cost - path cost) from
    the oracle, |f - p| <= 5 sqrt(p (1 - p) / K) + (1 + close) / K."""
    acts, labels, T, S = ragged(np.random.default_rng(41), [(6, 3)], 5)
    full, _ = oracle.oracle_rnnt(acts, labels, T, S, grads=False)
    paths, probs = [], []
    for frames in itertools.combinations(range(6), 3):
        row = np.full((1, 6), BLANK, np.int32)
        row[0, list(frames)] = labels[0, :3]
        c, _ = oracle.oracle_rnnt(acts, labels, T, S, alignment=row, max_shift=0, grads=False)
        paths.append(row[0])
        probs.append(float(np.exp(full[0] - c[0])))
    assert len(paths) == 20 and abs(sum(probs) - 1.0) <= 1e-9
    res = run(acts, labels, T, S, K, seed)
    close = int(np_sample(acts, labels, T, S, K, seed).close.sum())
    check_valid_all(res, labels, T, S)
    for row, p in zip(paths, probs):
        f = float(np.mean(np.all(res.alignments[0] == row[None, :], axis=1)))
        assert abs(f - p) <= _bound(p, K, close), (row, f, p, close)


def check_arc_marginals(run, run_posteriors, seed=78, K=4096):
    """4b. (T, S) = (12, 5): the frequency of the label arc out of every lattice row against
    monotonic_rnnt_posteriors(...).label under the same bound."""
    acts, labels, T, S = ragged(np.random.default_rng(42), [(12, 5)], 6)
    post = run_posteriors(acts, labels, T, S).label.reshape(12, 6).astype(np.float64)
    res = run(acts, labels, T, S, K, seed)
    close = int(np_sample(acts, labels, T, S, K, seed).close.sum())
    emits = res.alignments[0] != BLANK                                  # [K, T]
    before = np.cumsum(emits, axis=1) - emits                          # label position before frame t
    freq = np.zeros((12, 6))
    for t in range(12):
        freq[t] = np.bincount(before[emits[:, t], t], minlength=6) / K
    err = np.abs(freq - post)
    assert np.all(err <= _bound(post, K, close)), (float(err.max()), close)


def check_determinism(run):
    """5. Bitwise repeatable; K = 8 is the first 8 of K = 64; first_sample = 8 continues; the other utterances of the
    batch do not matter, only the utterance's index; the seed does."""
    rng = np.random.default_rng(19)
    shapes = [(21, 8), (34, 13), (9, 0), (17, 17)]
    acts, labels, T, S = ragged(rng, shapes, 7)
    r64 = run(acts, labels, T, S, 64, 99)
    again = run(acts, labels, T, S, 64, 99)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r64, again))
    r8 = run(acts, labels, T, S, 8, 99)
    assert np.array_equal(r8.alignments, r64.alignments[:, :8]) and r8.path_costs.tobytes() == r64.path_costs[:, :8].tobytes()
    n8 = run(acts, labels, T, S, 8, 99, first_sample=8)
    assert np.array_equal(n8.alignments, r64.alignments[:, 8:16])
    assert n8.path_costs.tobytes() == r64.path_costs[:, 8:16].tobytes()
    # utterances 0 and 3 keep their index, 1 and 2 are replaced by other utterances
    off = offsets(T, S)
    acts2, labels2, T2, S2 = ragged(rng, [shapes[0], (11, 4), (40, 2), shapes[3]], 7)
    off2 = offsets(T2, S2)
    for b in (0, 3):
        acts2[off2[b]:off2[b + 1]] = acts[off[b]:off[b + 1]]
        labels2[b, :S[b]] = labels[b, :S[b]]
    other = run(acts2, labels2, T2, S2, 64, 99)
    for b in (0, 3):
        Tb = int(T[b])
        assert np.array_equal(other.alignments[b, :, :Tb], r64.alignments[b, :, :Tb]), b
        assert other.path_costs[b].tobytes() == r64.path_costs[b].tobytes()
    seeded = run(acts, labels, T, S, 64, 100)
    assert not np.array_equal(seeded.alignments[0], r64.alignments[0])
    assert not np.array_equal(seeded.alignments[1], r64.alignments[1])
    big = run(acts, labels, T, S, 8, 99 + (5 << 32))  # the high half of the seed is part of the key
    assert not np.array_equal(big.alignments[1], r8.alignments[1])
    return r64


def check_value_domain(run):
    """7. -inf and NaN logits: their utterances all -1 with +inf / NaN path costs, the clean one bit-identical."""
    rng = np.random.default_rng(7)
    acts, labels, T, S = ragged(rng, [(11, 4), (9, 3), (8, 2)], 8)
    off = offsets(T, S)
    clean = run(acts, labels, T, S, 5, 31)
    bad = acts.copy()
    rows1 = off[1] + np.arange(int(T[1])) * (int(S[1]) + 1)  # rows (t, 0) of utterance 1: where label 0 is emitted
    bad[rows1, labels[1, 0]] = -np.inf
    bad[off[2], 3] = np.nan                                   # row (0, 0) of utterance 2: in every band
    res = run(bad, labels, T, S, 5, 31)
    assert res.costs[1] == np.inf and np.all(res.alignments[1] == -1) and np.all(res.path_costs[1] == np.inf)
    assert np.isnan(res.costs[2]) and np.all(res.alignments[2] == -1) and np.all(np.isnan(res.path_costs[2]))
    assert np.array_equal(res.alignments[0], clean.alignments[0])
    assert res.path_costs[0].tobytes() == clean.path_costs[0].tobytes()
    assert res.costs[0].tobytes() == clean.costs[0].tobytes()


def check_strides(run):
    """7. labels wider than S_max and an output wider than T_max: the same rows plus blank padding."""
    rng = np.random.default_rng(8)
    acts, labels, T, S = ragged(rng, [(9, 4), (14, 6), (5, 0)], 8, label_width=11)
    res = run(acts, labels, T, S, 6, 55)
    assert res.alignments.shape == (3, 6, 14)
    check_valid_all(res, labels, T, S)
    tight = run(acts, np.ascontiguousarray(labels[:, :6]), T, S, 6, 55)
    assert np.array_equal(res.alignments, tight.alignments) and np.array_equal(res.path_costs, tight.path_costs)
    wide = run(acts, labels, T, S, 6, 55, max_input_length=21)
    assert wide.alignments.shape == (3, 6, 21)
    assert np.array_equal(wide.alignments[:, :, :14], res.alignments) and np.all(wide.alignments[:, :, 14:] == BLANK)
    assert np.array_equal(wide.path_costs, res.path_costs) and np.array_equal(wide.costs, res.costs)


def check_host_refusals(fn, problem, ws, tail, T_max, lib):
    """7. fn = mrnnt_sample / mrnnt_cpu_sample: a short out_stride, num_samples = 0, a sample index past 2^32 and a
    NULL output are refused with a message before anything runs (tail: the stream / thread-count argument)."""
    import ctypes

    import _mrnnt_lib as L
    vp = ctypes.c_void_p
    out = np.zeros((problem.B, 4, T_max), np.int32)
    pc = np.zeros((problem.B, 4), np.float32)

    def call(w, K, first, o, stride):
        return fn(ctypes.byref(problem), w, K, 1, first, o, stride, vp(pc.ctypes.data), tail)
    o = vp(out.ctypes.data)
    assert call(ws, 4, 0, o, T_max - 1) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignments row stride" in lib.mrnnt_last_error()
    assert call(ws, 0, 0, o, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"num_samples" in lib.mrnnt_last_error()
    assert call(ws, 4, -1, o, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"first_sample" in lib.mrnnt_last_error()
    assert call(ws, 4, (1 << 32) - 3, o, T_max) == L.RNNT_STATUS_INVALID_VALUE
    assert b"first_sample" in lib.mrnnt_last_error()
    assert call(ws, 4, 0, None, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"alignments is null" in lib.mrnnt_last_error()
    assert call(None, 4, 0, o, T_max) == L.RNNT_STATUS_INVALID_VALUE and b"workspace is null" in lib.mrnnt_last_error()
    assert np.all(out == 0) and np.all(pc == 0)
