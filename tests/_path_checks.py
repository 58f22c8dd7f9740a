"""Checks of monotonic_rnnt_path_loss shared by tests/test_cpu_path_loss.py and tests/test_gpu_path_loss.py (only the
device differs).

`run(acts, labels, T, S, al, w=None, **kw)` -> (path_costs fp32 [B, K], grads fp32 in the shape of acts) as numpy
arrays: path_loss of the alignment rows al [B, K, L], then backward with the upstream gradient w [B, K] (None: ones).

Yardstick (independent of the library): torch on the CPU in float64. lsm = log_softmax(acts.double()); a path's cost is
a gather of lsm along the walk, written here in numpy; gradients are torch.autograd's of sum_{valid} w * cost. For
bf16 / fp16 the yardstick runs on the upcast values the kernel reads.

Tolerances are the project's (tests/_parity.py): costs assert_costs (1e-4); gradients GRAD_TOL absolute, scaled per
utterance by max(1, sum_k |w[b, k]|) -- a row's coefficients are sums of up to K weights, not probabilities <= 1 --
plus, for a reduced-precision output, one rounding of that type (2^-8 bf16, 2^-11 fp16) relative to the value. Logits
are N(0, 1): no value-domain term.
"""
import numpy as np
import torch

import _align_checks as A
import _sample_checks as SC
from _align_checks import BLANK, offsets, ragged  # noqa: F401  (re-exported)
from _parity import GRAD_TOL, assert_costs

ULP = 2.0 ** -22  # "within one fp32 ulp": relative


def walk(row, lab, Tb, Sb, blank=BLANK):
    """(lattice rows, columns) of the arcs of alignment row `row`, or None when it is no path of the utterance."""
    s, rows, cols = 0, [], []
    for t in range(Tb):
        v = int(row[t])
        if v == blank:
            rows.append(t * (Sb + 1) + s)
            cols.append(blank)
        elif v >= 0 and s < Sb and v == int(lab[s]):
            rows.append(t * (Sb + 1) + s)
            cols.append(v)
            s += 1
        else:
            return None
    return (rows, cols) if s == Sb else None


def yardstick(acts, labels, T, S, al, w=None):
    """costs fp64 [B, K] (+inf: invalid row), grads fp64 [N, V], visited bool [N] (rows some valid path stands on),
    wsum [N] (sum_k |w| of the row's utterance over its valid paths)."""
    B, K = al.shape[:2]
    w = np.ones((B, K)) if w is None else np.asarray(w, np.float64)
    a = torch.tensor(np.asarray(acts, np.float64), requires_grad=True)
    lsm = torch.log_softmax(a, dim=1)
    off = offsets(T, S)
    costs = np.full((B, K), np.inf)
    visited = np.zeros(len(acts), bool)
    wsum = np.zeros(len(acts))
    total = None
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        for k in range(K):
            arcs = walk(al[b, k], labels[b], Tb, Sb)
            if arcs is None:
                continue
            rows = torch.tensor(arcs[0], dtype=torch.int64) + int(off[b])
            c = -lsm[rows, torch.tensor(arcs[1], dtype=torch.int64)].sum()
            costs[b, k] = float(c.detach())
            visited[rows.numpy()] = True
            wsum[off[b]:off[b + 1]] += abs(w[b, k])
            term = c * float(w[b, k])
            total = term if total is None else total + term
    if total is None:
        return costs, np.zeros(a.shape), visited, wsum
    total.backward()
    return costs, a.grad.numpy(), visited, wsum


def assert_path_grads(g, ref, wsum, eps=0.0):
    """|g - ref| - eps |ref| <= GRAD_TOL max(1, wsum) on every row; non-finite in the same places."""
    g = np.asarray(g, np.float64)
    assert g.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(g), fin), np.argwhere(np.isfinite(g) != fin)[:5]
    err = np.where(fin, np.abs(np.where(fin, g, 0.0) - np.where(fin, ref, 0.0)) - eps * np.abs(np.where(fin, ref, 0.0)), 0.0)
    tol = GRAD_TOL * np.maximum(1.0, wsum)[:, None]
    print("path grads: max err / tol =", float((err / tol).max()) if err.size else 0.0)
    assert np.all(err <= tol), float((err / tol).max())


def extreme_paths(labels, T, S, L):
    """[B, 2, L]: all labels first, all labels last."""
    out = np.full((len(T), 2, L), BLANK, np.int32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, 0, :Sb] = labels[b, :Sb]
        out[b, 1, Tb - Sb:Tb] = labels[b, :Sb]
    return out


def make_paths(acts, labels, T, S, K, seed=11):
    """[B, K, max T] valid paths: the Viterbi path, the two extreme paths, then sampled paths (the host implementation's
    monotonic_rnnt_align / monotonic_rnnt_sample, fixed seed)."""
    L = int(T.max())
    parts = [A.run_cpu(acts, labels, T, S)[0][:, None, :], extreme_paths(labels, T, S, L)]
    if K > 3:
        parts.append(SC.run_cpu(acts, labels, T, S, K - 3, seed).alignments)
    al = np.ascontiguousarray(np.concatenate(parts, axis=1)[:, :K])
    assert al.shape == (len(T), K, L) and np.all(al >= 0)
    return al


def check_against_yardstick(run, acts, labels, T, S, al, w, eps=0.0, yard_acts=None, **kw):
    """Costs and gradients against the yardstick; every row no valid path visits is exactly 0."""
    costs, g = run(acts, labels, T, S, al, w, **kw)
    ref_c, ref_g, visited, wsum = yardstick(acts if yard_acts is None else yard_acts, labels, T, S, al, w)
    assert costs.dtype == np.float32 and costs.shape == al.shape[:2]
    assert_costs(costs, ref_c)
    assert_path_grads(g, ref_g, wsum, eps)
    assert np.all(g[~visited] == 0.0)
    return costs, g


# 1. shapes at the edges: (name, V, [(T, S)], K). T in {1, 63, 64, 65, 130} crosses the 64-frame blocks; S in {0, 1, T};
# S + 1 = 300 crosses the gradient kernel's 256-row segment; V = 5 takes the scalar path; the larger V with T <= 40.
EDGE_CASES = [
    ("scalar_v5_k3", 5, [(1, 1), (63, 0), (64, 64), (65, 1)], 3),
    ("v32_k64", 32, [(130, 130), (1, 0), (64, 1), (130, 40)], 64),
    ("segment_v8_k65", 8, [(301, 299), (5, 2), (65, 65), (63, 1)], 65),
    ("v400_k1", 400, [(40, 12), (17, 0), (9, 9), (33, 5)], 1),
    ("v1024_k3", 1024, [(40, 12), (20, 3), (1, 0), (12, 12)], 3),
]


def edge_problem(name):
    i = [c[0] for c in EDGE_CASES].index(name)
    _, V, shapes, K = EDGE_CASES[i]
    rng = np.random.default_rng(100 + i)
    acts, labels, T, S = ragged(rng, shapes, V)
    al = make_paths(acts, labels, T, S, K)
    w = rng.standard_normal((len(T), K)).astype(np.float32)  # signed
    return acts, labels, T, S, al, w


def check_edge_case(run, name, **kw):
    return check_against_yardstick(run, *edge_problem(name), **kw)


def small_problem(seed=21, K=6, V=12, shapes=((23, 9), (17, 17), (12, 0), (30, 4))):
    rng = np.random.default_rng(seed)
    acts, labels, T, S = ragged(rng, list(shapes), V)
    al = make_paths(acts, labels, T, S, K)
    w = rng.standard_normal((len(T), K)).astype(np.float32)
    return acts, labels, T, S, al, w


def check_signed_weights(run):
    """2. Cancellation, K identical paths, all-zero weights over a NaN logit."""
    rng = np.random.default_rng(22)
    acts, labels, T, S = ragged(rng, [(6, 2)], 7)
    ex = extreme_paths(labels, T, S, 6)  # labels first | labels last: they leave row (0, 0) by different arcs
    w = np.array([[1.0, -1.0]], np.float32)
    costs, g = check_against_yardstick(run, acts, labels, T, S, ex, w)
    want = np.zeros(7, np.float32)  # Wb = -1, We = +1, Wocc = 0: Wb (onehot_label - onehot_blank), exactly
    want[labels[0, 0]] = -1.0
    want[BLANK] = 1.0
    assert np.array_equal(g[0], want), g[0]
    # K identical paths: K times one path's gradient
    K = 5
    one_c, one_g = run(acts, labels, T, S, ex[:, :1], None)
    rep_c, rep_g = run(acts, labels, T, S, np.ascontiguousarray(np.repeat(ex[:, :1], K, axis=1)), None)
    assert np.all(rep_c == one_c[:, :1])
    assert np.abs(rep_g.astype(np.float64) - K * one_g.astype(np.float64)).max() <= GRAD_TOL * K
    # w = 0 for every path: all-zero grads, even with a NaN logit in a visited row
    bad = acts.copy()
    bad[0, 3] = np.nan
    c0, g0 = run(bad, labels, T, S, ex, np.zeros((1, 2), np.float32))
    assert np.all(np.isnan(c0)) and np.all(g0 == 0.0)


def invalid_rows(al, labels, T, S, b, k):
    """Four ways to spoil row (b, k) of an utterance with 0 < S_b < T_b: name -> row."""
    Tb, Sb = int(T[b]), int(S[b])
    base = al[b, k].copy()
    out = {"minus_one": np.full_like(base, -1)}
    r = base.copy()
    t = np.flatnonzero(r[:Tb] != BLANK)[0]
    r[t] = int(labels[b, 0]) + 1  # the first label replaced by another value (not blank)
    out["wrong_label"] = r
    r = base.copy()
    r[np.flatnonzero(r[:Tb] != BLANK)[-1]] = BLANK
    out["one_label_short"] = r
    r = base.copy()
    r[np.flatnonzero(r[:Tb] == BLANK)[-1]] = labels[b, Sb - 1]
    out["one_label_more"] = r
    return out


def check_invalid_rows(run):
    """3. An invalid row costs +inf, contributes nothing and leaves the other paths bit-identical to a call without it;
    an utterance with only invalid rows has all-zero grads."""
    acts, labels, T, S, al, w = small_problem()
    off = offsets(T, S)
    K = al.shape[1]
    keep = [k for k in range(K) if k != 2]
    ref_c, ref_g = run(acts, labels, T, S, np.ascontiguousarray(al[:, keep]), np.ascontiguousarray(w[:, keep]))
    for name, row in invalid_rows(al, labels, T, S, 0, 2).items():
        assert walk(row, labels[0], int(T[0]), int(S[0])) is None, name
        bad = al.copy()
        bad[0, 2] = row
        bad[1, 2] = -1                       # T = S: the all -1 row
        for b in (2, 3):
            bad[b, 2] = -1
        c, g = run(acts, labels, T, S, bad, w)
        assert np.all(c[:, 2] == np.inf), name
        assert c[:, keep].tobytes() == ref_c.tobytes(), name
        assert g.tobytes() == ref_g.tobytes(), name
        check_against_yardstick(run, acts, labels, T, S, bad, w)
    only = al.copy()
    only[1] = -1                             # utterance 1 (T = S): nothing but invalid rows
    only[2, :, 0] = labels[2, 0]             # utterance 2 (S = 0): a label where none fits
    c, g = check_against_yardstick(run, acts, labels, T, S, only, w)
    assert np.all(c[1] == np.inf) and np.all(c[2] == np.inf)
    assert np.all(g[off[1]:off[3]] == 0.0)


def pack_to_padded(acts, T, S, pad_T, pad_S1, fill):
    out = np.full((len(T), pad_T, pad_S1, acts.shape[1]), fill, np.float32)
    off = offsets(T, S)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    return out


def padded_to_packed(x, T, S):
    return np.concatenate([x[b, : T[b], : S[b] + 1].reshape(-1, x.shape[-1]) for b in range(len(T))])


def check_padded(run, V=12):
    """4. The padded layout (NaN in its padding rows) equals the packed result bit for bit; padding rows are 0."""
    acts, labels, T, S, al, w = small_problem(seed=23, V=V)
    c, g = run(acts, labels, T, S, al, w)
    pad_T, pad_S1 = int(T.max()) + 2, int(S.max()) + 3
    cp, gp = run(pack_to_padded(acts, T, S, pad_T, pad_S1, np.nan), labels, T, S, al, w)
    assert gp.shape == (len(T), pad_T, pad_S1, V)
    assert cp.tobytes() == c.tobytes()
    assert padded_to_packed(gp, T, S).tobytes() == g.tobytes()
    mask = np.ones(gp.shape[:3], bool)
    for b in range(len(T)):
        mask[b, : T[b], : S[b] + 1] = False
    assert np.all(gp[mask] == 0.0)


def check_consistency(run, run_align, run_sample, run_loss_grad):
    """5. path_loss(align) is align's cost and the k = 0 restricted loss's gradient; path_loss(sample) is the sample's
    path costs. run_align -> (al [B, L], costs); run_sample(K, seed) -> Samples; run_loss_grad(al) -> grads of
    monotonic_rnnt_loss(alignment=al, max_distance_from_alignment=0).sum()."""
    acts, labels, T, S, _, _ = small_problem(seed=24)
    al, c = run_align(acts, labels, T, S)
    pc, g = run(acts, labels, T, S, np.ascontiguousarray(al[:, None, :]), None)
    assert np.all(np.abs(pc[:, 0].astype(np.float64) - c) <= ULP * np.abs(c)), (pc[:, 0], c)
    gl = run_loss_grad(acts, labels, T, S, al)
    assert np.abs(g.astype(np.float64) - gl).max() <= GRAD_TOL
    smp = run_sample(acts, labels, T, S, 9, 5)
    pc, _ = run(acts, labels, T, S, smp.alignments, None)
    assert np.all(np.abs(pc.astype(np.float64) - smp.path_costs) <= ULP * np.abs(smp.path_costs))


def check_non_finite(run):
    """6. A -inf masked label on one path: +inf for that path only. A NaN logit in a visited row: NaN for the visiting
    paths and in that row's gradient. Everything else bit-identical to the clean call."""
    acts, labels, T, S, al, w = small_problem(seed=25)
    off = offsets(T, S)
    ex = extreme_paths(labels, T, S, al.shape[2])
    al[:, 1:3] = ex                                  # k = 1: labels first, k = 2: labels last
    c0, g0 = run(acts, labels, T, S, al, w)
    bad = acts.copy()
    first = [k for k in range(al.shape[1]) if al[0, k, 0] != BLANK]      # paths that emit label 0 at frame 0
    rest = [k for k in range(al.shape[1]) if k not in first]
    assert 1 in first and 2 in rest
    bad[off[0], labels[0, 0]] = -np.inf              # row (0, 0) of utterance 0: its label arc is masked
    t3 = int(T[3]) - int(S[3])                       # row (T - S, 0) of utterance 3: "labels last" stands there
    row3 = off[3] + t3 * (int(S[3]) + 1)
    visits = [k for k in range(al.shape[1]) if not np.any(al[3, k, :t3] != BLANK)]
    assert 2 in visits and 1 not in visits
    bad[row3, 4] = np.nan
    c, g = run(bad, labels, T, S, al, w)
    assert np.all(c[0, first] == np.inf) and np.all(np.isfinite(c[0, rest]))  # (rest: row (0, 0)'s den changed)
    assert np.all(np.isnan(c[3, visits]))
    others = [k for k in range(al.shape[1]) if k not in visits]
    assert c[3, others].tobytes() == c0[3, others].tobytes()
    assert c[1:3].tobytes() == c0[1:3].tobytes()
    assert np.all(np.isnan(g[row3])) and np.all(np.isfinite(np.delete(g, row3, axis=0)))
    same = np.ones(len(acts), bool)
    same[off[0]] = same[row3] = False                # the two touched rows; (0, 0)'s softmax changed with its logit
    assert g[same].tobytes() == g0[same].tobytes()
    check_against_yardstick(run, bad, labels, T, S, al, w)


def check_reproducible(run):
    """7. Two runs are bitwise equal."""
    acts, labels, T, S, al, w = small_problem(seed=26, K=9)
    c1, g1 = run(acts, labels, T, S, al, w)
    c2, g2 = run(acts, labels, T, S, al, w)
    assert c1.tobytes() == c2.tobytes() and g1.tobytes() == g2.tobytes()
    return acts, labels, T, S, al, w, c1, g1


def run_cpu(acts, labels, T, S, al, w=None):
    """`run` on the host implementation (CPU tensors; 2-D packed or 4-D padded acts)."""
    import monotonic_rnnt_op as op
    a = torch.from_numpy(np.ascontiguousarray(acts)).requires_grad_(True)
    pc = op.monotonic_rnnt_path_loss(a, torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S),
                                     torch.from_numpy(al), blank_label=BLANK)
    assert pc.dtype == torch.float32 and tuple(pc.shape) == tuple(al.shape[:2]) and pc.requires_grad
    pc.backward(torch.ones_like(pc) if w is None else torch.from_numpy(np.asarray(w, np.float32)))
    return pc.detach().numpy(), a.grad.numpy()
