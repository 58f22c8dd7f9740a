"""Checks of the factorised-blank (HAT) loss and its read-outs, shared by tests/test_gpu_hat.py and
tests/test_cpu_hat.py.

Reference: the fp64 oracle applied to transformed logits. In fp64,
    a'[b]      = log sigmoid(z_b)
    a'[v != b] = log sigmoid(-z_b) + z_v - LSE_{u != b} z_u
whose rows sum to 1 in probability, so log_softmax(a') = a' and oracle_rnnt(a') gives the expected costs and
G' = dcost / da'; the expected gradient is G' chained through the transform by torch autograd on a float64 copy.
(The oracle takes float32 acts: the rounding of a' is <= 2^-24 |a'| per arc, far inside the tolerances here.)
Tolerances are the project's: costs 1e-4 max(1, |c|), gradients 1e-4 absolute (f32), plus one rounding of the output
type for bf16 / fp16 gradients (tests/test_gpu_parity.py).

Shapes: B = 3, (T, S) = (12, 5), (5, 5) [S = T], (9, 0) [S = 0] -- 26 lattice columns, one workgroup each.
"""
import itertools
import math

import numpy as np
import torch

import oracle
from _parity import COST_TOL, GRAD_TOL, assert_costs

SHAPES = [(12, 5), (5, 5), (9, 0)]
T_ = np.array([t for t, _ in SHAPES], np.int32)
S_ = np.array([s for _, s in SHAPES], np.int32)
OFF = np.concatenate([[0], np.cumsum(T_.astype(np.int64) * (S_ + 1))])
ROWS = int(OFF[-1])


def blank_positions(V):
    """0, V - 1 and an interior index (in the second 1024-element chunk of an f32 row at V = 2048)."""
    return [0, V - 1, (3 * V) // 4 - 1]


def problem(V, blank, seed=0):
    """N(0,1) logits and labels that avoid the blank index."""
    rng = np.random.default_rng(1000 * V + 7 * blank + seed)
    acts = rng.standard_normal((ROWS, V)).astype(np.float32)
    lab = rng.integers(0, V - 1, (len(SHAPES), int(S_.max()))).astype(np.int32)
    lab += (lab >= blank).astype(np.int32)
    return acts, lab


def hat_transform(z, blank):
    """a' of a float64 torch tensor [rows, V] (differentiable)."""
    V = z.shape[1]
    keep = torch.ones(V, dtype=torch.bool)
    keep[blank] = False
    zb = z[:, blank]
    lse = torch.logsumexp(z[:, keep], dim=1)
    a = torch.nn.functional.logsigmoid(-zb)[:, None] + z - lse[:, None]
    col = torch.zeros(V, dtype=torch.bool)
    col[blank] = True
    return torch.where(col[None, :], torch.nn.functional.logsigmoid(zb)[:, None], a)


_REF_CACHE = {}


def reference(acts, labels, blank, alignment=None, k=0, scale=None, key=None):
    """(costs, grads, a') of the reference for packed float32 `acts` (the values the code under test reads). Results
    are cached by `key` and never modified."""
    if key is not None and key in _REF_CACHE:
        return _REF_CACHE[key]
    z = torch.from_numpy(acts.astype(np.float64)).requires_grad_(True)
    a = hat_transform(z, blank)
    a32 = a.detach().numpy().astype(np.float32)
    c, G = oracle.oracle_rnnt(a32, labels, T_, S_, blank=blank, alignment=alignment, max_shift=k)
    if scale is not None:
        G = G * np.repeat(np.asarray(scale, np.float64), T_ * (S_ + 1))[:, None]
    a.backward(torch.from_numpy(G))
    out = (c, z.grad.numpy(), a.detach().numpy())
    for x in out:
        x.setflags(write=False)
    if key is not None:
        _REF_CACHE[key] = out
    return out


def pack_to_padded(acts, pad_T, pad_S1, fill=np.nan):
    out = np.full((len(SHAPES), pad_T, pad_S1, acts.shape[1]), fill, np.float32)
    for b, (Tb, Sb) in enumerate(SHAPES):
        out[b, :Tb, :Sb + 1] = acts[OFF[b]:OFF[b + 1]].reshape(Tb, Sb + 1, -1)
    return out


def padded_to_packed(x):
    return np.concatenate([x[b, :Tb, :Sb + 1].reshape(-1, x.shape[-1]) for b, (Tb, Sb) in enumerate(SHAPES)])


class Runner:
    """The code under test on one device: loss(...) -> (costs f64 [B], packed grads f32 [rows, V] | None, raw grads)."""

    def __init__(self, op, device):
        self.op, self.device = op, device

    def tensors(self, labels, device_lengths):
        dev = self.device
        lab = torch.from_numpy(labels).to(dev)
        T, S = torch.from_numpy(T_), torch.from_numpy(S_)
        if device_lengths:
            T, S = T.to(dev), S.to(dev)
        return lab, T, S

    def acts(self, acts, dtype=torch.float32, padded=False):
        x = pack_to_padded(acts, int(T_.max()) + 2, int(S_.max()) + 3) if padded else acts
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.device).to(dtype)

    def loss(self, acts, labels, blank, alignment=None, k=0, scale=None, dtype=torch.float32, padded=False,
             device_lengths=False, grads=True, summed=False):
        a = self.acts(acts, dtype, padded).requires_grad_(grads)
        lab, T, S = self.tensors(labels, device_lengths)
        al = None if alignment is None else torch.from_numpy(np.asarray(alignment, np.int32)).to(self.device)
        costs = self.op.monotonic_rnnt_hat_loss(a, lab, T, S, al, k, blank)
        g = raw = None
        if grads:
            if summed:
                costs.sum().backward()
            else:
                sc = torch.ones(len(SHAPES)) if scale is None else torch.as_tensor(scale, dtype=torch.float32)
                (costs * sc.to(self.device)).sum().backward()
            raw = a.grad.detach().float().cpu().numpy()
            g = padded_to_packed(raw) if padded else raw
        return costs.detach().cpu().numpy().astype(np.float64), g, raw

    def align(self, acts, labels, blank, alignment=None, k=0):
        lab, T, S = self.tensors(labels, False)
        al = None if alignment is None else torch.from_numpy(np.asarray(alignment, np.int32)).to(self.device)
        out, costs = self.op.monotonic_rnnt_align(self.acts(acts), lab, T, S, al, k, blank, blank_factorized=True)
        return out.cpu().numpy(), costs.cpu().numpy().astype(np.float64)


def assert_grads(g, ref, rel=0.0):
    assert g.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(g), fin)
    err = (np.abs(g[fin] - ref[fin]) - rel * np.abs(ref[fin])).max()
    print(f"    max gradient error {err:.3e}")
    assert err <= GRAD_TOL, err


def check_parity(run, V, blank, dtype=torch.float32, layouts=(False, True), lengths=(False,), rel=0.0):
    """Costs and gradients against the reference, with and without alignment= at k = 1 (the alignment from
    monotonic_rnnt_align(blank_factorized=True)), over layouts x lengths."""
    acts, labels = problem(V, blank)
    up = torch.from_numpy(acts).to(dtype).float().numpy()  # the values the code under test reads
    scale = [1.0, -0.5, 2.0]
    al, _ = run.align(up, labels, blank)
    for alignment, k in ((None, 0), (al, 1)):
        c_ref, g_ref, _ = reference(up, labels, blank, alignment, k, scale,
                                    key=("parity", V, blank, str(dtype), alignment is not None))
        for padded, dyn in itertools.product(layouts, lengths):
            c, g, _ = run.loss(up, labels, blank, alignment, k, scale, dtype, padded, dyn)
            print(f"V={V} blank={blank} {dtype} aligned={alignment is not None} padded={padded} device_lengths={dyn}: "
                  f"max cost error {np.abs(c - c_ref).max():.3e}")
            assert_costs(c, c_ref)
            assert_grads(g, g_ref, rel)


def check_blank_logit(run, V, blank, zb):
    """z_b = zb on every row over N(0,1) labels: plain tolerances."""
    acts, labels = problem(V, blank, seed=1)
    acts[:, blank] = zb
    c_ref, g_ref, _ = reference(acts, labels, blank, key=("zb", V, blank, zb))
    c, g, _ = run.loss(acts, labels, blank)
    print(f"z_b={zb}: costs {c} ref {c_ref}")
    assert_costs(c, c_ref)
    assert_grads(g, g_ref)


def check_label_shift(run, V, blank):
    """Adding 1000 to every non-blank logit leaves the costs within tolerance. (The unshifted logits are the
    shifted float32 values minus 1000, which is exact: the two calls see the same numbers up to the shift.)"""
    acts, labels = problem(V, blank, seed=2)
    shifted = (acts + np.float32(1000.0)).astype(np.float32)
    shifted[:, blank] = acts[:, blank]
    base = (shifted - np.float32(1000.0)).astype(np.float32)
    base[:, blank] = acts[:, blank]
    c0, _, _ = run.loss(base, labels, blank, grads=False)
    c1, _, _ = run.loss(shifted, labels, blank, grads=False)
    print(f"shift: {c0} {c1}")
    assert_costs(c1, c0)
    c_ref, _, _ = reference(base, labels, blank)
    assert_costs(c1, c_ref)


def check_closed_form(run, V, blank):
    """z_b = 0 and all other logits equal: cost = -log(C(T, S) 2^-T (V - 1)^-S)."""
    acts, labels = problem(V, blank, seed=3)
    acts[:] = 0.75
    acts[:, blank] = 0.0
    c, _, _ = run.loss(acts, labels, blank, grads=False)
    ref = np.array([-(math.log(math.comb(t, s)) - t * math.log(2.0) - s * math.log(V - 1)) for t, s in SHAPES])
    print(f"closed form: {c} ref {ref}")
    assert_costs(c, ref)


def _rows(b, s):
    """packed rows (t, s) of utterance b, every t"""
    Tb, Sb = SHAPES[b]
    return OFF[b] + np.arange(Tb) * (Sb + 1) + s


def check_non_finite(run, V, blank):
    """-inf label logit on every path / z_b = -inf where every path takes blank: +inf; NaN logit / z_b = +inf in the
    band: NaN; the other utterances bit-identical to a clean run (costs and gradients)."""
    acts, labels = problem(V, blank, seed=4)
    clean_c, clean_g, _ = run.loss(acts, labels, blank)
    assert np.all(np.isfinite(clean_c))

    def run_bad(edit, b, want):
        bad = acts.copy()
        edit(bad)
        c, g, _ = run.loss(bad, labels, blank)
        print(f"non-finite case utterance {b}: costs {c}")
        assert (np.isnan(c[b]) if want == "nan" else c[b] == np.inf), c
        for o in range(len(SHAPES)):
            if o != b:
                assert c[o].tobytes() == clean_c[o].tobytes()
                assert g[OFF[o]:OFF[o + 1]].tobytes() == clean_g[OFF[o]:OFF[o + 1]].tobytes()

    def mask_label(a):  # label 0 of utterance 0 is emitted from some row (t, 0): every path needs one of them
        a[_rows(0, 0), labels[0, 0]] = -np.inf

    def mask_blank(a):  # utterance 2 (S = 0): every path leaves row (3, 0) by blank
        a[_rows(2, 0)[3], blank] = -np.inf

    def nan_logit(a):  # row (0, 0) of utterance 0 is on every path
        a[OFF[0], (blank + 2) % V] = np.nan

    def inf_blank(a):  # utterance 1 (S = T): row (0, 0) is on every path, and no path takes its blank arc
        a[OFF[1], blank] = np.inf

    def inf_blank_taken(a):  # utterance 2 (S = 0): every path takes the blank arc of row (2, 0)
        a[_rows(2, 0)[2], blank] = np.inf

    def mask_all_labels_needed(a):  # utterance 1 (S = T): row (0, 0) must emit, and none of its labels has any mass
        zb = a[OFF[1], blank]
        a[OFF[1], :] = -np.inf
        a[OFF[1], blank] = zb

    run_bad(mask_label, 0, "inf")
    run_bad(mask_blank, 2, "inf")
    run_bad(mask_all_labels_needed, 1, "inf")
    # every label masked on rows that only ever take their blank arc (utterance 2, S = 0): nothing changes at all
    bad = acts.copy()
    zb = bad[_rows(2, 0), blank].copy()
    bad[_rows(2, 0), :] = -np.inf
    bad[_rows(2, 0), blank] = zb
    c, g, _ = run.loss(bad, labels, blank)
    assert c.tobytes() == clean_c.tobytes() and g.tobytes() == clean_g.tobytes()
    run_bad(nan_logit, 0, "nan")
    run_bad(inf_blank, 1, "nan")
    run_bad(inf_blank_taken, 2, "nan")


def check_masked_entries(run, V, blank, masked):
    """-inf on non-label, non-blank logits of every row (`masked`: indices): those entries have no mass and nothing
    else changes -- finite costs and gradients equal to the reference's, which handles -inf there (a' = -inf, G' = 0).
    Exercises the masked denominator with -inf inputs: an entry next to the blank, a whole chunk of a long row."""
    acts, labels = problem(V, blank, seed=11)
    masked = np.asarray(masked)
    free = np.setdiff1d(np.arange(V), np.append(masked, blank))
    hit = np.isin(labels, masked)
    labels = np.where(hit, free[labels % len(free)], labels).astype(np.int32)
    acts[:, masked] = -np.inf
    c_ref, g_ref, _ = reference(acts, labels, blank)
    assert np.all(np.isfinite(c_ref)) and np.all(np.isfinite(g_ref))
    c, g, _ = run.loss(acts, labels, blank)
    print(f"masked entries V={V} blank={blank}: costs {c} ref {c_ref}")
    assert_costs(c, c_ref)
    assert_grads(g, g_ref)
    assert np.all(g[:, masked] == 0.0)


MASKED_CASES = [(5, 1, [0]), (64, 62, [63]), (1024, 767, [766, 768]), (2048, 1535, list(range(1024)))]


def brute_best_path(a, labels, b, blank):
    """(best log-prob, alignment row) over all monotonic paths of utterance b under per-row log-probs a [rows, V]."""
    Tb, Sb = SHAPES[b]
    best = (-np.inf, None)
    for frames in itertools.combinations(range(Tb), Sb):
        s, tot, row = 0, 0.0, []
        for t in range(Tb):
            r = OFF[b] + t * (Sb + 1) + s
            if s < Sb and t == frames[s]:
                tot += a[r, labels[b, s]]
                row.append(labels[b, s])
                s += 1
            else:
                tot += a[r, blank]
                row.append(blank)
        if tot > best[0]:
            best = (tot, row)
    return best


def check_align(run, V, blank):
    """monotonic_rnnt_align(blank_factorized=True): path and cost equal the brute-force best path over a' (every
    utterance of the batch: T = 5, and T = 9 / 12 whose 1 / 792 paths are as cheap to enumerate)."""
    acts, labels = problem(V, blank, seed=5)
    _, _, a = reference(acts, labels, blank)
    out, costs = run.align(acts, labels, blank)
    for b, (Tb, Sb) in enumerate(SHAPES):
        lp, row = brute_best_path(a, labels, b, blank)
        assert abs(costs[b] + lp) <= COST_TOL * max(1.0, abs(lp)), (b, costs[b], lp)
        assert list(out[b, :Tb]) == row, (b, out[b], row)
        assert np.all(out[b, Tb:] == blank)


def check_posteriors(run_post, V, blank):
    """monotonic_rnnt_posteriors(blank_factorized=True) against the arc posteriors in the oracle's state on a':
    occupancy x softmax(a') minus G' on the blank / label column; per-frame sums are 1."""
    acts, labels = problem(V, blank, seed=6)
    _, _, a = reference(acts, labels, blank)
    a32 = a.astype(np.float32)
    c, G, den, alpha, beta = oracle.oracle_rnnt(a32, labels, T_, S_, blank=blank, debug=True)
    res = run_post(acts, labels, blank)
    bp_ref, ep_ref = np.zeros(ROWS), np.zeros(ROWS)
    for b, (Tb, Sb) in enumerate(SHAPES):
        W = Sb + 1
        for t in range(Tb):
            for s in range(max(0, t - (Tb - Sb)), min(t, Sb) + 1):
                r = OFF[b] + t * W + s
                ap = (0.0 if s == 0 else -np.inf) if t == 0 else alpha[r - W]
                occ = np.exp(ap + beta[r] + c[b])  # c = -ll
                soft = np.exp(a32[r].astype(np.float64) + den[r])
                bp_ref[r] = occ * soft[blank] - G[r, blank]
                if s < Sb:
                    ep_ref[r] = occ * soft[labels[b, s]] - G[r, labels[b, s]]
    bp, ep = res.blank.reshape(-1).astype(np.float64), res.label.reshape(-1).astype(np.float64)
    print(f"posteriors: max error blank {np.abs(bp - bp_ref).max():.3e} label {np.abs(ep - ep_ref).max():.3e}")
    assert np.abs(bp - bp_ref).max() <= GRAD_TOL and np.abs(ep - ep_ref).max() <= GRAD_TOL
    assert_costs(res.costs.astype(np.float64), c)
    for b, (Tb, Sb) in enumerate(SHAPES):
        frame = (bp + ep)[OFF[b]:OFF[b + 1]].reshape(Tb, Sb + 1).sum(axis=1)
        n_band = min(Sb, Tb - Sb) + 1
        assert np.abs(frame - 1.0).max() <= 2 * n_band * GRAD_TOL, (b, frame)  # (the posterior tests' bound)


def check_sample(run_sample, V, blank, K=5):
    """monotonic_rnnt_sample(blank_factorized=True): path_costs equal the sum of a' along each drawn path."""
    acts, labels = problem(V, blank, seed=7)
    _, _, a = reference(acts, labels, blank)
    res = run_sample(acts, labels, blank, K)
    al, pc = res.alignments, res.path_costs.astype(np.float64)
    for b, (Tb, Sb) in enumerate(SHAPES):
        for k in range(K):
            s, tot = 0, 0.0
            for t in range(Tb):
                r = OFF[b] + t * (Sb + 1) + s
                v = int(al[b, k, t])
                if v == blank:
                    tot += a[r, blank]
                else:
                    assert s < Sb and v == labels[b, s], (b, k, t)
                    tot += a[r, v]
                    s += 1
            assert s == Sb
            assert abs(pc[b, k] + tot) <= COST_TOL * max(1.0, abs(tot)), (b, k, pc[b, k], tot)
