"""Checks of the factorised-blank (HAT) path scores and expected costs, monotonic_rnnt_path_loss(blank_factorized=True)
and monotonic_rnnt_expected_cost(blank_factorized=True), shared by tests/test_cpu_hat_path_loss.py,
tests/test_cpu_hat_expect.py and their GPU twins (only the device differs).

Yardstick (independent of the library): torch on the CPU in float64. a' = _hat_checks.hat_transform(z.double(), blank)
has rows that sum to 1 in probability; a path's cost is a gather of a' along _path_checks.walk; the expected cost is
the brute-force enumeration (T <= 7) and the log-domain DP of _expect_checks restated for any blank index (and an
optional alignment band) over a' in place of log_softmax. Gradients are torch.autograd's through the transform. For
bf16 / fp16 the yardstick runs on the upcast values the kernel reads.

Tolerances are the project's own: costs _parity.assert_costs; path gradients _path_checks.assert_path_grads; the
expected value and its gradients the bounds at the head of _expect_checks.py (assert_expected, grad_tol).

Shapes: _hat_checks.SHAPES -- (12, 5), (5, 5) [S = T], (9, 0) [S = 0] -- and at V = 64 one more utterance (70, 9) whose
paths cross a 64-frame block of the walk / coefficient kernels with a non-trivial hull.
"""
import itertools
import math

import numpy as np
import torch

import _expect_checks as E
import _hat_checks as H
import _path_checks as P
from _align_checks import band_of, offsets
from _parity import COST_TOL, GRAD_TOL, assert_costs

NI = -math.inf


def shapes(V):
    return list(H.SHAPES) + ([(70, 9)] if V == 64 else [])


def problem(V, blank, seed=0, shp=None):
    """N(0, 1) logits and labels that avoid the blank index: (acts, labels, T, S)."""
    shp = shapes(V) if shp is None else list(shp)
    rng = np.random.default_rng(5000 * V + 11 * blank + seed)
    T = np.array([t for t, _ in shp], np.int32)
    S = np.array([s for _, s in shp], np.int32)
    acts = rng.standard_normal((int(offsets(T, S)[-1]), V)).astype(np.float32)
    lab = rng.integers(0, V - 1, (len(shp), max(1, int(S.max())))).astype(np.int32)
    lab += (lab >= blank).astype(np.int32)
    return acts, lab, T, S


def make_paths(labels, T, S, K, blank, seed=3):
    """[B, K, max T] valid paths, made here: a random one, labels first, labels last, then random ones."""
    rng = np.random.default_rng(seed)
    L = int(T.max())
    out = np.full((len(T), K, L), blank, np.int32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        for k in range(K):
            if k == 1:
                frames = np.arange(Sb)
            elif k == 2:
                frames = np.arange(Tb - Sb, Tb)
            else:
                frames = np.sort(rng.choice(Tb, Sb, replace=False))
            out[b, k, frames] = labels[b, :Sb]
    return out


def upcast(acts, dtype):
    return acts if dtype is None else torch.from_numpy(acts).to(dtype).float().numpy()


# ---- the code under test ---------------------------------------------------------------------------------------------

class Dev:
    """The two functions on one device, numpy in and out."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.gpu = self.device.type == "cuda"

    def t(self, x):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def lengths(self, T, S, device_lengths):
        return (self.t(T), self.t(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))

    def acts(self, acts, dtype=None, unaligned=False, grads=True):
        a = self.t(acts)
        a = a if dtype is None else a.to(dtype)
        if unaligned:  # rows that start 4 bytes past a 16-byte boundary: the scalar kernels
            n = 4 // a.element_size()
            buf = torch.empty(a.numel() + n, dtype=a.dtype, device=self.device)
            buf[n:].copy_(a.reshape(-1))
            a = buf[n:].view(a.shape)
            assert a.data_ptr() % 16 == 4 and a.is_contiguous()
        return a.requires_grad_(grads)

    def path(self, acts, labels, T, S, al, w, blank, hat=True, dtype=None, device_lengths=False, unaligned=False):
        """(path_costs fp32 [B, K], grads fp32 in the shape of acts)"""
        import monotonic_rnnt_op as op
        a = self.acts(acts, dtype, unaligned)
        Tt, St = self.lengths(T, S, device_lengths)
        kw = {"blank_factorized": True} if hat else {}
        pc = op.monotonic_rnnt_path_loss(a, self.t(labels), Tt, St, self.t(al), blank_label=blank, **kw)
        assert pc.dtype == torch.float32 and tuple(pc.shape) == tuple(al.shape[:2]) and pc.requires_grad
        pc.backward(torch.ones_like(pc) if w is None else self.t(np.asarray(w, np.float32)))
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
        return pc.detach().cpu().numpy(), a.grad.float().cpu().numpy()

    def expect(self, acts, labels, T, S, wb, we, ge, gc, blank, alignment=None, k=0, hat=True, dtype=None,
               device_lengths=False, unaligned=False):
        """(expected fp32 [B], costs fp32 [B], grads fp32 in the shape of acts)"""
        import monotonic_rnnt_op as op
        a = self.acts(acts, dtype, unaligned)
        Tt, St = self.lengths(T, S, device_lengths)
        kw = {"blank_factorized": True} if hat else {}
        e, c = op.monotonic_rnnt_expected_cost(a, self.t(labels), Tt, St, self.t(wb), self.t(we), self.t(alignment), k,
                                               blank, **kw)
        B = len(T)
        assert e.dtype == torch.float32 and c.dtype == torch.float32 and e.shape == (B,) and c.shape == (B,)
        one = np.ones(B, np.float32)
        torch.autograd.backward((e, c), (self.t(one if ge is None else np.asarray(ge, np.float32)),
                                         self.t(one if gc is None else np.asarray(gc, np.float32))))
        return e.detach().cpu().numpy(), c.detach().cpu().numpy(), a.grad.float().cpu().numpy()

    def hat_loss(self, acts, labels, T, S, gc, blank, alignment=None, k=0, dtype=None, device_lengths=False,
                 unaligned=False):
        """(costs fp32 [B], grads fp64 in the shape of acts -- 2-D packed or 4-D padded) of monotonic_rnnt_hat_loss
        with the per-utterance upstream gradient gc; gc None: the cost-only forward, (costs, None)."""
        import monotonic_rnnt_op as op
        a = self.acts(acts, dtype, unaligned, grads=gc is not None)
        Tt, St = self.lengths(T, S, device_lengths)
        c = op.monotonic_rnnt_hat_loss(a, self.t(labels), Tt, St, self.t(alignment), k, blank)
        assert c.dtype == torch.float32 and c.shape == (len(T),)
        if gc is None:
            return c.detach().cpu().numpy(), None
        c.backward(self.t(np.asarray(gc, np.float32)))
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
        return c.detach().cpu().numpy(), a.grad.float().cpu().numpy().astype(np.float64)

    def readout(self, name, acts, labels, T, S, blank, *args, **kw):
        import monotonic_rnnt_op as op
        r = getattr(op, name)(self.t(acts), self.t(labels), torch.from_numpy(T), torch.from_numpy(S), *args,
                              blank_label=blank, blank_factorized=True, **kw)
        out = [x.cpu().numpy() for x in r]
        return type(r)(*out) if hasattr(r, "_fields") else tuple(out)


# ---- yardsticks ------------------------------------------------------------------------------------------------------

def transformed(acts, blank):
    """(z float64 leaf, a' = hat_transform(z))"""
    z = torch.tensor(np.asarray(acts, np.float64), requires_grad=True)
    return z, H.hat_transform(z, blank)


def path_yardstick(acts, labels, T, S, al, w, blank):
    """costs fp64 [B, K] (+inf: invalid row), grads fp64 [N, V], visited bool [N], wsum [N] (_path_checks.yardstick
    over a')."""
    B, K = al.shape[:2]
    w = np.ones((B, K)) if w is None else np.asarray(w, np.float64)
    z, a = transformed(acts, blank)
    off = offsets(T, S)
    costs = np.full((B, K), np.inf)
    visited = np.zeros(len(acts), bool)
    wsum = np.zeros(len(acts))
    total = None
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        for k in range(K):
            arcs = P.walk(al[b, k], labels[b], Tb, Sb, blank)
            if arcs is None:
                continue
            rows = torch.tensor(arcs[0], dtype=torch.int64) + int(off[b])
            c = -a[rows, torch.tensor(arcs[1], dtype=torch.int64)].sum()
            costs[b, k] = float(c.detach())
            visited[rows.numpy()] = True
            wsum[off[b]:off[b + 1]] += abs(w[b, k])
            term = c * float(w[b, k])
            total = term if total is None else total + term
    if total is None:
        return costs, np.zeros(z.shape), visited, wsum
    total.backward()
    return costs, z.grad.numpy(), visited, wsum


def _brute_utt(z, lab, Tb, Sb, wb, we, blank, band=None):
    """_expect_checks._brute_utt for any blank index; band = (lo [T], hi [T]) keeps the paths whose state after every
    frame t lies in [lo[t], hi[t]]."""
    logps, fs = [], []
    for emit in itertools.combinations(range(Tb), Sb):
        s, lp, f, ok = 0, 0.0, 0.0, True
        for t in range(Tb):
            if t in emit:
                lp = lp + z[t, s, int(lab[s])]
                f += float(we[t, s])
                s += 1
            else:
                lp = lp + z[t, s, blank]
                f += float(wb[t, s])
            ok = ok and (band is None or band[0][t] <= s <= band[1][t])
        if ok:
            logps.append(lp)
            fs.append(f)
    logps = torch.stack(logps)
    ll = torch.logsumexp(logps, 0)
    return ll, (torch.exp(logps - ll) * torch.tensor(fs, dtype=torch.float64)).sum()


def _dp_utt(z, lab, Tb, Sb, wb, we, blank, band=None):
    """_expect_checks._dp_utt for any blank index and an optional band."""
    W = Sb + 1
    lpb = z[:, :, blank]
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
        if band is not None:
            ok = ok & (s >= int(band[0][t])) & (s <= int(band[1][t]))
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


def expect_yardstick(acts, labels, T, S, wb, we, ge, gc, blank, brute=False, alignment=None, k=0):
    """expected fp64 [B], costs fp64 [B], grads fp64 [N, V] of sum_b ge[b] expected[b] + gc[b] costs[b] over a'."""
    B = len(T)
    ge = np.ones(B) if ge is None else np.asarray(ge, np.float64)
    gc = np.ones(B) if gc is None else np.asarray(gc, np.float64)
    n = int(offsets(T, S)[-1])
    wb = np.zeros(n) if wb is None else np.asarray(wb, np.float64)
    we = np.zeros(n) if we is None else np.asarray(we, np.float64)
    z, a = transformed(acts, blank)
    off = offsets(T, S)
    exp_, cst, total = np.zeros(B), np.zeros(B), 0.0
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        sl = slice(int(off[b]), int(off[b + 1]))
        band = None if alignment is None else band_of(alignment[b], Tb, k, blank)
        fn = _brute_utt if brute else _dp_utt
        ll, R = fn(a[sl].view(Tb, Sb + 1, -1), labels[b], Tb, Sb, wb[sl].reshape(Tb, Sb + 1),
                   we[sl].reshape(Tb, Sb + 1), blank, band)
        exp_[b], cst[b] = float(R.detach()), float(-ll.detach())
        total = total + float(ge[b]) * R - float(gc[b]) * ll
    total.backward()
    return exp_, cst, z.grad.numpy()


# ---- 1. parity -------------------------------------------------------------------------------------------------------

def pad_shape(T, S):
    return int(T.max()) + 2, int(S.max()) + 3


def check_path_parity(dev, V, blank, K, dtype=None, eps=0.0):
    """Costs and gradients against the yardstick with random signed weights; rows outside every path exact zeros; the
    padded 4-D layout and (GPU) device lengths give the packed / host-length bits."""
    acts, labels, T, S = problem(V, blank)
    al = make_paths(labels, T, S, K, blank)
    w = np.random.default_rng(V + K).standard_normal((len(T), K)).astype(np.float32)
    c, g = dev.path(acts, labels, T, S, al, w, blank, dtype=dtype)
    ref_c, ref_g, visited, wsum = path_yardstick(upcast(acts, dtype), labels, T, S, al, w, blank)
    print(f"path V={V} blank={blank} K={K} {dtype}: max cost error {np.abs(c - ref_c).max():.3e}")
    assert_costs(c, ref_c)
    P.assert_path_grads(g, ref_g, wsum, eps)
    assert np.all(g[~visited] == 0.0)
    pad_T, pad_S1 = pad_shape(T, S)
    cp, gp = dev.path(P.pack_to_padded(acts, T, S, pad_T, pad_S1, np.nan), labels, T, S, al, w, blank, dtype=dtype)
    assert cp.tobytes() == c.tobytes() and P.padded_to_packed(gp, T, S).tobytes() == g.tobytes()
    assert np.all(gp[_padding(T, S, gp.shape)] == 0.0)
    if dev.gpu:
        cd, gd = dev.path(acts, labels, T, S, al, w, blank, dtype=dtype, device_lengths=True)
        assert cd.tobytes() == c.tobytes() and gd.tobytes() == g.tobytes()


def _padding(T, S, shape):
    mask = np.ones(shape[:3], bool)
    for b in range(len(T)):
        mask[b, : T[b], : S[b] + 1] = False
    return mask


def expect_problem(V, blank, seed=0, shp=None):
    acts, labels, T, S = problem(V, blank, seed, shp)
    rng = np.random.default_rng(77 + V + seed)
    wb, we = E.random_costs(rng, T, S)
    ge, gc = E.upstreams(rng, len(T))
    return acts, labels, T, S, wb, we, ge, gc


def assert_expect(res, ref, T, S, wb, we, ge, gc, eps=0.0):
    e, c, g = res
    ref_e, ref_c, ref_g = ref
    Wb = E.cost_bound(wb, we, T, S)
    E.assert_expected(e, ref_e, Wb)
    assert_costs(c, ref_c)
    E.assert_grads(g, ref_g, E.grad_tol(T, S, Wb, ge, gc), eps)


def check_expect_parity(dev, V, blank, dtype=None, eps=0.0):
    """Expected values, costs and gradients of random signed g_e / g_c against the DP yardstick; padded and (GPU)
    device lengths bit-identical."""
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank)
    res = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank, dtype=dtype)
    ref = expect_yardstick(upcast(acts, dtype), labels, T, S, wb, we, ge, gc, blank)
    assert_expect(res, ref, T, S, wb, we, ge, gc, eps)
    pad_T, pad_S1 = pad_shape(T, S)
    pad = lambda x: P.pack_to_padded(x, T, S, pad_T, pad_S1, np.nan)  # noqa: E731
    ep, cp, gp = dev.expect(pad(acts), labels, T, S, pad(wb[:, None])[..., 0], pad(we[:, None])[..., 0], ge, gc, blank,
                            dtype=dtype)
    assert ep.tobytes() == res[0].tobytes() and cp.tobytes() == res[1].tobytes()
    assert P.padded_to_packed(gp, T, S).tobytes() == res[2].tobytes()
    assert np.all(gp[_padding(T, S, gp.shape)] == 0.0)
    if dev.gpu:
        rd = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank, dtype=dtype, device_lengths=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(rd, res))


def check_expect_brute(dev, V, blank):
    """Tiny lattices (T <= 7) against path enumeration over a'."""
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=1, shp=E.BRUTE_SHAPES)
    res = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    ref = expect_yardstick(acts, labels, T, S, wb, we, ge, gc, blank, brute=True)
    assert_expect(res, ref, T, S, wb, we, ge, gc)


# ---- 2. transform identity -------------------------------------------------------------------------------------------

def check_transform_identity(dev, V, blank, K=5):
    """log_softmax(a') = a': the softmax functions on a'.float() give the factorised costs and expected values."""
    acts, labels, T, S, wb, we, _, _ = expect_problem(V, blank, seed=2)
    al = make_paths(labels, T, S, K, blank)
    a32 = transformed(acts, blank)[1].detach().numpy().astype(np.float32)
    c, _ = dev.path(acts, labels, T, S, al, None, blank)
    cs, _ = dev.path(a32, labels, T, S, al, None, blank, hat=False)
    assert_costs(c, cs.astype(np.float64))
    e, lc, _ = dev.expect(acts, labels, T, S, wb, we, None, None, blank)
    es, ls, _ = dev.expect(a32, labels, T, S, wb, we, None, None, blank, hat=False)
    E.assert_expected(e, es.astype(np.float64), E.cost_bound(wb, we, T, S))
    assert_costs(lc, ls.astype(np.float64))


# ---- 3. signed weights -----------------------------------------------------------------------------------------------

def check_signed_weights(dev, V=7, blank=3):
    """+1 on the blank arc and -1 on the label arc of one row: live, blank element -1, the others
    -(softmax' - [label]); all-zero weights: an exactly zero gradient, NaN logit or not."""
    acts, labels, T, S = problem(V, blank, seed=4, shp=[(6, 2)])
    al = make_paths(labels, T, S, 3, blank)[:, 1:]  # labels first | labels last: they leave row (0, 0) by other arcs
    w = np.array([[-1.0, 1.0]], np.float32)         # Wb(0, 0) = +1 (labels last), We(0, 0) = -1 (labels first)
    c, g = dev.path(acts, labels, T, S, al, w, blank)
    ref_c, ref_g, visited, wsum = path_yardstick(acts, labels, T, S, al, w, blank)
    assert_costs(c, ref_c)
    P.assert_path_grads(g, ref_g, wsum)
    assert np.all(g[~visited] == 0.0)
    z = acts[0].astype(np.float64)
    keep = np.arange(V) != blank
    soft = np.zeros(V)
    soft[keep] = np.exp(z[keep] - z[keep].max()) / np.exp(z[keep] - z[keep].max()).sum()
    want = -(soft - (np.arange(V) == labels[0, 0]))
    want[blank] = -1.0
    print("row (0, 0):", g[0], "want", want)
    assert np.abs(g[0] - want).max() <= GRAD_TOL * 2 and abs(g[0, blank] + 1.0) <= P.ULP  # (sum_k |w| = 2)
    bad = acts.copy()
    bad[0, (blank + 1) % V] = np.nan
    for a in (acts, bad):
        _, g0 = dev.path(a, labels, T, S, al, np.zeros((1, 2), np.float32), blank)
        assert np.all(g0 == 0.0)
    wb, we = E.random_costs(np.random.default_rng(5), T, S)
    zero = np.zeros(1, np.float32)
    _, _, g0 = dev.expect(acts, labels, T, S, wb, we, zero, zero, blank)
    assert np.all(g0 == 0.0)


# ---- 4. dominant and suppressed blank --------------------------------------------------------------------------------

def check_blank_logit(dev, V, blank, zb, K=5):
    """z_b = zb on every row over N(0, 1) labels: finite, equal to the yardstick -- the blank element where
    sigmoid(-z_b) underflows or exp(z_b + den') overflows included."""
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=6)
    acts[:, blank] = zb
    al = make_paths(labels, T, S, K, blank)
    w = np.random.default_rng(8).standard_normal((len(T), K)).astype(np.float32)
    c, g = dev.path(acts, labels, T, S, al, w, blank)
    ref_c, ref_g, visited, wsum = path_yardstick(acts, labels, T, S, al, w, blank)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(g)) and np.all(np.isfinite(ref_g))
    assert_costs(c, ref_c)
    P.assert_path_grads(g, ref_g, wsum)
    tol = GRAD_TOL * np.maximum(1.0, wsum)
    assert np.all(np.abs(g[:, blank] - ref_g[:, blank]) <= tol)
    res = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    ref = expect_yardstick(acts, labels, T, S, wb, we, ge, gc, blank)
    assert np.all(np.isfinite(ref[2]))
    assert_expect(res, ref, T, S, wb, we, ge, gc)


# ---- 5. non-finite logits --------------------------------------------------------------------------------------------

def _row(T, S, b, t, s):
    return int(offsets(T, S)[b]) + t * (int(S[b]) + 1) + s


def _others_same(b, T, S, c, g, c0, g0):
    off = offsets(T, S)
    for o in range(len(T)):
        if o != b:
            assert c[o].tobytes() == c0[o].tobytes(), o
            assert g[off[o]:off[o + 1]].tobytes() == g0[off[o]:off[o + 1]].tobytes(), o


def check_path_non_finite(dev, V, blank):
    acts, labels, T, S = problem(V, blank, seed=9, shp=H.SHAPES)
    al = make_paths(labels, T, S, 3, blank)  # k = 1: labels first, k = 2: labels last
    w = np.array([[1.0, -0.5, 2.0]] * 3, np.float32)
    c0, g0 = dev.path(acts, labels, T, S, al, w, blank)
    assert np.all(np.isfinite(c0)) and np.all(np.isfinite(g0))
    other = next(v for v in range(V) if v != blank and v != labels[0, 0])

    def run(edit):
        bad = acts.copy()
        edit(bad)
        return dev.path(bad, labels, T, S, al, w, blank)

    # a NaN logit on row (0, 0) of utterance 0, which every path visits: those costs and that row, nothing else
    r = _row(T, S, 0, 0, 0)
    c, g = run(lambda a: a.__setitem__((r, other), np.nan))
    assert np.all(np.isnan(c[0])) and np.all(np.isnan(g[r]))
    rest = np.ones(len(acts), bool)
    rest[r] = False
    assert g[rest].tobytes() == g0[rest].tobytes()
    _others_same(0, T, S, c, g, c0, g0)
    # z_b = -inf on a row of utterance 2 (S = 0: every path leaves it by blank): +inf
    r2 = _row(T, S, 2, 3, 0)
    c, g = run(lambda a: a.__setitem__((r2, blank), -np.inf))
    assert np.all(c[2] == np.inf)
    _others_same(2, T, S, c, g, c0, g0)
    # a -inf label logit on row (0, 0): the paths that emit there cost +inf, the others stay finite
    c, g = run(lambda a: a.__setitem__((r, labels[0, 0]), -np.inf))
    emit = al[0, :, 0] != blank
    assert emit[1] and not emit[2]
    assert np.all(c[0, emit] == np.inf) and np.all(np.isfinite(c[0, ~emit]))
    _others_same(0, T, S, c, g, c0, g0)
    # z_b = +inf on row (0, 0) of utterance 1 (S = T: every path emits there): NaN
    r1 = _row(T, S, 1, 0, 0)
    c, g = run(lambda a: a.__setitem__((r1, blank), np.inf))
    assert np.all(np.isnan(c[1]))
    _others_same(1, T, S, c, g, c0, g0)

    # every non-blank logit -inf on a row that is left by blank only: nothing of the costs changes, the row's non-blank
    # elements are exact zeros and its blank element is the clean one
    def mask_row(a):
        zb = a[r2, blank]
        a[r2, :] = -np.inf
        a[r2, blank] = zb
    c, g = run(mask_row)
    assert c.tobytes() == c0.tobytes()
    keep = np.arange(V) != blank
    assert np.all(g[r2, keep] == 0.0) and np.isfinite(g[r2, blank]) and g[r2, blank] == g0[r2, blank] != 0.0
    rest = np.ones(len(acts), bool)
    rest[r2] = False
    assert g[rest].tobytes() == g0[rest].tobytes()


def check_expect_non_finite(dev, V, blank):
    """An utterance without a finite ll: NaN expected value and NaN gradient rows; the others untouched."""
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=10, shp=H.SHAPES)
    off = offsets(T, S)
    e0, c0, g0 = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    assert np.all(np.isfinite(e0)) and np.all(np.isfinite(g0))
    other = next(v for v in range(V) if v != blank and v != labels[0, 0])
    for how in ("nan_logit", "masked_label", "inf_blank"):
        bad = acts.copy()
        if how == "nan_logit":
            bad[_row(T, S, 0, 3, 2), other] = np.nan
        elif how == "masked_label":  # label 0 of utterance 0 masked in every row (t, 0): no path survives
            bad[off[0]:off[1]].reshape(T[0], S[0] + 1, -1)[:, 0, labels[0, 0]] = -np.inf
        else:
            bad[_row(T, S, 0, 0, 0), blank] = np.inf
        e, c, g = dev.expect(bad, labels, T, S, wb, we, ge, gc, blank)
        assert np.isnan(e[0]) and np.all(np.isnan(g[off[0]:off[1]])), how
        assert e[1:].tobytes() == e0[1:].tobytes() and c[1:].tobytes() == c0[1:].tobytes(), how
        assert g[off[1]:].tobytes() == g0[off[1]:].tobytes(), how


# ---- 6. consistency with the read-outs -------------------------------------------------------------------------------

def check_path_consistency(dev, V, blank, K=5):
    acts, labels, T, S = problem(V, blank, seed=12)
    L = int(T.max())
    smp = dev.readout("monotonic_rnnt_sample", acts, labels, T, S, blank, num_samples=K, seed=5, max_input_length=L)
    pc, _ = dev.path(acts, labels, T, S, smp.alignments, None, blank)
    assert_costs(pc, smp.path_costs.astype(np.float64))
    best, _ = dev.readout("monotonic_rnnt_align", acts, labels, T, S, blank, max_input_length=L)
    bc, _ = dev.path(acts, labels, T, S, np.ascontiguousarray(best[:, None, :]), None, blank)
    slack = COST_TOL * np.maximum(1.0, np.abs(pc))
    assert np.all(bc <= pc + slack), (bc, pc)


def check_expect_consistency(dev, V, blank):
    acts, labels, T, S, wb, we, _, _ = expect_problem(V, blank, seed=13)
    B = len(T)
    utt = E.utt_of_row(T, S)
    Wb = E.cost_bound(wb, we, T, S)
    e, c, _ = dev.expect(acts, labels, T, S, wb, we, None, None, blank)
    post = dev.readout("monotonic_rnnt_posteriors", acts, labels, T, S, blank)
    rows = np.asarray(post.blank, np.float64).reshape(-1) * wb + np.asarray(post.label, np.float64).reshape(-1) * we
    E.assert_expected(e, np.array([rows[utt == b].sum() for b in range(B)]), Wb)
    # costs: monotonic_rnnt_hat_loss's bits; g_e = 0: its gradient
    gc = np.linspace(-0.5, 2.0, B).astype(np.float32)
    _, c2, g = dev.expect(acts, labels, T, S, wb, we, 0 * gc, gc, blank)
    lc, lg = dev.hat_loss(acts, labels, T, S, gc, blank)
    assert c.tobytes() == lc.tobytes() and c2.tobytes() == lc.tobytes()
    tol = GRAD_TOL * np.abs(gc)[utt][:, None]
    assert np.all(np.abs(g.astype(np.float64) - lg) <= tol), float(np.abs(g - lg).max())
    # constant costs c_b: expected = c_b T_b, and with g_c = 0 a zero gradient
    cval = np.linspace(-2.5, 3.0, B)
    cw = cval[utt].astype(np.float32)
    one = np.ones(B, np.float32)
    e, _, g = dev.expect(acts, labels, T, S, cw, cw, one, 0 * one, blank)
    Wc = E.cost_bound(cw, cw, T, S)
    E.assert_expected(e, cval * T, Wc)
    assert np.all(np.abs(g) <= E.grad_tol(T, S, Wc, one, 0 * one))


# ---- 7. a restricting alignment --------------------------------------------------------------------------------------

def check_restriction(dev, V, blank, k=1):
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=14)
    al = np.ascontiguousarray(make_paths(labels, T, S, 1, blank)[:, 0])
    res = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank, alignment=al, k=k)
    ref = expect_yardstick(acts, labels, T, S, wb, we, ge, gc, blank, alignment=al, k=k)
    assert_expect(res, ref, T, S, wb, we, ge, gc)
    free = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    assert np.any(res[0] != free[0])  # (the band does restrict something)
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=15, shp=[(7, 3), (6, 2), (5, 5)])
    al = np.ascontiguousarray(make_paths(labels, T, S, 1, blank)[:, 0])
    res = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank, alignment=al, k=k)
    ref = expect_yardstick(acts, labels, T, S, wb, we, ge, gc, blank, brute=True, alignment=al, k=k)
    assert_expect(res, ref, T, S, wb, we, ge, gc)


# ---- 8. reproducibility, independence --------------------------------------------------------------------------------

def check_path_reproducible(dev, V, blank, K=5):
    """Two runs are bitwise equal; an utterance alone equals itself inside the batch."""
    acts, labels, T, S = problem(V, blank, seed=16)
    al = make_paths(labels, T, S, K, blank)
    w = np.random.default_rng(17).standard_normal((len(T), K)).astype(np.float32)
    r1 = dev.path(acts, labels, T, S, al, w, blank)
    r2 = dev.path(acts, labels, T, S, al, w, blank)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r1, r2))
    off = offsets(T, S)
    for b in range(len(T)):
        sl = slice(int(off[b]), int(off[b + 1]))
        c, g = dev.path(acts[sl], labels[b:b + 1], T[b:b + 1], S[b:b + 1],
                        np.ascontiguousarray(al[b:b + 1, :, :int(T[b])]), w[b:b + 1], blank)
        assert c.tobytes() == r1[0][b:b + 1].tobytes() and g.tobytes() == r1[1][sl].tobytes(), b
    return (acts, labels, T, S, al, w), r1


def check_expect_reproducible(dev, V, blank):
    acts, labels, T, S, wb, we, ge, gc = expect_problem(V, blank, seed=18)
    r1 = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    r2 = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r1, r2))
    off = offsets(T, S)
    for b in range(len(T)):
        sl = slice(int(off[b]), int(off[b + 1]))
        e, c, g = dev.expect(acts[sl], labels[b:b + 1], T[b:b + 1], S[b:b + 1], wb[sl], we[sl], ge[b:b + 1],
                             gc[b:b + 1], blank)
        assert e.tobytes() == r1[0][b:b + 1].tobytes() and c.tobytes() == r1[1][b:b + 1].tobytes(), b
        assert g.tobytes() == r1[2][sl].tobytes(), b
    return (acts, labels, T, S, wb, we, ge, gc), r1
