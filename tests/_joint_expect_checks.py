"""Yardstick of monotonic_rnnt_joint_expected_cost, independent of the library (tests/test_gpu_joint_expect.py; checked
on the host by tests/test_joint_expect_yardstick.py).

From the same bf16 inputs, on the host in fp64 -- the composition the fused op replaces:
  hs, acts = _joint_path_checks.joint_logits(enc, pred, weight, bias, T, S)        (bf16 activation, fp32 logits)
  expected, costs, dz = _expect_checks.yardstick(acts, labels, T, S, wb, we, ge, gc)
                                                   (dz: the logit gradient of sum_b ge expected + gc costs, autograd)
  d_enc, d_pred, d_weight, d_bias = _joint_path_checks.chain(enc, pred, weight, T, S, hs, dz)
A blank other than _expect_checks.BLANK is brought there by exchanging the two vocabulary entries (columns of acts,
values of labels) and back, as _joint_path_checks.path_yardstick does. Under a restricting alignment (bands: per
utterance the (lo, hi) arrays of _align_checks.band_of) the recursion of _expect_checks._dp_utt runs with the states
after frame t kept inside [lo[t], hi[t]] -- banded_yardstick, which test_joint_expect_yardstick.py holds to
_expect_checks.yardstick without bands and to path enumeration with them.

Cost arrays: wb / we are packed [N] here (one value per lattice row, as _expect_checks has them); grid() scatters them
onto the [B, grid_T, grid_S1] grid the op takes, with garbage in every slot the contract calls never-read.

Tolerances: costs and the four gradients as _joint_path_checks (1e-5 max(1, |c|); 1.5e-2 max|ref| + 1e-5); expected
within COST_TOL + (4e-6 + 2 COST_REL max(1, |cost_b|)) W_b, W_b = _expect_checks.cost_bound: the first term is the
dense op's, the second covers the joint's logits differing from the fp64 composition by what the cost tolerance allows
-- a relative path-probability error of that size times a deviation of at most 2 W_b.
"""
import itertools

import numpy as np
import torch

import _expect_checks as EC
import _joint_path_checks as JC
from _parity import COST_TOL

GARBAGE = 1e30


def random_costs(rng, T, S):
    return EC.random_costs(rng, T, S)


def grid(wb, we, T, S, grid_T, grid_S1, garbage=GARBAGE):
    """(blank_costs, label_costs) fp32 numpy [B, grid_T, grid_S1] (None stays None) from the packed arrays; `garbage`
    at t >= T_b, at s > S_b, and in label_costs at s = S_b."""
    off = EC.offsets(T, S)
    out = []
    for x, is_label in ((wb, False), (we, True)):
        if x is None:
            out.append(None)
            continue
        g = np.full((len(T), grid_T, grid_S1), garbage, np.float32)
        for b, (Tb, Sb) in enumerate(zip(T, S)):
            g[b, :Tb, :Sb + 1] = np.asarray(x[off[b]:off[b + 1]], np.float32).reshape(Tb, Sb + 1)
            if is_label:
                g[b, :Tb, Sb] = garbage
        out.append(g)
    return out[0], out[1]


def _exchange(acts, labels, blank):
    perm = np.arange(acts.shape[1])
    perm[[blank, EC.BLANK]] = perm[[EC.BLANK, blank]]
    return perm, np.ascontiguousarray(acts[:, perm]), perm[labels].astype(labels.dtype)


def _dp_utt_band(z, lab, Tb, Sb, wb, we, lo, hi):
    """_expect_checks._dp_utt with the states after frame t kept inside [lo[t], hi[t]]."""
    NI = EC.NI
    W = Sb + 1
    lpb = z[:, :, EC.BLANK]
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
        ok = (s <= t + 1) & (Sb - s <= Tb - 1 - t) & (s >= int(lo[t])) & (s <= int(hi[t]))
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


def _brute_utt_band(z, lab, Tb, Sb, wb, we, lo, hi):
    """Path enumeration over the paths whose state after every frame t lies in [lo[t], hi[t]]."""
    logps, fs = [], []
    for emit in itertools.combinations(range(Tb), Sb):
        s, lp, f, inside = 0, 0.0, 0.0, True
        for t in range(Tb):
            if t in emit:
                lp = lp + z[t, s, int(lab[s])]
                f += float(we[t, s])
                s += 1
            else:
                lp = lp + z[t, s, EC.BLANK]
                f += float(wb[t, s])
            inside = inside and int(lo[t]) <= s <= int(hi[t])
        if inside:
            logps.append(lp)
            fs.append(f)
    logps = torch.stack(logps)
    ll = torch.logsumexp(logps, 0)
    return ll, (torch.exp(logps - ll) * torch.tensor(fs, dtype=torch.float64)).sum()


def banded_yardstick(acts, labels, T, S, wb, we, ge, gc, bands, brute=False):
    """_expect_checks.yardstick under the restriction of bands[b] = (lo [T_b], hi [T_b])."""
    B = len(T)
    ge = np.ones(B) if ge is None else np.asarray(ge, np.float64)
    gc = np.ones(B) if gc is None else np.asarray(gc, np.float64)
    off = EC.offsets(T, S)
    n = int(off[-1])
    wb = np.zeros(n) if wb is None else np.asarray(wb, np.float64)
    we = np.zeros(n) if we is None else np.asarray(we, np.float64)
    a = torch.tensor(np.asarray(acts, np.float64), requires_grad=True)
    lsm = torch.log_softmax(a, dim=1)
    exp_, cst, total = np.zeros(B), np.zeros(B), 0.0
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        sl = slice(int(off[b]), int(off[b + 1]))
        fn = _brute_utt_band if brute else _dp_utt_band
        ll, R = fn(lsm[sl].view(Tb, Sb + 1, -1), labels[b], Tb, Sb, wb[sl].reshape(Tb, Sb + 1),
                   we[sl].reshape(Tb, Sb + 1), bands[b][0], bands[b][1])
        exp_[b], cst[b] = float(R.detach()), float(-ll.detach())
        total = total + float(ge[b]) * R - float(gc[b]) * ll
    total.backward()
    return exp_, cst, a.grad.numpy()


def logit_yardstick(acts, labels, T, S, wb, we, ge, gc, blank=EC.BLANK, bands=None, brute=False):
    """(expected fp64 [B], costs fp64 [B], dz fp64 [N, V]) on the logits `acts`, for any blank."""
    perm = None
    if blank != EC.BLANK:
        perm, acts, labels = _exchange(acts, labels, blank)
    if bands is None:
        e, c, dz = EC.yardstick(acts, labels, T, S, wb, we, ge, gc, brute)
    else:
        e, c, dz = banded_yardstick(acts, labels, T, S, wb, we, ge, gc, bands, brute)
    return e, c, (dz if perm is None else np.ascontiguousarray(dz[:, perm]))


def yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge=None, gc=None, blank=EC.BLANK, logits=None, bands=None,
              brute=False):
    """(expected, costs, d_enc, d_pred, d_weight, d_bias), fp64, of sum_b ge[b] expected[b] + gc[b] costs[b].
    logits: joint_logits of the same inputs, when the caller shares them among tests."""
    hs, acts = JC.joint_logits(enc, pred, w, bias, T, S) if logits is None else logits
    e, c, dz = logit_yardstick(acts, labels, T, S, wb, we, ge, gc, blank, bands, brute)
    return (e, c) + JC.chain(enc, pred, w, T, S, hs, dz)


def autograd_reference(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank=EC.BLANK, brute=False):
    """The same six quantities from torch.autograd through the fp64 composition, the two roundings passing gradients
    straight through (as _joint_path_checks.autograd_reference)."""
    B = len(T)
    off = EC.offsets(T, S)
    e64 = enc.double().requires_grad_(True)
    p64 = pred.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = (torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()).requires_grad_(True)
    perm = np.arange(w.shape[0])
    perm[[blank, EC.BLANK]] = perm[[EC.BLANK, blank]]
    lab = perm[labels]
    exp_, cst, total = np.zeros(B), np.zeros(B), 0.0
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        x = e64[b, :Tb, None, :] + p64[b, None, : Sb + 1, :]
        hr = torch.tanh(x.detach().float()).to(torch.bfloat16).double()
        h = torch.tanh(x + (torch.atanh(hr) - x).detach())
        a = (h @ w64.T + b64).reshape(-1, w.shape[0])
        a = a + (a.detach().float().double() - a.detach())
        z = torch.log_softmax(a, dim=1)[:, torch.from_numpy(perm)].view(Tb, Sb + 1, -1)
        sl = slice(int(off[b]), int(off[b + 1]))
        fn = EC._brute_utt if brute else EC._dp_utt
        ll, R = fn(z, lab[b], Tb, Sb, np.asarray(wb[sl], np.float64).reshape(Tb, Sb + 1),
                   np.asarray(we[sl], np.float64).reshape(Tb, Sb + 1))
        exp_[b], cst[b] = float(R.detach()), float(-ll.detach())
        total = total + float(ge[b]) * R - float(gc[b]) * ll
    total.backward()
    return (exp_, cst) + tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in (e64, p64, w64, b64))


def expected_tol(ref_costs, Wb):
    """COST_TOL + (4e-6 + 2 COST_REL max(1, |cost_b|)) W_b (module doc)."""
    return COST_TOL + (4e-6 + 2 * JC.COST_REL * np.maximum(1.0, np.abs(ref_costs))) * Wb


def assert_expected(e, ref, ref_costs, Wb, what="expected"):
    e = np.asarray(e, np.float64)
    assert e.shape == ref.shape and np.all(np.isfinite(e)), e
    err, tol = np.abs(e - ref), expected_tol(ref_costs, Wb)
    print(f"{what}: max err {float(err.max()):.3e}, max err / tol = {float((err / tol).max()):.3e}")
    assert np.all(err <= tol), (err, tol)
