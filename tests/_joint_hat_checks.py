"""Host reference and runner of the fused joint's factorised-blank (HAT) loss, for tests/test_gpu_joint_hat.py.

The reference, in this order:
  z    = bf16(tanh(enc + pred)) @ weight.T + bias in fp64 from the bf16 operands, as test_gpu_joint.host_reference
         forms the joint logits (fp32 tanh, round-to-nearest-even to bf16, fp64 products), packed rows;
  a'   = _hat_checks.hat_transform(z)           (a'[b] = log sigmoid(z_b), a'[v] = log sigmoid(-z_b) + z_v - LSE_{u != b})
  c, G'= oracle.oracle_rnnt(a')                 (rows of a' sum to 1 in probability, so log_softmax(a') = a')
  dz   = G' chained back through the transform by torch autograd on the fp64 z
  d_weight = dz^T h, d_bias = sum dz, dpre = (dz weight) (1 - h^2), d_enc / d_pred = dpre summed over s / t,
         exactly as test_gpu_joint.host_reference does.
Each reference is computed once per key and never modified.
"""
import numpy as np
import torch

import oracle as O
from _hat_checks import hat_transform
from test_gpu_joint import close, make_case  # noqa: F401  (the joint tests' cases and gradient bound)

SCALE = [1.0, -0.5, 2.0]
COST_REL = 1e-5  # tests/test_gpu_joint.py: |dc| <= 1e-5 max(1, |c|); gradients: close() = 1.5e-2 max|ref| + 1e-5


def hat_case(seed, H, V, blank, Trange=(8, 24), Smax=8, B=3):
    """make_case with one S = 0 utterance and labels that avoid `blank`."""
    enc, pred, w, bias, labels, T, S = make_case(seed, B, Trange, Smax, H, V)
    S = S.copy()
    S[1] = 0
    if int(S.max()) == 0:  # keep a label arc in the batch
        S[0] = min(int(T[0]), 2)
        if S[0] == 0:
            T = T.copy()
            T[0], S[0] = 3, 2
    labels = np.where(labels == blank, (blank + 1) % V, labels).astype(np.int32)
    need_T, need_S = int(T.max()), int(S.max())
    assert enc.shape[1] >= need_T and pred.shape[1] >= need_S + 1 and labels.shape[1] >= max(1, need_S)
    return enc, pred, w, bias, labels, T, S


def joint_logits(enc, pred, w, bias, T, S):
    """(z fp64 [N, V] packed, [h of utterance b: fp64 [T_b, S_b + 1, H]])"""
    W64 = w.double()
    hs, rows = [], []
    for b in range(len(T)):
        e = enc[b, : T[b]].float()
        p = pred[b, : S[b] + 1].float()
        h = torch.tanh(e[:, None, :] + p[None, :, :]).to(torch.bfloat16).double()
        hs.append(h)
        z = h @ W64.T
        rows.append((z if bias is None else z + bias.double()).reshape(-1, w.shape[0]))
    return torch.cat(rows), hs


_CACHE = {}


def host_reference(enc, pred, w, bias, labels, T, S, blank, scale=None, alignment=None, k=0, key=None):
    """dict(costs [B] f64, d_enc, d_pred, d_w, d_b (fp64 tensors), dz [N, V], a (a' fp64 numpy))."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    z, hs = joint_logits(enc, pred, w, bias, T, S)
    z = z.clone().requires_grad_(True)
    a = hat_transform(z, blank)
    a32 = a.detach().numpy().astype(np.float32)
    costs, G = O.oracle_rnnt(a32, labels, T, S, blank=blank, alignment=alignment, max_shift=k, num_threads=4)
    if scale is not None:
        G = G * np.repeat(np.asarray(scale, np.float64), T * (S + 1))[:, None]
    a.backward(torch.from_numpy(np.ascontiguousarray(G)))
    dz = z.grad
    W64 = w.double()
    d_enc = torch.zeros(enc.shape, dtype=torch.float64)
    d_pred = torch.zeros(pred.shape, dtype=torch.float64)
    d_w = torch.zeros(w.shape, dtype=torch.float64)
    r = 0
    for b in range(len(T)):
        n = int(T[b]) * (int(S[b]) + 1)
        g = dz[r:r + n]
        h = hs[b].reshape(n, -1)
        d_w += g.T @ h
        dpre = ((g @ W64) * (1 - h * h)).reshape(T[b], S[b] + 1, -1)
        d_enc[b, : T[b]] = dpre.sum(1)
        d_pred[b, : S[b] + 1] = dpre.sum(0)
        r += n
    out = dict(costs=costs, d_enc=d_enc, d_pred=d_pred, d_w=d_w, d_b=dz.sum(0), dz=dz, a=a.detach().numpy(),
               z=z.detach())
    if key is not None:
        _CACHE[key] = out
    return out


def run_hat(J, dev, enc, pred, w, bias, labels, T, S, blank, scale=None, alignment=None, k=0, capturable=None):
    """(costs f64 numpy, d_enc, d_pred, d_weight, d_bias) of monotonic_rnnt_joint_hat_loss, (costs * scale).sum()."""
    e = enc.to(dev).requires_grad_(True)
    p = pred.to(dev).requires_grad_(True)
    ww = w.to(dev).requires_grad_(True)
    bb = None if bias is None else bias.to(dev).requires_grad_(True)
    al = None if alignment is None else torch.from_numpy(np.ascontiguousarray(alignment)).to(dev)
    costs = J.monotonic_rnnt_joint_hat_loss(e, p, ww, bb, torch.from_numpy(labels).to(dev), torch.from_numpy(T),
                                            torch.from_numpy(S), blank, al, k, capturable)
    sc = torch.ones(len(T), device=dev) if scale is None else torch.tensor(scale, dtype=torch.float32, device=dev)
    (costs * sc).sum().backward()
    torch.cuda.synchronize()
    return costs.detach().cpu().double().numpy(), e.grad, p.grad, ww.grad, None if bb is None else bb.grad


def assert_costs(c, ref, what=""):
    dev = np.abs(c - ref) / np.maximum(1.0, np.abs(ref))
    print(f"    {what} costs {c} ref {ref} max rel dev {dev.max():.3e}")
    assert np.all(np.isfinite(c)), (what, c)
    assert np.all(dev <= COST_REL), (what, c, ref)


def assert_grads(got, ref, T, S, what=""):
    """The four gradients within the joint's bound, and exact zeros on padding frames / label slots."""
    c, de, dp, dw, db = got
    for x, r, name in ((de, ref["d_enc"], "d_enc"), (dp, ref["d_pred"], "d_pred"), (dw, ref["d_w"], "d_weight"),
                       (db, ref["d_b"], "d_bias")):
        err = (x.double().cpu() - r).abs().max().item()
        print(f"    {what} {name}: max err {err:.3e} of max |ref| {r.abs().max().item():.3e}")
        close(x, r, name=f"{what} {name}")
    for b in range(len(T)):
        assert torch.all(de[b, T[b]:] == 0) and torch.all(dp[b, S[b] + 1:] == 0), (what, b)


def assert_blank_dbias(db, ref, blank, what=""):
    """The blank column of d_bias by itself: |db[blank] - ref| <= 1.5e-2 sum_rows |dz[row, blank]| + 1e-5."""
    err = abs(float(db[blank]) - float(ref["d_b"][blank]))
    lim = 1.5e-2 * float(ref["dz"][:, blank].abs().sum()) + 1e-5
    print(f"    {what} d_bias[blank]: {float(db[blank]):.6e} ref {float(ref['d_b'][blank]):.6e} err {err:.3e} lim {lim:.3e}")
    assert err <= lim, (what, err, lim)
