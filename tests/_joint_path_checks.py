"""Yardstick of monotonic_rnnt_joint_path_loss, independent of the library (tests/test_gpu_joint_path_loss.py; checked
on the host by tests/test_joint_path_yardstick.py).

From the same bf16 inputs, on the host in fp64 -- the composition the fused op replaces:
  h    = bf16(tanh(enc + pred))                    (fp32 tanh, round-to-nearest-even to bf16, like the kernel)
  acts = h @ weight.T + bias, rounded to fp32
  costs, dz = _path_checks.yardstick(acts, labels, T, S, al, w)       (gather of log_softmax along the walks; autograd)
then the chain of test_gpu_joint.host_reference:
  dweight = dz^T h, dbias = sum dz, dpre = (dz weight) (1 - h^2), d_enc / d_pred = dpre summed over s / t.

Tolerances are the project's own for this arithmetic (tests/test_gpu_joint.py): costs within 1e-5 max(1, |c|), each
gradient tensor within 1.5e-2 max|ref| + 1e-5 (the logit gradient is stored as bf16 and dH = G weight is a bf16 GEMM).
"""
import numpy as np
import torch

import _path_checks as PC

COST_REL = 1e-5
GRAD_REL = 1.5e-2


def joint_logits(enc, pred, w, bias, T, S):
    """(hs: per utterance fp64 [T_b, S_b + 1, H], acts: fp32 numpy [N, V] packed) from bf16 enc / pred / w (CPU)."""
    W64 = w.double()
    b64 = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    hs, rows = [], []
    for b in range(len(T)):
        e = enc[b, : T[b]].float()
        p = pred[b, : S[b] + 1].float()
        h = torch.tanh(e[:, None, :] + p[None, :, :]).to(torch.bfloat16).double()
        hs.append(h)
        rows.append((h @ W64.T + b64).reshape(-1, w.shape[0]))
    return hs, torch.cat(rows).float().numpy()


def path_yardstick(acts, labels, T, S, al, wts, blank):
    """(costs fp64 [B, K], dz fp64 [N, V]) of _path_checks.yardstick; a blank other than its BLANK is brought there by
    exchanging the two vocabulary entries (columns of acts, values of labels and alignments) and back."""
    if blank == PC.BLANK:
        return PC.yardstick(acts, labels, T, S, al, wts)[:2]
    perm = np.arange(acts.shape[1])
    perm[[blank, PC.BLANK]] = perm[[PC.BLANK, blank]]
    al2 = np.where(al >= 0, perm[np.maximum(al, 0)], al).astype(al.dtype)
    costs, dz = PC.yardstick(np.ascontiguousarray(acts[:, perm]), perm[labels].astype(labels.dtype), T, S, al2, wts)[:2]
    return costs, np.ascontiguousarray(dz[:, perm])


def chain(enc, pred, w, T, S, hs, dz):
    """(d_enc, d_pred, d_weight, d_bias) fp64 from the logit gradient dz [N, V] (numpy) and the activations hs."""
    W64 = w.double()
    dz = torch.from_numpy(np.asarray(dz, np.float64))
    d_enc = torch.zeros(enc.shape, dtype=torch.float64)
    d_pred = torch.zeros(pred.shape, dtype=torch.float64)
    d_w = torch.zeros(w.shape, dtype=torch.float64)
    r = 0
    for b in range(len(T)):
        n = int(T[b]) * (int(S[b]) + 1)
        g = dz[r:r + n]
        h = hs[b].reshape(n, -1)
        d_w += g.T @ h
        dpre = ((g @ W64) * (1 - h * h)).reshape(int(T[b]), int(S[b]) + 1, -1)
        d_enc[b, : T[b]] = dpre.sum(1)
        d_pred[b, : S[b] + 1] = dpre.sum(0)
        r += n
    return d_enc, d_pred, d_w, dz.sum(0)


def yardstick(enc, pred, w, bias, labels, T, S, al, wts=None, blank=PC.BLANK, logits=None):
    """costs fp64 [B, K] (+inf: invalid row) and (d_enc, d_pred, d_weight, d_bias) fp64 of sum_valid wts * costs.
    logits: joint_logits of the same inputs, when the caller shares them among tests."""
    hs, acts = joint_logits(enc, pred, w, bias, T, S) if logits is None else logits
    costs, dz = path_yardstick(acts, labels, T, S, al, wts, blank)
    return (costs,) + chain(enc, pred, w, T, S, hs, dz)


def autograd_reference(enc, pred, w, bias, labels, T, S, al, wts=None, blank=PC.BLANK):
    """The same quantities from torch.autograd through the fp64 composition. The two roundings pass gradients straight
    through: the fp32 rounding of acts as acts + (rounded - acts).detach(), the bf16 rounding of the activation in its
    pre-activation, h = tanh(x + (atanh(bf16(tanh(x))) - x).detach()) -- so that the derivative is 1 - h^2 at the
    rounded h, as the kernels (and the hand-written chain) form it. fp64 throughout."""
    B, K = al.shape[:2]
    wts = np.ones((B, K)) if wts is None else np.asarray(wts, np.float64)
    e64 = enc.double().requires_grad_(True)
    p64 = pred.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = (torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()).requires_grad_(True)
    costs = np.full((B, K), np.inf)
    total = None
    for b in range(B):
        Tb, Sb = int(T[b]), int(S[b])
        x = e64[b, :Tb, None, :] + p64[b, None, : Sb + 1, :]
        hr = torch.tanh(x.detach().float()).to(torch.bfloat16).double()
        h = torch.tanh(x + (torch.atanh(hr) - x).detach())
        a = (h @ w64.T + b64).reshape(-1, w.shape[0])
        a = a + (a.detach().float().double() - a.detach())
        lsm = torch.log_softmax(a, dim=1)
        for k in range(K):
            arcs = PC.walk(al[b, k], labels[b], Tb, Sb, blank)
            if arcs is None:
                continue
            c = -lsm[torch.tensor(arcs[0], dtype=torch.int64), torch.tensor(arcs[1], dtype=torch.int64)].sum()
            costs[b, k] = float(c.detach())
            term = c * float(wts[b, k])
            total = term if total is None else total + term
    if total is None:
        z = torch.zeros
        return costs, z(enc.shape).double(), z(pred.shape).double(), z(w.shape).double(), z(w.shape[0]).double()
    total.backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad for t in (e64, p64, w64, b64)]
    return (costs,) + tuple(grads)


def close(x, ref, name="", rel=GRAD_REL):
    """max |x - ref| <= rel max|ref| + 1e-5 (test_gpu_joint.close); prints the figure first."""
    x = x.detach().double().cpu()
    ref = ref.double()
    err = (x - ref).abs().max().item() if ref.numel() else 0.0
    lim = rel * (ref.abs().max().item() if ref.numel() else 0.0) + 1e-5
    print(f"{name}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, (name, err, lim)


def assert_costs(c, ref, rel=COST_REL):
    c = np.asarray(c, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(c[~fin], ref[~fin]), (c, ref)  # +inf in the same places
    err = np.abs(c[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    print("path costs: max rel err", float(err.max()) if err.size else 0.0)
    assert np.all(err <= rel), (c, ref)


def extreme_paths(labels, T, S, L, blank=PC.BLANK):
    """_path_checks.extreme_paths ([B, 2, L]: all labels first, all labels last) for any blank."""
    if blank == PC.BLANK:
        return PC.extreme_paths(labels, T, S, L)
    out = np.full((len(T), 2, L), blank, np.int32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, 0, :Sb] = labels[b, :Sb]
        out[b, 1, Tb - Sb:Tb] = labels[b, :Sb]
    return out


def make_case(seed, shapes, H, V, blank=PC.BLANK):
    """bf16 enc / pred / weight, fp32 bias, labels (never the blank), T, S for the ragged shapes [(T, S)]."""
    rng = np.random.default_rng(seed)
    T = np.array([t for t, _ in shapes], np.int32)
    S = np.array([s for _, s in shapes], np.int32)
    B, Tm, Sm = len(T), int(T.max()), int(S.max())
    enc = torch.from_numpy(rng.standard_normal((B, Tm + 1, H)).astype(np.float32)).to(torch.bfloat16)
    pred = torch.from_numpy(rng.standard_normal((B, Sm + 2, H)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy((rng.standard_normal((V, H)) / np.sqrt(H) * 2.0).astype(np.float32)).to(torch.bfloat16)
    bias = torch.from_numpy(0.1 * rng.standard_normal(V).astype(np.float32))
    labels = rng.integers(0, V - 1, (B, max(1, Sm))).astype(np.int32)
    labels = np.where(labels >= blank, labels + 1, labels).astype(np.int32)  # [0, V) without the blank
    return enc, pred, w, bias, labels, T, S
