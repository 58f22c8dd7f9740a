"""Time monotonic_rnnt_joint_path_loss (mrnnt_joint_path_*) next to the two routes it replaces, in one process.

  python tools/joint_path_bench.py [--config headline|c2] [--H 512] [--paths 8] [--steps 5] [--warmup 2] [--no-unfused]

K paths per utterance are drawn once with monotonic_rnnt_joint_sample (fixed seed); signed random path weights. Timed
with HIP events, median of --steps after --warmup:
  (a) the joint path forward, and forward + backward through autograd: default (one 8-byte read-back of the path-live
      row count) and capturable (buffers sized by mrnnt_joint_path_row_bound); then one pass stage by stage --
      forward (walk, hull, row list, joint log-softmax, score), rows (coefficients, path-live list), gradient pass,
      dweight GEMM, dH GEMM, reduce -- with the library's per-kernel profile of the same step beside it (the row-list
      launches are the stages' remainders), and the path-live row count against its bound;
  (b) the K restricted joint-loss steps (alignment = al_k, max_distance_from_alignment = 0);
  (c) the materialised bf16 logits followed by monotonic_rnnt_path_loss.
Prints one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monotonic-rnnt_amd", "pytorch_binding"))
sys.path.insert(0, ROOT)


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def _stat(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="headline")
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-unfused", action="store_true", help="skip (c), the materialised logits")
    a = ap.parse_args()
    import _mrnnt_lib as L
    import monotonic_rnnt_joint as J
    import monotonic_rnnt_op as op
    from bench import lengths_for

    dev = torch.device("cuda:0")
    Tn, Sn, V, workload = lengths_for(a.config, 0, 1)[:4]
    B, T, S, H, K = len(Tn), int(Tn.max()), int(Sn.max()), a.H, a.paths
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(B, T, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    pred = torch.randn(B, S + 1, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    W = (torch.randn(V, H, device=dev, generator=g) * (2.0 / H ** 0.5)).to(torch.bfloat16).requires_grad_(True)
    bias = (0.1 * torch.randn(V, device=dev, generator=g)).requires_grad_(True)
    leaves = (enc, pred, W, bias)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, S)).astype(np.int32)).to(dev)
    Tl, Sl = torch.from_numpy(Tn), torch.from_numpy(Sn)
    with torch.no_grad():
        smp = J.monotonic_rnnt_joint_sample(enc, pred, W, bias, labels, Tl, Sl, K, 2024)
    al = smp.alignments.contiguous()
    per_path = [al[:, k].contiguous() for k in range(K)]
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((B, K)).astype(np.float32)).to(dev)  # signed

    def clear():
        for x in leaves:
            x.grad = None

    def path_forward():
        with torch.no_grad():
            return J.monotonic_rnnt_joint_path_loss(enc, pred, W, bias, labels, Tl, Sl, al)

    def path_step(capturable):
        clear()
        pc = J.monotonic_rnnt_joint_path_loss(enc, pred, W, bias, labels, Tl, Sl, al, capturable=capturable)
        pc.backward(w)
        return pc

    def restricted():
        clear()
        for k in range(K):
            c = J.monotonic_rnnt_joint_loss(enc, pred, W, bias, labels, Tl, Sl, alignment=per_path[k],
                                            max_distance_from_alignment=0)
            (c * w[:, k]).sum().backward()

    def materialised():
        clear()
        h = torch.tanh(enc[:, :, None, :] + pred[:, None, :, :])
        z = torch.nn.functional.linear(h, W, bias.to(torch.bfloat16))  # [B, T, S + 1, V] bf16
        op.monotonic_rnnt_path_loss(z, labels, Tl, Sl, al).backward(w)

    pc = path_step(False)
    torch.cuda.synchronize()
    got, want = pc.detach().cpu().double().numpy(), smp.path_costs.cpu().double().numpy()
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want)), float(np.abs(got / want - 1).max())

    out = {"workload": workload, "B": B, "T": T, "S": S, "V": V, "H": H, "K": K, "steps": a.steps, "warmup": a.warmup,
           "lattice_rows": int(np.sum(Tn.astype(np.int64) * (Sn + 1)))}
    out["a_path_forward"] = _stat(_timed(path_forward, a.steps, a.warmup))
    out["a_path_forward_backward"] = _stat(_timed(lambda: path_step(False), a.steps, a.warmup))
    out["a_path_forward_backward_capturable"] = _stat(_timed(lambda: path_step(True), a.steps, a.warmup))

    # one step stage by stage (the autograd Function's own calls), HIP events around each stage
    prep = J._JointPrepared(enc.detach(), pred.detach(), W.detach(), bias.detach(), labels, Tl, Sl, 0)
    wt = W.detach().t().contiguous().t()
    box = {}

    def stages(capturable):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        marks[0].record()
        _, ws = prep.path_forward(al)
        marks[1].record()
        db = torch.zeros(V, dtype=torch.float32, device=dev) if J._dbias_in_pass(H, V) else None
        # (rows + gradient pass in one call of the binding: split below by the library's profile)
        G, Hact = prep.path_backward_rows(ws, al, w, dbias=db, capturable=capturable)
        marks[2].record()
        marks[3].record()
        J._split_k_weight_grad(G, Hact)
        marks[4].record()
        dH = G @ wt
        marks[5].record()
        prep.reduce(ws, dH, Hact, True, True, scratch=G)
        marks[6].record()
        box["rows"] = G.shape[0]
        return marks

    for cap in (False, True):
        for _ in range(a.warmup):
            stages(cap)
        runs = []
        for _ in range(a.steps):
            m = stages(cap)
            torch.cuda.synchronize()
            runs.append([m[i].elapsed_time(m[i + 1]) for i in range(6)])
        med = np.median(np.array(runs), axis=0)
        L.profile_enable(True)
        stages(cap)
        torch.cuda.synchronize()
        prof = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
        out["a_stages_capturable" if cap else "a_stages"] = {
            "forward_ms": round(float(med[0]), 4), "rows_and_gradient_pass_ms": round(float(med[1]), 4),
            "dweight_ms": round(float(med[3]), 4), "dH_ms": round(float(med[4]), 4), "reduce_ms": round(float(med[5]), 4),
            "row_buffers": box["rows"], "library_profile": prof}
    cnt = prep.path_rows(prep.path_forward(al)[1], al, w)
    out["path_live_rows"] = int(cnt.item())
    out["path_row_bound"] = prep.path_row_bound(K)
    nb = ctypes_row_bound(L, prep)
    out["in_band_rows"] = nb

    out["b_restricted_joint_loss_x_K"] = _stat(_timed(restricted, a.steps, a.warmup))
    if not a.no_unfused:
        torch.cuda.empty_cache()
        out["c_materialised_logits_path_loss"] = _stat(_timed(materialised, a.steps, a.warmup))
        out["c_peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
    base = out["a_path_forward_backward"]["median_ms"]
    out["b_over_a"] = round(out["b_restricted_joint_loss_x_K"]["median_ms"] / base, 3)
    if not a.no_unfused:
        out["c_over_a"] = round(out["c_materialised_logits_path_loss"]["median_ms"] / base, 3)
    out["capturable_over_default"] = round(out["a_path_forward_backward_capturable"]["median_ms"] / base, 3)
    print(json.dumps(out), flush=True)


def ctypes_row_bound(L, prep):
    import ctypes
    nb = ctypes.c_int64(0)
    L.check(L.load().mrnnt_joint_row_bound(ctypes.byref(prep.problem), ctypes.byref(nb)), "joint_row_bound")
    return nb.value


if __name__ == "__main__":
    main()
