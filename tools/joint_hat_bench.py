"""Time monotonic_rnnt_joint_hat_loss (mrnnt_joint_hat_forward / _backward) next to the monotonic_rnnt_joint_loss step
of the same process, and next to the composition a user writes without it (torch joint -> bf16 logits ->
monotonic_rnnt_hat_loss -> autograd).

  python tools/joint_hat_bench.py [--B 64 --T 1000 --S 200 --V 1024 --H 512] [--rounds 5] [--steps 3] [--warmup 2]
                                  [--only loss|hat] [--no-composition] [--trace-steps N]

Synthetic N(0, 1) enc / pred, W ~ N(0, 4/H), bias N(0, 0.01) (tools/joint_bench.py's inputs), blank 0, the product
library. Each step is forward + backward through the autograd surface, timed with HIP events. The steps run
alternately, round after round (loss, hat, loss, ...), so drift of the device shows up inside every series alike; a
series' figure is the median over all its steps, its spread the range of its rounds' medians. The live-row counts of
both steps (mrnnt_joint_live_rows on the state of either forward) say whether a gap comes from the data -- the two
distributions spread their paths over different numbers of rows -- or from the kernels; a last pass with the library's
per-kernel profile gives the launches' own times. The composition materialises [B, T, S + 1, V] bf16 logits and their
gradient: it runs at the largest batch (B, B/2, ...) that fits, together with the fused step at that batch.
--only: that step alone (the process-to-process comparison of two library builds through MRNNT_LIB_PATH).
--trace-steps N: N untimed steps of --only and nothing else (to run under a kernel tracer). Prints one JSON object.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monotonic-rnnt_amd", "pytorch_binding"))


def _time(fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _series(v):
    med = [float(np.median(r)) for r in v]
    return {"median_ms": round(float(np.median(np.concatenate([np.asarray(r) for r in v]))), 4),
            "round_medians_ms": [round(x, 4) for x in med], "spread_ms": round(max(med) - min(med), 4),
            "min_ms": round(float(min(min(r) for r in v)), 4)}


def inputs(B, T, S, V, H, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(B, T, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    pred = torch.randn(B, S + 1, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    W = (torch.randn(V, H, device=dev, generator=g) * (2.0 / H ** 0.5)).to(torch.bfloat16).requires_grad_(True)
    bias = (0.1 * torch.randn(V, device=dev, generator=g)).requires_grad_(True)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, S)).astype(np.int32)).to(dev)
    return enc, pred, W, bias, labels, torch.full((B,), T, dtype=torch.int32), torch.full((B,), S, dtype=torch.int32)


def run(a, B, only=None, composition=False):
    import _mrnnt_lib as L
    import monotonic_rnnt_joint as J
    import monotonic_rnnt_op as op

    dev = torch.device("cuda:0")
    enc, pred, W, bias, labels, Tl, Sl = inputs(B, a.T, a.S, a.V, a.H, dev)
    leaves = (enc, pred, W, bias)

    def step(loss):
        def fn():
            for x in leaves:
                x.grad = None
            c = loss(enc, pred, W, bias, labels, Tl, Sl)
            c.sum().backward()
            return c
        return fn

    def comp_step():
        for x in leaves:
            x.grad = None
        h = torch.tanh(enc[:, :, None, :] + pred[:, None, :, :])
        z = torch.nn.functional.linear(h, W, bias.to(torch.bfloat16))  # [B, T, S + 1, V] bf16
        c = op.monotonic_rnnt_hat_loss(z, labels, Tl, Sl)
        c.sum().backward()
        return c

    fns = {}
    if only in (None, "loss"):
        fns["loss"] = step(J.monotonic_rnnt_joint_loss)
    if only in (None, "hat"):
        fns["hat"] = step(J.monotonic_rnnt_joint_hat_loss)
    if composition:
        fns = {"hat": step(J.monotonic_rnnt_joint_hat_loss), "composition": comp_step}
    if a.trace_steps:
        for fn in fns.values():
            for _ in range(a.trace_steps):
                fn()
        torch.cuda.synchronize()
        return {"traced_steps": a.trace_steps, "steps": list(fns)}
    out = {"B": B, "T": a.T, "S": a.S, "V": a.V, "H": a.H, "rounds": a.rounds, "steps_per_round": a.steps,
           "warmup": a.warmup}
    costs = {}
    for k, fn in fns.items():
        for _ in range(a.warmup):
            costs[k] = fn().detach()
    torch.cuda.synchronize()
    if composition:
        out["peak_mem_GiB"] = round(torch.cuda.max_memory_allocated() / 2**30, 1)
        out["max_rel_cost_diff"] = float(((costs["hat"].double() - costs["composition"].double()).abs()
                                          / costs["composition"].double().abs().clamp(min=1)).max())
    out["cost_mean"] = {k: round(float(v.mean()), 3) for k, v in costs.items()}
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms[k].append(_time(fn, a.steps))
    for k, v in ms.items():
        out[k] = _series(v)
    prof = {}
    for k, fn in fns.items():
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[k] = {n: {"ms": round(v[0], 4), "launches": v[1]} for n, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
    out["kernels"] = prof
    if not composition:
        live = {}
        for k in fns:
            prep = J._JointPrepared(enc.detach(), pred.detach(), W.detach(), bias.detach(), labels, Tl, Sl, 0,
                                    **({"hat": True} if k == "hat" else {}))
            _, ws = prep.forward(with_beta=True)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            L.check(L.load().mrnnt_joint_live_rows(ctypes.byref(prep.problem), ctypes.c_void_p(ws.data_ptr()),
                                                   ctypes.c_void_p(cnt.data_ptr()), prep.stream()),
                    "mrnnt_joint_live_rows")
            live[k] = int(cnt.item())
            del ws, prep
        out["live_rows"] = live
        out["in_band_rows"] = B * ((a.S + 1) * (a.T - a.S + 1) - 1)
    if "loss" in out and "hat" in out:
        out["hat_over_loss"] = round(out["hat"]["median_ms"] / out["loss"]["median_ms"], 4)
    if composition:
        out["composition_over_hat"] = round(out["composition"]["median_ms"] / out["hat"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--S", type=int, default=200)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["loss", "hat"], default=None)
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    import _mrnnt_lib as L
    res = {"library": os.path.relpath(L.LIB_PATH, ROOT), "library_sha256": L.library_sha256(L.LIB_PATH),
           "device": torch.cuda.get_device_name(0)}
    res["fused"] = run(a, a.B, only=a.only)
    if a.only is None and not a.no_composition and not a.trace_steps:
        B = a.B
        while B >= 1:
            try:
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                res["composition"] = run(a, B, composition=True)
                break
            except torch.cuda.OutOfMemoryError:
                res.setdefault("composition_out_of_memory_at_B", []).append(B)
                B //= 2
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
