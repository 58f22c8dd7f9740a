"""Time monotonic_rnnt_joint_align against the fused joint's cost-only forward on one shape (HIP events per call).

  python tools/joint_align_bench.py [--B 64 --T 1000 --S 200 --V 1024 --H 512] [--steps 10] [--warmup 3]

(a) monotonic_rnnt_joint_align; (b) monotonic_rnnt_joint_loss on inputs without requires_grad (cost only, no beta);
(c) monotonic_rnnt_joint_posteriors (the forward with beta + the read-out). (a) and (b) run the same setup, row list and
joint log-softmax pass and differ in their last launch: the Viterbi launch or the alpha recursion. Inputs as
tools/joint_bench.py: N(0, 1) enc / pred, W ~ N(0, 4/H), bias N(0, 0.01), full-length utterances, host lengths. Calls
alternate a, b, c; each is timed by its own pair of events. A second pass collects the per-launch split of
mrnnt_profile_read. Prints one JSON object.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monotonic-rnnt_amd", "pytorch_binding"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--S", type=int, default=200)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import _mrnnt_lib as L
    import monotonic_rnnt_joint as J

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    B, T, S, V, H = a.B, a.T, a.S, a.V, a.H
    enc = torch.randn(B, T, H, device=dev, generator=g).to(torch.bfloat16)
    pred = torch.randn(B, S + 1, H, device=dev, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, H, device=dev, generator=g) * (2.0 / H ** 0.5)).to(torch.bfloat16)
    bias = 0.1 * torch.randn(V, device=dev, generator=g)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, S)).astype(np.int32)).to(dev)
    Tl = torch.full((B,), T, dtype=torch.int32)
    Sl = torch.full((B,), S, dtype=torch.int32)
    args = (enc, pred, W, bias, labels, Tl, Sl)
    fns = (("joint_align", lambda: J.monotonic_rnnt_joint_align(*args)),
           ("joint_loss_cost_only", lambda: J.monotonic_rnnt_joint_loss(*args)),
           ("joint_posteriors", lambda: J.monotonic_rnnt_joint_posteriors(*args)))

    for _ in range(a.warmup):
        (al, ca), cb, post = (fn() for _, fn in fns)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ca).all()) and bool((cb <= ca).all()), "best-path cost below the loss"
    assert bool((post.costs == cb).all()), "posterior costs differ from the loss"
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
          for _ in fns]
    for i in range(a.steps):
        for j, (_, fn) in enumerate(fns):
            ev[j][i][0].record()
            fn()
            ev[j][i][1].record()
    torch.cuda.synchronize()
    ms = [np.array([x.elapsed_time(y) for x, y in e]) for e in ev]
    split = {}
    for name, fn in fns:
        L.profile_enable(True)
        for _ in range(a.steps):
            fn()
        prof = L.profile_read()
        L.profile_enable(False)
        split[name] = {k: round(v[0] / max(1, v[1]), 4) for k, v in prof.items() if v[1]}
    out = {"config": {"B": B, "T": T, "S": S, "V": V, "H": H}, "steps": a.steps, "warmup": a.warmup,
           "ms": {name: {"median": round(float(np.median(m)), 4), "min": round(float(m.min()), 4)}
                  for (name, _), m in zip(fns, ms)},
           "align_minus_cost_only_ms": round(float(np.median(ms[0]) - np.median(ms[1])), 4),
           "per_launch_ms": split,
           "mean_cost": {"align": float(ca.mean()), "loss": float(cb.mean())}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
