"""Time monotonic_rnnt_align against the cost-only loss on one shape, in one process (HIP events per step).

  python tools/align_bench.py [--config headline] [--steps 30] [--warmup 5]

(a) monotonic_rnnt_align; (b) monotonic_rnnt_loss on acts without requires_grad (cost only, no beta). Both run through
the development build with chase = 0 and dyn_fused = 0, so both take the separate-kernel route -- setup kernel, the
same log-softmax pass, then the Viterbi launch (a) or the alpha recursion (b) -- and their difference is the
difference of those last launches. Device-resident lengths, fp32 synthetic logits. Steps alternate a, b; each is timed
by its own pair of events. A second pass collects the per-kernel split of mrnnt_profile_read for each.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="headline")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import _mrnnt_lib as L
    from bench import lengths_for

    L.select_dev()
    for knob in ("chase", "dyn_fused"):
        if L.tune(knob, 0) < 0:
            raise SystemExit(f"align_bench: unknown knob {knob}")
    import monotonic_rnnt_op as op

    dev = torch.device("cuda:0")
    T, S, V, workload = lengths_for(args.config, 0, 1)[:4]
    B = len(T)
    rows = int(np.sum(T.astype(np.int64) * (S + 1)))
    acts = torch.empty((rows, V), dtype=torch.float32, device=dev)
    L.synth_acts(acts.data_ptr(), 0, rows * V, 0, True, torch.cuda.current_stream().cuda_stream)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, int(S.max()))).astype(np.int32)).to(dev)
    Td, Sd = torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)
    L_out = int(T.max())

    def step_a():
        return op.monotonic_rnnt_align(acts, labels, Td, Sd, max_input_length=L_out)

    def step_b():
        return op.monotonic_rnnt_loss(acts, labels, Td, Sd)

    for _ in range(args.warmup):
        al, ca = step_a()
        cb = step_b()
    torch.cuda.synchronize()
    op.check_lengths()
    assert bool(torch.isfinite(ca).all()) and bool((cb <= ca).all()), "best-path cost below the loss"
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
          for _ in range(2)]
    for i in range(args.steps):
        for j, fn in enumerate((step_a, step_b)):
            ev[j][i][0].record()
            fn()
            ev[j][i][1].record()
    torch.cuda.synchronize()
    ms = [np.array([a.elapsed_time(b) for a, b in e]) for e in ev]
    split = {}
    for name, fn in (("align", step_a), ("loss_cost_only", step_b)):
        L.profile_enable(True)
        for _ in range(args.steps):
            fn()
        prof = L.profile_read()
        L.profile_enable(False)
        split[name] = {k: round(v[0] / max(1, v[1]), 4) for k, v in prof.items() if v[1]}
    # where the Viterbi launch's time goes: its recursion has the form of the per-step-barrier alpha kernel
    # (dp_halo = 0), so that kernel's time stands for the recursion and the rest is back-pointer stores + backtrace
    halo = L.tune("dp_halo", 0)
    L.profile_enable(True)
    for _ in range(args.warmup + args.steps):
        step_b()
    prof = L.profile_read()
    L.profile_enable(False)
    L.tune("dp_halo", halo)
    split["loss_cost_only_step_barrier_alpha"] = {k: round(v[0] / max(1, v[1]), 4) for k, v in prof.items() if v[1]}
    out = {"workload": workload, "B": B, "T_max": int(T.max()), "S_max": int(S.max()), "V": V, "rows": rows,
           "steps": args.steps, "warmup": args.warmup,
           "align_ms": {"median": round(float(np.median(ms[0])), 4), "min": round(float(ms[0].min()), 4)},
           "loss_cost_only_ms": {"median": round(float(np.median(ms[1])), 4), "min": round(float(ms[1].min()), 4)},
           "difference_ms": round(float(np.median(ms[0]) - np.median(ms[1])), 4),
           "per_launch_ms": split,
           "mean_cost": {"align": float(ca.mean()), "loss": float(cb.mean())}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
