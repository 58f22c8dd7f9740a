"""The row state of the gradient arena with inputs that change from step to step.

One acts tensor (B utterances of 201,000 lattice rows each, V logits) and two sets of lengths that lay the same rows
out as different lattices -- (T, S) = (1000, 200) and (804, 249) -- alternate step by step, so the band and the dead
set of every step differ from the step before and only the rows that are zero in both are skipped. Timed in one
process, eager, device lengths: with the row state tracked, and with the state forgotten before every step (every row
is written: the behaviour before the row state). Also reports the share of the gradient's rows skipped per step.

    python tools/zero_rows_bench.py [--B 64] [--V 1024] [--steps 20] [--warmup 4]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "monotonic-rnnt_amd", "pytorch_binding"))
import _grads_placement as GP  # noqa: E402
import _mrnnt_lib as L  # noqa: E402
import monotonic_rnnt_op as op  # noqa: E402

LENGTHS = ((1000, 200), (804, 249))  # 201,000 rows per utterance either way


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--V", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, V = args.B, args.V
    rows = B * LENGTHS[0][0] * (LENGTHS[0][1] + 1)
    assert all(B * T * (S + 1) == rows for T, S in LENGTHS)
    acts = torch.empty((rows, V), dtype=torch.float32, device=dev)
    L.synth_acts(acts.data_ptr(), 0, rows * V, 0, True, torch.cuda.current_stream(dev).cuda_stream)
    acts.requires_grad_(True)
    labels = torch.randint(1, V, (B, max(S for _, S in LENGTHS)), generator=torch.Generator().manual_seed(0),
                           dtype=torch.int32).to(dev)
    lens = [(torch.full((B,), T, dtype=torch.int32, device=dev), torch.full((B,), S, dtype=torch.int32, device=dev))
            for T, S in LENGTHS]

    def step(i, forget):
        acts.grad = None
        if forget:
            GP.forget()
        T, S = lens[i % 2]
        op.monotonic_rnnt_loss(acts, labels, T, S, blank_label=0).sum().backward()

    def timed(forget):
        for i in range(args.warmup):
            step(i, forget)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(args.warmup + i, forget)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def state():
        (t,) = GP.ARENA._track.values()
        torch.cuda.synchronize()
        return t.state[:rows].clone()

    ms = {"forgotten": timed(True), "tracked": timed(False), "forgotten_again": timed(True), "tracked_again": timed(False)}
    vouched0 = GP.ARENA.track_stats["vouched"]
    step(0, False)
    s0 = state()
    step(1, False)
    s1 = state()
    step(2, False)
    s2 = state()
    assert GP.ARENA.track_stats["vouched"] == vouched0 + 3, "the arena did not vouch for the steps measured"
    skipped = [int(((a != 0) & (a == b)).sum()) for a, b in ((s0, s1), (s1, s2))]
    print(json.dumps({
        "workload": f"B={B} V={V} f32, lengths alternating {LENGTHS[0]} / {LENGTHS[1]} per step, eager, device lengths",
        "rows": rows, "steps": args.steps,
        "ms_per_step": {k: round(v, 3) for k, v in ms.items()},
        "zero_rows": [int((s != 0).sum()) for s in (s0, s1)],
        "rows_skipped": skipped, "share_skipped": [round(x / rows, 4) for x in skipped],
        "arena": {**GP.ARENA.stats, **GP.ARENA.track_stats},
    }))


if __name__ == "__main__":
    main()
