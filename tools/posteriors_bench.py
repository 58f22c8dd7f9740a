"""Time the posterior read-out (mrnnt_posteriors) next to the forward pass it reads, in one process.

  python tools/posteriors_bench.py [--configs headline,c2] [--steps 30] [--warmup 5]

Each step is one call's two halves on the same stream and workspace, through the product library: (a)
mrnnt_forward(with_beta = 1), (b) mrnnt_posteriors with all four outputs. Each half is timed by its own pair of HIP
events. Device-resident lengths, fp32 synthetic logits. A second pass times (b) alone per output group: the per-row
pair + emit (the column workgroups, with the utterance workgroups' fills) and label_time (the utterance workgroups).
A third pass replays 20 calls of each from a HIP graph: device time without the host's launch gaps. Effective bytes/s
of the read-out counts what its kernel must move: per in-band row lp (16 B), alpha and beta (8 + 8 B; the shifted
beta reads share their lines) for the column workgroups and again for the label-time workgroups, plus the two fp32
stores per lattice row.
Prints one JSON object per config.
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
sys.path.insert(0, ROOT)


def band_rows(T, S):
    """In-band lattice rows: sum_b sum_t (min(t, S) - max(0, t - (T - S)) + 1)."""
    n = 0
    for Tb, Sb in zip(T.astype(np.int64), S.astype(np.int64)):
        t = np.arange(Tb)
        n += int(np.sum(np.minimum(t, Sb) - np.maximum(0, t - (Tb - Sb)) + 1))
    return n


def run(config, steps, warmup):
    import _mrnnt_lib as L
    import monotonic_rnnt_op as op
    from bench import lengths_for

    dev = torch.device("cuda:0")
    T, S, V, workload = lengths_for(config, 0, 1)[:4]
    B = len(T)
    rows = int(np.sum(T.astype(np.int64) * (S + 1)))
    acts = torch.empty((rows, V), dtype=torch.float32, device=dev)
    L.synth_acts(acts.data_ptr(), 0, rows * V, 0, True, torch.cuda.current_stream().cuda_stream)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, int(S.max()))).astype(np.int32)).to(dev)
    Td, Sd = torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)
    Lt, Sw = int(T.max()), labels.size(1)
    prep = op._Prepared(acts, labels, Td, Sd, None, 0, 0)
    lib = L.load()
    blank = torch.empty(rows, dtype=torch.float32, device=dev)
    label = torch.empty_like(blank)
    emit = torch.empty((B, Lt), dtype=torch.float32, device=dev)
    ltime = torch.empty((B, Sw), dtype=torch.float32, device=dev)
    vp = ctypes.c_void_p
    state = {}

    def forward():
        state["costs"], state["ws"] = op._forward(prep, with_beta=True)

    def readout(rows_too=True, time_too=True):
        L.check(lib.mrnnt_posteriors(ctypes.byref(prep.problem), vp(state["ws"].data_ptr()),
                                     vp(blank.data_ptr()) if rows_too else None,
                                     vp(label.data_ptr()) if rows_too else None,
                                     vp(emit.data_ptr()) if rows_too else None, Lt,
                                     vp(ltime.data_ptr()) if time_too else None, Sw, prep.stream()), "mrnnt_posteriors")

    for _ in range(warmup):
        forward()
        readout()
    torch.cuda.synchronize()
    op.check_lengths()
    assert bool(torch.isfinite(state["costs"]).all())
    if len(set(zip(T.tolist(), S.tolist()))) == 1:  # equal shapes: every frame's arcs sum to 1
        err = float(((blank + label).view(B, int(T[0]), int(S[0]) + 1).sum(-1) - 1.0).abs().max())
        assert err < 1e-3, err
    names = ("forward", "readout", "rows_and_emit", "label_time")
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k in names}
    for i in range(steps):
        for k, fn in (("forward", forward), ("readout", readout)):
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    for i in range(steps):
        for k, fn in (("rows_and_emit", lambda: readout(True, False)), ("label_time", lambda: readout(False, True))):
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in ev[k]]) for k in names}
    # the same launches replayed from a HIP graph, `reps` calls per graph: device time without the host's launch gaps
    # (at small shapes the eager figures above are bound by the host issuing the launches)
    graph_ms = {}
    reps = 20
    side = torch.cuda.Stream(dev)
    for k, fn in (("forward", forward), ("readout", readout), ("rows_and_emit", lambda: readout(True, False)),
                  ("label_time", lambda: readout(False, True))):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(reps):
                    fn()
            g.replay()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                g.replay()
            b.record()
        torch.cuda.synchronize()
        graph_ms[k] = round(a.elapsed_time(b) / (5 * reps), 4)
        forward()  # the workspace the next read-outs use, outside the graph's pool
        torch.cuda.synchronize()
    inb = band_rows(T, S)
    moved = inb * (16 + 8 + 8) * 2 + rows * 8 + (B * Lt + B * Sw) * 4
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    return {"workload": workload, "B": B, "T_max": Lt, "S_max": int(S.max()), "V": V, "rows": rows, "band_rows": inb,
            "steps": steps, "warmup": warmup, "median_ms": med, "graph_replay_ms_per_call": graph_ms,
            "min_ms": {k: round(float(v.min()), 4) for k, v in ms.items()},
            "readout_over_forward": round(med["readout"] / med["forward"], 4),
            "readout_bytes": moved, "readout_GBps": round(moved / (med["readout"] * 1e-3) / 1e9, 1),
            "forward_acts_bytes": rows * V * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="headline,c2")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    for config in args.configs.split(","):
        print(json.dumps(run(config, args.steps, args.warmup), indent=1), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
