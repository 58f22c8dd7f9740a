"""Time the path sampler (mrnnt_sample) next to the forward pass it reads and next to the posterior read-out on the
same state, in one process.

  python tools/sample_bench.py [--configs headline,c2] [--samples 1,16,64] [--steps 30] [--warmup 5]

Each step is one call's halves on the same stream and workspace, through the product library: (a)
mrnnt_forward(with_beta = 1), (b) mrnnt_sample with num_samples = K (alignments and path costs), (c) mrnnt_posteriors
with all four outputs. Each is timed by its own pair of HIP events. Device-resident lengths, fp32 synthetic logits. A
second pass replays 20 launches of each from a HIP graph: device time without the host's launch gaps. `spread` is the
largest distance in label positions between two samples of one utterance at one frame: past 96 (the staged window of
mrnnt_sample.hip) lanes leave the LDS path.
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


def run(config, samples, steps, warmup):
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
    Kmax = max(samples)
    out = torch.empty((B, Kmax, Lt), dtype=torch.int32, device=dev)
    pcost = torch.empty((B, Kmax), dtype=torch.float32, device=dev)
    vp = ctypes.c_void_p
    state = {}

    def forward():
        state["costs"], state["ws"] = op._forward(prep, with_beta=True)

    def posteriors():
        L.check(lib.mrnnt_posteriors(ctypes.byref(prep.problem), vp(state["ws"].data_ptr()), vp(blank.data_ptr()),
                                     vp(label.data_ptr()), vp(emit.data_ptr()), Lt, vp(ltime.data_ptr()), Sw,
                                     prep.stream()), "mrnnt_posteriors")

    def sample(K):
        L.check(lib.mrnnt_sample(ctypes.byref(prep.problem), vp(state["ws"].data_ptr()), K, 1234, 0,
                                 vp(out.data_ptr()), Lt, vp(pcost.data_ptr()), prep.stream()), "mrnnt_sample")

    for _ in range(warmup):
        forward()
        sample(Kmax)
        posteriors()
    torch.cuda.synchronize()
    op.check_lengths()
    assert bool(torch.isfinite(state["costs"]).all())
    al = out.cpu().numpy()
    assert np.all((al != 0).sum(axis=2) == S[:, None])  # every sample emits S_b labels
    assert bool((pcost >= state["costs"][:, None] - 1e-3).all())
    pos = np.cumsum(al != 0, axis=2)
    spread = int((pos.max(axis=1) - pos.min(axis=1)).max())
    jobs = [("forward", forward), ("posteriors", posteriors)] + [(f"sample_K{K}", lambda K=K: sample(K)) for K in samples]
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
          for k, _ in jobs}
    for i in range(steps):
        for k, fn in jobs:
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in ev[k]]) for k, _ in jobs}
    graph_ms = {}
    reps = 20
    side = torch.cuda.Stream(dev)
    for k, fn in jobs:
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
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    return {"workload": workload, "B": B, "T_max": Lt, "S_max": int(S.max()), "V": V, "rows": rows, "steps": steps,
            "warmup": warmup, "spread": spread, "median_ms": med, "graph_replay_ms_per_call": graph_ms,
            "min_ms": {k: round(float(v.min()), 4) for k, v in ms.items()},
            "sample_over_forward": {f"K{K}": round(graph_ms[f"sample_K{K}"] / graph_ms["forward"], 4) for K in samples},
            "waves": {f"K{K}": B * ((K + 63) // 64) for K in samples}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="headline,c2")
    ap.add_argument("--samples", default="1,16,64")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    samples = [int(x) for x in args.samples.split(",")]
    for config in args.configs.split(","):
        print(json.dumps(run(config, samples, args.steps, args.warmup), indent=1), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
