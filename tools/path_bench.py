"""Time monotonic_rnnt_path_loss (mrnnt_path_forward / mrnnt_path_backward) next to the composition it replaces -- one
alignment-restricted loss step per path (alignment = al_k, max_distance_from_alignment = 0) -- in one process.

  python tools/path_bench.py [--configs headline] [--paths 8] [--steps 5] [--warmup 2]

K paths per utterance are drawn once with monotonic_rnnt_sample (fixed seed). Device-resident lengths, fp32 synthetic
logits, the product library, one gradient buffer shared by every call (the composition's K gradients overwrite one
another: autograd's K - 1 additions of dense buffers, which a training step would also pay, are NOT in its time -- the
reported ratio is a lower bound). Timed with HIP events around: (a) the path forward, (b) path forward + backward, (c)
the K restricted-loss forward + backward steps. A last pass with the library's per-kernel profile gives the gradient
launch's own time and its store rate, N V 4 bytes over that time, for both gradient kernels.
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


def run(config, K, steps, warmup):
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
    Lt = int(T.max())
    smp = op.monotonic_rnnt_sample(acts, labels, Td, Sd, K, 2024, max_input_length=Lt)
    al = smp.alignments.contiguous()
    per_path = [al[:, k].contiguous() for k in range(K)]
    grads = torch.empty_like(acts)
    lib = L.load()
    vp = ctypes.c_void_p
    prep = op._Prepared(acts, labels, Td, Sd, None, 0, 0)
    ws = prep.workspace(num_paths=K)
    pc = torch.empty((B, K), dtype=torch.float32, device=dev)
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((B, K)).astype(np.float32)).to(dev)  # signed

    def path_forward():
        L.check(lib.mrnnt_path_forward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(al.data_ptr()), K,
                                       Lt, vp(pc.data_ptr()), prep.stream()), "mrnnt_path_forward")

    def path_step():
        path_forward()
        L.check(lib.mrnnt_path_backward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(al.data_ptr()), K,
                                        Lt, vp(w.data_ptr()), vp(grads.data_ptr()), prep.stream()), "mrnnt_path_backward")

    restricted = [op._Prepared(acts, labels, Td, Sd, a, 0, 0) for a in per_path]

    def composition():
        for r in restricted:
            _, rws = op._forward(r, with_beta=True)
            op._backward(r, rws, None, grads)

    path_step()
    torch.cuda.synchronize()
    op.check_lengths()
    got, want = pc.cpu().numpy().astype(np.float64), smp.path_costs.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want)), float(np.abs(got / want - 1).max())
    live = int((grads != 0).any(dim=1).sum())
    ms = {"path_forward": _timed(path_forward, steps, warmup), "path_forward_backward": _timed(path_step, steps, warmup),
          "restricted_loss_x_K": _timed(composition, steps, warmup)}
    # per-kernel times of one step each (events around every launch: not the timings above)
    prof = {}
    for name, fn in (("path", path_step), ("restricted", composition)):
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[name] = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
    gbytes = rows * V * 4 / 1e9
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    return {"workload": workload, "B": B, "T_max": Lt, "S_max": int(S.max()), "V": V, "rows": rows, "K": K,
            "steps": steps, "warmup": warmup, "live_rows": live, "median_ms": med,
            "min_ms": {k: round(float(v.min()), 4) for k, v in ms.items()},
            "max_ms": {k: round(float(v.max()), 4) for k, v in ms.items()},
            "composition_over_path": round(med["restricted_loss_x_K"] / med["path_forward_backward"], 3),
            "kernels": prof, "grads_GB": round(gbytes, 3),
            "grad_store_TBps": {"path": round(gbytes / prof["path"]["grad"]["ms"], 3),
                                "restricted_loss": round(gbytes * K / prof["restricted"]["grad"]["ms"], 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="headline")
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    for config in args.configs.split(","):
        print(json.dumps(run(config, args.paths, args.steps, args.warmup), indent=1), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
