"""Time the factorised-blank path scores and expected costs -- monotonic_rnnt_path_loss(blank_factorized=True) and
monotonic_rnnt_expected_cost(blank_factorized=True) -- each next to its softmax twin in the same process, and next to
the PyTorch composition a user would write without them (transform the logits, then the softmax function).

  python tools/hat_weights_bench.py [--config headline] [--rounds 5] [--steps 3] [--warmup 2] [--paths 8]
                                    [--comp-batch 16]

Device-resident lengths, fp32 synthetic logits, the product library, blank 0. Each step is forward + backward through
the autograd surface, timed with HIP events. Path scores: --paths alignments per utterance drawn once by
monotonic_rnnt_sample(blank_factorized=True) and given to both twins (the same rows are live for both), signed
upstream weights. Expected costs: the emission frame on the label arc (expected latency), backward of
(costs + 0.01 latency).sum(). The steps run alternately, round after round, so drift of the device shows up inside
every series alike; the spread of a series is the range of its rounds' medians. The compositions hold several more
N x V tensors: they are timed at the first --comp-batch utterances together with the library steps (the ratio of
record). A last pass with the library's per-kernel profile gives the launches' own times, and the count of gradient
rows that are not all zero says how many rows either gradient pass had to read and write. Prints one JSON object.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hat_bench import _time, transform  # noqa: E402


def run_shape(T, S, V, rounds, steps, warmup, K, comp):
    import _mrnnt_lib as L
    import monotonic_rnnt_op as op

    dev = torch.device("cuda:0")
    B = len(T)
    rows = int(np.sum(T.astype(np.int64) * (S + 1)))
    acts = torch.empty((rows, V), dtype=torch.float32, device=dev)
    L.synth_acts(acts.data_ptr(), 0, rows * V, 0, True, torch.cuda.current_stream().cuda_stream)
    acts.requires_grad_(True)
    rng = np.random.default_rng(1)
    labels = torch.from_numpy(rng.integers(1, V, (B, int(S.max()))).astype(np.int32)).to(dev)
    Td, Sd = torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)
    al = op.monotonic_rnnt_sample(acts.detach(), labels, Td, Sd, num_samples=K, seed=7, max_input_length=int(T.max()),
                                  blank_factorized=True).alignments
    w = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).to(dev)
    frame = torch.from_numpy(np.concatenate([np.repeat(np.arange(t), s + 1) for t, s in zip(T, S)]).astype(np.float32))
    frame = frame.to(dev)

    def path_step(hat, f=lambda z: z):
        acts.grad = None
        op.monotonic_rnnt_path_loss(f(acts), labels, Td, Sd, al, blank_factorized=hat).backward(w)

    def expect_step(hat, f=lambda z: z):
        acts.grad = None
        lat, costs = op.monotonic_rnnt_expected_cost(f(acts), labels, Td, Sd, label_costs=frame, blank_factorized=hat)
        (costs + 0.01 * lat).sum().backward()

    fns = {"path": lambda: path_step(False), "hat_path": lambda: path_step(True),
           "expect": lambda: expect_step(False), "hat_expect": lambda: expect_step(True)}
    if comp:
        fns["path_composition"] = lambda: path_step(False, transform)
        fns["expect_composition"] = lambda: expect_step(False, transform)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    op.check_lengths()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_time(fn, steps))
    prof, nonzero = {}, {}
    for k, fn in fns.items():
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[k] = {n: {"ms": round(v[0], 4), "launches": v[1]} for n, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
        g, n = acts.grad, 0
        for i in range(0, rows, 1 << 20):
            n += int((g[i:i + (1 << 20)] != 0).any(dim=1).sum())
        nonzero[k] = n
    acts.grad = None
    out = {"B": B, "T_max": int(T.max()), "S_max": int(S.max()), "V": V, "rows": rows, "paths": K,
           "acts_GiB": round(rows * V * 4 / 2**30, 2), "rounds": rounds, "steps_per_round": steps, "warmup": warmup}
    for k, v in ms.items():
        med = [float(np.median(r)) for r in v]
        out[k] = {"median_ms": round(float(np.median(np.concatenate([np.asarray(r) for r in v]))), 4),
                  "round_medians_ms": [round(x, 4) for x in med], "spread_ms": round(max(med) - min(med), 4),
                  "min_ms": round(float(min(min(r) for r in v)), 4)}
    out["nonzero_grad_rows"] = nonzero
    for k in ("path", "expect"):
        out[f"hat_{k}_over_{k}"] = round(out["hat_" + k]["median_ms"] / out[k]["median_ms"], 4)
        if comp:
            out[f"{k}_composition_over_hat_{k}"] = round(out[k + "_composition"]["median_ms"] /
                                                         out["hat_" + k]["median_ms"], 3)
    out["kernels"] = prof
    del acts
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="headline")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", type=int, default=8)
    ap.add_argument("--comp-batch", type=int, default=16)
    args = ap.parse_args()
    import _mrnnt_lib as L
    from bench import lengths_for
    T, S, V, workload = lengths_for(args.config, 0, 1)[:4]
    res = {"workload": workload, "library_sha256": L.library_sha256(), "device": torch.cuda.get_device_name(0)}
    res["full"] = run_shape(T, S, V, args.rounds, args.steps, args.warmup, args.paths, comp=False)
    n = min(args.comp_batch, len(T))
    if n > 0:
        res[f"first_{n}"] = run_shape(T[:n], S[:n], V, args.rounds, args.steps, args.warmup, args.paths, comp=True)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
