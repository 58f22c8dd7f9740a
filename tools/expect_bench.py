"""Time monotonic_rnnt_expected_cost (mrnnt_expect_forward / mrnnt_expect_backward) next to the monotonic_rnnt_loss
step of the same process.

  python tools/expect_bench.py [--configs headline,c2] [--steps 5] [--warmup 2]

Device-resident lengths, fp32 synthetic logits, the product library, latency costs (label_costs = the frame index t,
no blank costs). Timed with HIP events around: (a) the expected-cost forward (the loss's forward with beta, then the
expectation recursion), (b) the step (expected + costs).sum().backward() through the autograd surface, (c) the step
monotonic_rnnt_loss(...).sum().backward(). A last pass with the library's per-kernel profile gives the launches' own
times; the expectation recursion's is the alpha_beta total of (a) minus that of the loss's forward (where the chase
launch carries the loss's recursion, all of it).
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
    acts.requires_grad_(True)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, int(S.max()))).astype(np.int32)).to(dev)
    Td, Sd = torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)
    we = torch.cat([torch.arange(int(t), dtype=torch.float32).repeat_interleave(int(s) + 1) for t, s in zip(T, S)]).to(dev)
    lib = L.load()
    vp = ctypes.c_void_p
    prep = op._Prepared(acts.detach(), labels, Td, Sd, None, 0, 0)
    ws = prep.workspace(expect=True)
    ex = torch.empty(B, dtype=torch.float32, device=dev)
    cs = torch.empty(B, dtype=torch.float32, device=dev)

    def expect_forward():
        L.check(lib.mrnnt_expect_forward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), None,
                                         vp(we.data_ptr()), vp(ex.data_ptr()), vp(cs.data_ptr()), 1, prep.stream()),
                "mrnnt_expect_forward")

    def loss_forward():
        op._forward(prep, with_beta=True)

    def expect_step():
        acts.grad = None
        e, c = op.monotonic_rnnt_expected_cost(acts, labels, Td, Sd, None, we)
        (e + c).sum().backward()

    def loss_step():
        acts.grad = None
        op.monotonic_rnnt_loss(acts, labels, Td, Sd).sum().backward()

    expect_step()
    torch.cuda.synchronize()
    op.check_lengths()
    expect_forward()
    torch.cuda.synchronize()
    expected = ex.cpu().numpy().astype(np.float64)
    # the value: the posteriors-weighted cost of the same inputs
    post = op.monotonic_rnnt_posteriors(acts.detach(), labels, Td, Sd, max_input_length=int(T.max()))
    ref = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(
        0, torch.repeat_interleave(torch.arange(B, device=dev), torch.from_numpy(T.astype(np.int64) * (S + 1)).to(dev)),
        post.label.double() * we.double()).cpu().numpy()
    del post
    bound = np.array([float(np.arange(int(t)).sum()) for t in T])
    assert np.all(np.abs(expected - ref) <= 1e-4 + 4e-6 * bound), float(np.abs(expected - ref).max())
    ms = {"expect_forward": _timed(expect_forward, steps, warmup), "expect_forward_backward": _timed(expect_step, steps, warmup),
          "loss_forward_backward": _timed(loss_step, steps, warmup), "loss_forward": _timed(loss_forward, steps, warmup)}
    prof = {}
    for name, fn in (("expect_forward", expect_forward), ("loss_forward", loss_forward), ("expect_step", expect_step),
                     ("loss_step", loss_step)):
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[name] = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
    dp = lambda p: p.get("alpha_beta", {"ms": 0.0})["ms"]  # noqa: E731
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    return {"workload": workload, "B": B, "T_max": int(T.max()), "S_max": int(S.max()), "V": V, "rows": rows,
            "steps": steps, "warmup": warmup, "expected_mean": round(float(expected.mean()), 4), "median_ms": med,
            "min_ms": {k: round(float(v.min()), 4) for k, v in ms.items()},
            "max_ms": {k: round(float(v.max()), 4) for k, v in ms.items()},
            "expect_recursion_ms": round(dp(prof["expect_forward"]) - dp(prof["loss_forward"]), 4),
            "expect_step_over_loss_step": round(med["expect_forward_backward"] / med["loss_forward_backward"], 4),
            "kernels": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="headline,c2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    for config in args.configs.split(","):
        print(json.dumps(run(config, args.steps, args.warmup), indent=1), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
