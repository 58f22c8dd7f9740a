"""Time monotonic_rnnt_hat_loss (mrnnt_hat_forward / mrnnt_hat_backward) next to the monotonic_rnnt_loss step of the
same process, and next to the PyTorch composition a user would write without it (transform the logits, then
monotonic_rnnt_loss).

  python tools/hat_bench.py [--config headline] [--rounds 5] [--steps 3] [--warmup 2] [--comp-batch 16]

Device-resident lengths, fp32 synthetic logits, the product library, blank 0. Each step is forward + backward through
the autograd surface, timed with HIP events. The three steps run alternately, round after round (loss, factorised,
composition, loss, ...), so drift of the device shows up inside every series alike; the spread of a series is the
range of its rounds' medians. The composition holds several more N x V tensors than the two library steps: it is timed
at the configured shape only where the free memory covers them, and always at the first --comp-batch utterances of it
together with the two library steps (the ratio of record). A last pass with the library's per-kernel profile gives the
launches' own times. Two counts say how many rows either gradient pass had to read and write -- the two distributions
spread their paths over different numbers of rows (on N(0,1) logits a factorised blank has probability 1/2, a softmax
blank 1/V): the rows of the gradient that are not all zero, and mrnnt_grad_live_rows on the state of either forward
(the standard loss's rule, LossRows::alive: occupancy >= e^-110 and not flush-dead, i.e. not every fp32 exponential of
the row zero -- mrnnt_host.h kFlushLog2; it is evaluated on whatever den the forward left, so after the factorised
forward the count is that predicate on den', not HatRows' own). Prints one JSON object.
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

COMP_TENSORS = 6.5  # N x V tensors alive at the composition's peak (acts, a', both gradients, autograd temporaries)


def transform(z):
    """a' of monotonic_rnnt_hat_loss for blank 0, as a user composes it from torch ops."""
    F = torch.nn.functional
    zb = z[:, 0]
    lse = torch.logsumexp(z[:, 1:], dim=1)
    lab = z[:, 1:] + (F.logsigmoid(-zb) - lse).unsqueeze(1)
    return torch.cat([F.logsigmoid(zb).unsqueeze(1), lab], dim=1)


def _time(fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def run_shape(T, S, V, rounds, steps, warmup, comp):
    import _mrnnt_lib as L
    import monotonic_rnnt_op as op

    dev = torch.device("cuda:0")
    B = len(T)
    rows = int(np.sum(T.astype(np.int64) * (S + 1)))
    acts = torch.empty((rows, V), dtype=torch.float32, device=dev)
    L.synth_acts(acts.data_ptr(), 0, rows * V, 0, True, torch.cuda.current_stream().cuda_stream)
    acts.requires_grad_(True)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, int(S.max()))).astype(np.int32)).to(dev)
    Td, Sd = torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)

    def loss_step():
        acts.grad = None
        op.monotonic_rnnt_loss(acts, labels, Td, Sd).sum().backward()

    def hat_step():
        acts.grad = None
        op.monotonic_rnnt_hat_loss(acts, labels, Td, Sd).sum().backward()

    def comp_step():
        acts.grad = None
        op.monotonic_rnnt_loss(transform(acts), labels, Td, Sd).sum().backward()

    fns = {"loss": loss_step, "hat": hat_step}
    note = None
    if comp:
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        need = (COMP_TENSORS - 1) * acts.numel() * 4
        if free >= need:
            fns["composition"] = comp_step
        else:
            note = (f"composition not run at this shape: it needs about {need / 2**30:.0f} GiB beside the logits, "
                    f"{free / 2**30:.0f} GiB are free")
    # the composition computes the same costs (the check that the three steps are one computation)
    c_hat = op.monotonic_rnnt_hat_loss(acts.detach(), labels, Td, Sd)
    c_loss = op.monotonic_rnnt_loss(acts.detach(), labels, Td, Sd)
    if "composition" in fns:
        c_comp = op.monotonic_rnnt_loss(transform(acts.detach()), labels, Td, Sd)
        err = float(((c_hat - c_comp).abs() / c_comp.abs().clamp(min=1.0)).max())
        assert err <= 1e-4, err
        del c_comp
    torch.cuda.synchronize()
    op.check_lengths()
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(_time(fn, steps))
    prof = {}
    for k, fn in fns.items():
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[k] = {n: {"ms": round(v[0], 4), "launches": v[1]} for n, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
    # rows of the gradient that are not all zero: what either gradient pass had to read and write
    nonzero = {}
    for k in ("loss", "hat"):
        fns[k]()
        g, n = acts.grad, 0
        for i in range(0, rows, 1 << 20):
            n += int((g[i:i + (1 << 20)] != 0).any(dim=1).sum())
        nonzero[k] = n
    acts.grad = None
    live = {}
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    for k in ("loss", "hat"):
        prep = op._Prepared(acts.detach(), labels, Td, Sd, None, 0, 0)
        _, ws = op._forward(prep, with_beta=True, hat=k == "hat")
        L.check(L.load().mrnnt_grad_live_rows(ctypes.byref(prep.problem), ctypes.c_void_p(ws.data_ptr()),
                                              ctypes.c_void_p(count.data_ptr()), prep.stream()), "mrnnt_grad_live_rows")
        live[k] = int(count.item())
        del ws, prep
    out = {"B": B, "T_max": int(T.max()), "S_max": int(S.max()), "V": V, "rows": rows,
           "acts_GiB": round(rows * V * 4 / 2**30, 2), "rounds": rounds, "steps_per_round": steps, "warmup": warmup,
           "cost_mean": {"loss": round(float(c_loss.mean()), 3), "hat": round(float(c_hat.mean()), 3)}}
    for k, v in ms.items():
        med = [float(np.median(r)) for r in v]
        out[k] = {"median_ms": round(float(np.median(np.concatenate([np.asarray(r) for r in v]))), 4),
                  "round_medians_ms": [round(x, 4) for x in med], "spread_ms": round(max(med) - min(med), 4),
                  "min_ms": round(float(min(min(r) for r in v)), 4)}
    out["live_rows"] = live
    out["nonzero_grad_rows"] = nonzero
    out["hat_over_loss"] = round(out["hat"]["median_ms"] / out["loss"]["median_ms"], 4)
    if "composition" in out:
        out["composition_over_hat"] = round(out["composition"]["median_ms"] / out["hat"]["median_ms"], 3)
    if note:
        out["note"] = note
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
    ap.add_argument("--comp-batch", type=int, default=16)
    args = ap.parse_args()
    import _mrnnt_lib as L
    from bench import lengths_for
    T, S, V, workload = lengths_for(args.config, 0, 1)[:4]
    res = {"workload": workload, "library_sha256": L.library_sha256(), "device": torch.cuda.get_device_name(0)}
    res["full"] = run_shape(T, S, V, args.rounds, args.steps, args.warmup, comp=True)
    n = min(args.comp_batch, len(T))
    if "composition" not in res["full"] and n > 0:
        res[f"first_{n}"] = run_shape(T[:n], S[:n], V, args.rounds, args.steps, args.warmup, comp=True)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
