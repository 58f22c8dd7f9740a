"""Time monotonic_rnnt_joint_expected_cost (mrnnt_joint_expect_*) next to the joint loss step -- the floor, and what
a regulariser costs over it -- and the route it replaces, in one process.

  python tools/joint_expect_bench.py [--config headline|c2] [--H 512] [--steps 5] [--warmup 2] [--no-unfused]

Latency costs (label_costs = the frame index t, no blank costs). Timed with HIP events, median of --steps after
--warmup:
  the expected-cost forward alone (no gradient: the joint pass, the recursion, A only) and with_grad;
  the step (costs + 0.01 * expected).sum().backward() through autograd, default and capturable;
  one such step stage by stage -- forward (row list, joint pass, alpha / beta, expectation recursion), rows (the
      coefficient launch, the expect-live list), gradient pass, dweight GEMM, dH GEMM, reduce -- the coefficient launch
      with its algorithmic bytes (what one in-band row reads and writes) and the rate that makes, the library's
      per-kernel profile of the same step beside it, and the expect-live row count against the loss's live rows;
  (a) the monotonic_rnnt_joint_loss step;
  (b) the materialised bf16 logits followed by monotonic_rnnt_expected_cost.
Prints one JSON object.
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

LAMBDA = 0.01
# one in-band row of the coefficient launch: alpha(t-1), three beta, lp (two fp64), A, two Bk, one fp32 cost read
# (neighbouring rows share cache lines: beta / Bk of frame t+1 are read by two rows each); Wb, We written
COEF_ROW_BYTES = {"read": 8 * 9 + 4, "write": 16}


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


def _stat(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="headline")
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-unfused", action="store_true", help="skip (b), the materialised logits")
    a = ap.parse_args()
    import _mrnnt_lib as L
    import monotonic_rnnt_joint as J
    import monotonic_rnnt_op as op
    from bench import lengths_for

    dev = torch.device("cuda:0")
    Tn, Sn, V, workload = lengths_for(a.config, 0, 1)[:4]
    B, T, S, H = len(Tn), int(Tn.max()), int(Sn.max()), a.H
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(B, T, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    pred = torch.randn(B, S + 1, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    W = (torch.randn(V, H, device=dev, generator=g) * (2.0 / H ** 0.5)).to(torch.bfloat16).requires_grad_(True)
    bias = (0.1 * torch.randn(V, device=dev, generator=g)).requires_grad_(True)
    leaves = (enc, pred, W, bias)
    labels = torch.from_numpy(np.random.default_rng(1).integers(1, V, (B, S)).astype(np.int32)).to(dev)
    Tl, Sl = torch.from_numpy(Tn), torch.from_numpy(Sn)
    we = torch.arange(T, dtype=torch.float32, device=dev).view(1, T, 1).expand(B, T, S + 1).contiguous()  # latency

    def clear():
        for x in leaves:
            x.grad = None

    def expect_forward():
        with torch.no_grad():
            return J.monotonic_rnnt_joint_expected_cost(enc, pred, W, bias, labels, Tl, Sl, None, we)

    def expect_step(capturable):
        clear()
        e, c = J.monotonic_rnnt_joint_expected_cost(enc, pred, W, bias, labels, Tl, Sl, None, we, capturable=capturable)
        (c + LAMBDA * e).sum().backward()
        return e, c

    def loss_step():
        clear()
        J.monotonic_rnnt_joint_loss(enc, pred, W, bias, labels, Tl, Sl).sum().backward()

    def materialised():
        clear()
        h = torch.tanh(enc[:, :, None, :] + pred[:, None, :, :])
        z = torch.nn.functional.linear(h, W, bias.to(torch.bfloat16))  # [B, T, S + 1, V] bf16
        e, c = op.monotonic_rnnt_expected_cost(z, labels, Tl, Sl, None, we)
        (c + LAMBDA * e).sum().backward()

    e, c = expect_step(False)
    torch.cuda.synchronize()
    # the value: the posteriors-weighted cost of the same inputs; the costs: the loss's bits
    with torch.no_grad():
        post = J.monotonic_rnnt_joint_posteriors(enc, pred, W, bias, labels, Tl, Sl)
        ref = (post.label.double() * we.double()).sum((1, 2)).cpu().numpy()
        assert torch.equal(c.detach(), J.monotonic_rnnt_joint_loss(enc, pred, W, bias, labels, Tl, Sl))
    del post
    got = e.detach().cpu().double().numpy()
    bound = np.array([float(np.arange(int(t)).sum()) for t in Tn])
    assert np.all(np.abs(got - ref) <= 1e-4 + 4e-6 * bound), float(np.abs(got - ref).max())

    rows = int(np.sum(Tn.astype(np.int64) * (Sn + 1)))
    out = {"workload": workload, "B": B, "T": T, "S": S, "V": V, "H": H, "steps": a.steps, "warmup": a.warmup,
           "lattice_rows": rows, "lambda": LAMBDA, "expected_mean": round(float(got.mean()), 4)}
    out["expect_forward_no_grad"] = _stat(_timed(expect_forward, a.steps, a.warmup))
    out["expect_step"] = _stat(_timed(lambda: expect_step(False), a.steps, a.warmup))
    out["expect_step_capturable"] = _stat(_timed(lambda: expect_step(True), a.steps, a.warmup))
    out["a_joint_loss_step"] = _stat(_timed(loss_step, a.steps, a.warmup))

    # one step stage by stage (the autograd Function's own calls), HIP events around each stage
    prep = J._JointPrepared(enc.detach(), pred.detach(), W.detach(), bias.detach(), labels, Tl, Sl, 0)
    wt = W.detach().t().contiguous().t()
    gc = torch.ones(B, dtype=torch.float32, device=dev)
    ge = torch.full((B,), LAMBDA, dtype=torch.float32, device=dev)
    box = {}

    def stages():
        m = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        m[0].record()
        _, _, ws = prep.expect_forward(None, we, T, S + 1, True)
        m[1].record()
        cnt = prep.expect_rows(ws, None, we, T, S + 1, ge, gc)
        m[2].record()
        db = torch.zeros(V, dtype=torch.float32, device=dev) if J._dbias_in_pass(H, V) else None
        # (the binding's call lists the rows again before its gradient pass: rows_ms is taken off below)
        G, Hact = prep.expect_backward_rows(ws, None, we, T, S + 1, ge, gc, dbias=db)
        m[3].record()
        J._split_k_weight_grad(G, Hact)
        m[4].record()
        dH = G @ wt
        m[5].record()
        prep.reduce(ws, dH, Hact, True, True, scratch=G)
        m[6].record()
        box["rows"], box["cnt"] = G.shape[0], cnt
        return m

    for _ in range(a.warmup):
        stages()
    runs = []
    for _ in range(a.steps):
        m = stages()
        torch.cuda.synchronize()
        runs.append([m[i].elapsed_time(m[i + 1]) for i in range(6)])
    med = np.median(np.array(runs), axis=0)
    prof = {}
    for name, fn in (("expect_step", lambda: expect_step(False)), ("joint_loss_step", loss_step)):
        L.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        prof[name] = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in L.profile_read().items() if v[1]}
        L.profile_enable(False)
    # the coefficient launch alone: the library's alpha_beta slot around mrnnt_joint_expect_rows
    _, _, ws = prep.expect_forward(None, we, T, S + 1, True)
    coef = []
    for _ in range(a.warmup + a.steps):
        L.profile_enable(True)
        prep.expect_rows(ws, None, we, T, S + 1, ge, gc)
        torch.cuda.synchronize()
        coef.append(L.profile_read()["alpha_beta"][0])
        L.profile_enable(False)
    coef_ms = float(np.median(coef[a.warmup:]))
    nb = ctypes.c_int64(0)
    L.check(L.load().mrnnt_joint_row_bound(ctypes.byref(prep.problem), ctypes.byref(nb)), "joint_row_bound")
    coef_bytes = nb.value * (COEF_ROW_BYTES["read"] + COEF_ROW_BYTES["write"])
    live = torch.zeros(1, dtype=torch.int64, device=dev)
    _, lws = prep.forward(with_beta=True)
    L.check(L.load().mrnnt_joint_live_rows(ctypes.byref(prep.problem), ctypes.c_void_p(lws.data_ptr()),
                                           ctypes.c_void_p(live.data_ptr()), prep.stream()), "mrnnt_joint_live_rows")
    out["stages"] = {
        "forward_ms": round(float(med[0]), 4), "rows_ms": round(float(med[1]), 4),
        "coefficient_launch_ms": round(coef_ms, 4), "row_list_ms": round(float(med[1]) - coef_ms, 4),
        "gradient_pass_ms": round(float(med[2] - med[1]), 4), "dweight_ms": round(float(med[3]), 4),
        "dH_ms": round(float(med[4]), 4), "reduce_ms": round(float(med[5]), 4),
        "coefficient_algorithmic_bytes": coef_bytes,
        "coefficient_gb_per_s": round(coef_bytes / (coef_ms * 1e-3) / 1e9, 1),
        "library_profile": prof}
    out["expect_live_rows"] = int(box["cnt"].item())
    out["loss_live_rows"] = int(live.item())
    out["in_band_rows"] = nb.value
    if not a.no_unfused:
        del lws, ws
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        out["b_materialised_logits_expected_cost"] = _stat(_timed(materialised, a.steps, a.warmup))
        out["b_peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
    base = out["expect_step"]["median_ms"]
    out["expect_step_over_loss_step"] = round(base / out["a_joint_loss_step"]["median_ms"], 4)
    out["capturable_over_default"] = round(out["expect_step_capturable"]["median_ms"] / base, 4)
    if not a.no_unfused:
        out["b_over_expect_step"] = round(out["b_materialised_logits_expected_cost"]["median_ms"] / base, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
