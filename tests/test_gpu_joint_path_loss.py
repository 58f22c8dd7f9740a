"""monotonic_rnnt_joint_path_loss (mrnnt_joint_path_*: mrnnt_joint.hip with the path coefficients, mrnnt_path.hip's walk /
hull / score / coef launches) against the yardstick of tests/_joint_path_checks.py -- the fp64 composition the fused op
replaces, from the same bf16 inputs -- and against the library's own read-outs and unfused twin.

Tolerances (tests/test_gpu_joint.py's, for this arithmetic): costs within 1e-5 max(1, |c|); each gradient tensor within
1.5e-2 max|ref| + 1e-5. Where a result must not change at all, the comparison is bitwise.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _joint_path_checks as JC
import _path_checks as PC

pytestmark = pytest.mark.gpu

NAMES = ("d_enc", "d_pred", "d_weight", "d_bias")
# mixed signs without wholesale cancellation
WEIGHTS = np.array([1.0, -0.5, 2.0, 0.75, -1.5, 0.5, 1.25, -0.25, 1.0], np.float32)
# ragged, T <= 130, S <= 40: T = 1 with S = 0, S = T, T = 65 (one frame past a 64-frame block), and T = 130, where 9
# paths stand on more than 256 rows (the backward's workgroup)
SHAPES = {"t130": [(130, 40), (1, 0), (33, 33)], "t65": [(65, 23), (1, 0), (40, 40)]}


@pytest.fixture(scope="module")
def jm():
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def parity_case(H, V, shapes):
    """Inputs and their host logits, computed once per (H, V, shapes) and shared by the K = 1 and K = 9 cases."""
    blank = V - 1 if (H, V) == (256, 100) else 0
    case = JC.make_case(H + V + len(shapes), SHAPES[shapes], H, V, blank)
    enc, pred, w, bias, labels, T, S = case
    if (H, V) == (128, 64):
        bias = None
    return (enc, pred, w, bias, labels, T, S), blank, JC.joint_logits(enc, pred, w, bias, T, S)


def on(dev, enc, pred, w, bias, labels, T, S):
    return (enc.to(dev), pred.to(dev), w.to(dev), None if bias is None else bias.to(dev),
            torch.from_numpy(labels).to(dev), torch.from_numpy(T), torch.from_numpy(S))


def make_paths(jm, dev, case, K, blank=0, seed=5):
    """int32 [B, K, max T] (numpy): joint_align's path, the two extreme paths, then joint_sample's draws."""
    enc, pred, w, bias, labels, T, S = case
    args = on(dev, *case)
    L = int(T.max())
    al, _ = jm.monotonic_rnnt_joint_align(*args, blank_label=blank)
    parts = [al.cpu().numpy()[:, None, :]]
    if K > 1:
        parts.append(JC.extreme_paths(labels, T, S, L, blank))
    if K > 3:
        parts.append(jm.monotonic_rnnt_joint_sample(*args, num_samples=K - 3, seed=seed,
                                                    blank_label=blank).alignments.cpu().numpy())
    out = np.ascontiguousarray(np.concatenate(parts, axis=1)[:, :K]).astype(np.int32)
    assert out.shape == (len(T), K, L)
    return out


def run(jm, dev, case, al, wts=None, blank=0, capturable=None):
    """(path costs fp64 numpy [B, K], d_enc, d_pred, d_weight, d_bias or None) of one forward + backward."""
    enc, pred, w, bias, lab, T, S = on(dev, *case)
    leaves = [x.requires_grad_(True) for x in (enc, pred, w)] + ([] if bias is None else [bias.requires_grad_(True)])
    pc = jm.monotonic_rnnt_joint_path_loss(enc, pred, w, bias, lab, T, S, torch.from_numpy(al).to(dev),
                                           blank_label=blank, capturable=capturable)
    assert pc.dtype == torch.float32 and tuple(pc.shape) == tuple(al.shape[:2]) and pc.requires_grad
    up = torch.ones_like(pc) if wts is None else torch.from_numpy(np.asarray(wts, np.float32)).to(dev)
    pc.backward(up)
    torch.cuda.synchronize()
    grads = [x.grad for x in leaves] + ([None] if bias is None else [])
    for x, like in zip(grads, (enc, pred, w, bias)):
        assert x is None or (x.dtype == like.dtype and x.shape == like.shape)
    return (pc.detach().cpu().double().numpy(),) + tuple(grads)


def check_vs_yardstick(got, ref, T, S):
    JC.assert_costs(got[0], ref[0])
    for x, r, name in zip(got[1:], ref[1:], NAMES):
        if x is not None:
            JC.close(x, r, name)
    de, dp = got[1], got[2]
    for b in range(len(T)):  # padding frames / label slots: exactly zero
        assert torch.all(de[b, T[b]:] == 0) and torch.all(dp[b, S[b] + 1:] == 0)


def same_bits(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True)
    for x, y, name in zip(a[1:], b[1:], NAMES):
        assert (x is None and y is None) or torch.equal(x, y), name


def weights(B, K):
    return np.ascontiguousarray(np.outer([1.0, -2.0, 0.5, 1.5][:B], WEIGHTS[:K])).astype(np.float32)


# 1. parity: both MFMA tiles (H <= 512 / H = 640), V % 4 != 0, blank = V - 1 at (256, 100), no bias at (128, 64)
@pytest.mark.parametrize("K", [1, 9])
@pytest.mark.parametrize("shapes", ["t130", "t65"])
@pytest.mark.parametrize("H,V", [(128, 64), (256, 100), (256, 1000), (512, 256), (384, 96), (640, 130)])
def test_parity_vs_yardstick(jm, dev, H, V, shapes, K):
    case, blank, logits = parity_case(H, V, shapes)
    enc, pred, w, bias, labels, T, S = case
    al = make_paths(jm, dev, case, K, blank)
    wts = weights(len(T), K)
    got = run(jm, dev, case, al, wts, blank)
    ref = JC.yardstick(enc, pred, w, bias, labels, T, S, al, wts, blank, logits=logits)
    assert np.all(np.isfinite(ref[0]))
    check_vs_yardstick(got, ref, T, S)
    if K == 9 and shapes == "t130":  # the row list crosses the backward's 256-row workgroup
        rows = {(b, t, s) for b in range(len(T)) for k in range(K)
                for t, s in zip(*np.divmod(PC.walk(al[b, k], labels[b], int(T[b]), int(S[b]), blank)[0], int(S[b]) + 1))}
        assert len(rows) > 256


# 2. consistency with the read-outs
def test_consistent_with_align_sample_and_the_restricted_loss(jm, dev):
    case = JC.make_case(24, [(23, 9), (17, 17), (12, 0), (30, 4)], 256, 64)
    enc, pred, w, bias, labels, T, S = case
    args = on(dev, *case)
    al, c = jm.monotonic_rnnt_joint_align(*args)
    c = c.cpu().double().numpy()
    got = run(jm, dev, case, np.ascontiguousarray(al.cpu().numpy()[:, None, :]))
    assert np.all(np.abs(got[0][:, 0] - c) <= PC.ULP * np.abs(c)), (got[0][:, 0], c)
    smp = jm.monotonic_rnnt_joint_sample(*args, num_samples=9, seed=5)
    pcs = smp.path_costs.cpu().double().numpy()
    pc = jm.monotonic_rnnt_joint_path_loss(*args, smp.alignments).cpu().double().numpy()
    assert np.all(np.abs(pc - pcs) <= PC.ULP * np.abs(pcs)), (pc, pcs)
    # K = 1: the four gradients are those of the loss restricted to the path itself
    leaves = [x.clone().requires_grad_(True) for x in args[:4]]
    jm.monotonic_rnnt_joint_loss(*leaves, *args[4:], alignment=al, max_distance_from_alignment=0).sum().backward()
    torch.cuda.synchronize()
    for x, leaf, name in zip(got[1:], leaves, NAMES):
        JC.close(x, leaf.grad.double().cpu(), name)


# 3. against the materialised route
def test_matches_path_loss_on_materialised_logits(jm, dev):
    import monotonic_rnnt_op as op
    H, V = 256, 256
    case = JC.make_case(11, [(40, 12), (5, 3), (17, 0), (12, 12)], H, V)
    enc, pred, w, bias, labels, T, S = case
    al = make_paths(jm, dev, case, 6)
    args = on(dev, *case)
    c_fused = jm.monotonic_rnnt_joint_path_loss(*args, torch.from_numpy(al).to(dev)).cpu().double().numpy()
    rows = []
    for b in range(len(T)):
        e = enc[b, : T[b]].to(dev).float()
        p = pred[b, : S[b] + 1].to(dev).float()
        h = torch.tanh(e[:, None] + p[None]).to(torch.bfloat16).float()
        rows.append((h @ w.to(dev).float().T + bias.to(dev)).reshape(-1, V))
    acts = torch.cat(rows).contiguous()
    c_acts = op.monotonic_rnnt_path_loss(acts, args[4], args[5], args[6],
                                         torch.from_numpy(al).to(dev)).cpu().double().numpy()
    assert np.all(np.abs(c_fused - c_acts) <= 1e-3 * np.maximum(1.0, np.abs(c_acts))), (c_fused, c_acts)


# 4. invalid rows
def test_invalid_rows_cost_inf_and_change_nothing_else(jm, dev):
    case = JC.make_case(21, [(23, 9), (17, 17), (12, 0), (30, 4)], 128, 64)
    enc, pred, w, bias, labels, T, S = case
    K = 6
    al = make_paths(jm, dev, case, K)
    wts = weights(len(T), K)
    keep = [k for k in range(K) if k != 2]
    ref = run(jm, dev, case, np.ascontiguousarray(al[:, keep]), np.ascontiguousarray(wts[:, keep]))
    spoiled = PC.invalid_rows(al, labels, T, S, 0, 2)
    assert "minus_one" in spoiled
    for name, row in spoiled.items():
        assert PC.walk(row, labels[0], int(T[0]), int(S[0])) is None, name
        bad = al.copy()
        bad[0, 2] = row
        bad[1:, 2] = -1  # the -1 sentinel row in the other utterances (T = S and S = 0 among them)
        got = run(jm, dev, case, bad, wts)
        assert np.all(got[0][:, 2] == np.inf), name
        assert got[0][:, keep].tobytes() == ref[0].tobytes(), name
        for x, y, g in zip(got[1:], ref[1:], NAMES):
            assert torch.equal(x, y), (name, g)
    check_vs_yardstick(got, JC.yardstick(enc, pred, w, bias, labels, T, S, bad, wts), T, S)
    only = al.copy()
    only[1] = -1                   # utterance 1 (T = S): nothing but invalid rows
    only[2, :, 0] = labels[2, 0]   # utterance 2 (S = 0): a label where none fits
    got = run(jm, dev, case, only, wts)
    assert np.all(got[0][1] == np.inf) and np.all(got[0][2] == np.inf)
    for b in (1, 2):
        assert torch.all(got[1][b] == 0) and torch.all(got[2][b] == 0)
    check_vs_yardstick(got, JC.yardstick(enc, pred, w, bias, labels, T, S, only, wts), T, S)


def live_rows(jm, dev, case, al, wts):
    """The path-live row count of mrnnt_joint_path_rows after a forward on the same paths."""
    enc, pred, w, bias, lab, T, S = on(dev, *case)
    prep = jm._JointPrepared(enc, pred, w, bias, lab, T, S, 0)
    ald = torch.from_numpy(al).to(dev)
    _, ws = prep.path_forward(ald)
    n = int(prep.path_rows(ws, ald, torch.from_numpy(np.asarray(wts, np.float32)).to(dev)).item())
    assert 0 <= n <= prep.path_row_bound(al.shape[1])
    return n


# 5. signed weights
def test_signed_weights(jm, dev):
    case = JC.make_case(22, [(12, 5), (9, 9), (6, 0)], 256, 100)
    enc, pred, w, bias, labels, T, S = case
    B, L = len(T), int(T.max())
    ex = JC.extreme_paths(labels, T, S, L)
    # two identical paths, weights (+1, -1): Wb = We = 0 on every row, exactly
    twin = np.ascontiguousarray(np.repeat(ex[:, :1], 2, axis=1))
    pm = np.tile(np.array([[1.0, -1.0]], np.float32), (B, 1))
    got = run(jm, dev, case, twin, pm)
    assert np.all(got[0][:, 0] == got[0][:, 1])
    for x, name in zip(got[1:], NAMES):
        assert torch.all(x == 0), name
    assert live_rows(jm, dev, case, twin, pm) == 0
    # all-zero weights: an empty row list, exactly zero gradients
    zero = np.zeros((B, 2), np.float32)
    got = run(jm, dev, case, ex, zero)
    for x, name in zip(got[1:], NAMES):
        assert torch.all(x == 0), name
    assert live_rows(jm, dev, case, ex, zero) == 0
    assert live_rows(jm, dev, case, ex, np.ones((B, 2), np.float32)) > 0
    # (+a, -a) on the two extreme paths: where they leave a row by different arcs (row (0, 0) of utterance 0, with
    # 0 < S < T) wocc = 0 and the two corrections stay
    assert 0 < S[0] < T[0]
    pa = np.tile(np.array([[0.75, -0.75]], np.float32), (B, 1))
    got = run(jm, dev, case, ex, pa)
    ref = JC.yardstick(enc, pred, w, bias, labels, T, S, ex, pa)
    assert all(float(r.abs().max()) > 1e-3 for r in ref[1:])  # (something to compare: utterance 0 does not cancel)
    check_vs_yardstick(got, ref, T, S)


# 6. masked bias
def test_masked_bias(jm, dev):
    """bias = -inf on a label only utterance 0 emits (every path of an utterance emits all its labels): its paths cost
    +inf, nothing else does; every gradient stays finite and within tolerance (the masked entry's softmax term is
    e^-inf = 0, its correction -We stays), also with an ordinary masked entry nobody emits."""
    H, V = 256, 130
    case = JC.make_case(H + V + 9, [(20, 6), (14, 3), (9, 0)], H, V)
    enc, pred, w, bias, labels, T, S = case
    v = int(labels[0, 2])
    labels[1] = np.where(labels[1] == v, v % (V - 2) + 1, labels[1])
    assert v not in labels[1, : S[1]] and v in labels[0, : S[0]]
    other = next(u for u in range(1, V) if u not in set(labels.reshape(-1).tolist()))
    bias = bias.clone()
    bias[v] = bias[other] = -float("inf")
    case = (enc, pred, w, bias, labels, T, S)
    clean = (enc, pred, w, case[3].clone().index_fill_(0, torch.tensor([v]), 0.0), labels, T, S)
    al = make_paths(jm, dev, clean, 3)  # (paths from the model with label v unmasked: every path is a path still)
    wts = weights(len(T), 3)
    got = run(jm, dev, case, al, wts)
    ref = JC.yardstick(enc, pred, w, bias, labels, T, S, al, wts)
    assert np.all(ref[0][0] == np.inf) and np.all(np.isfinite(ref[0][1:]))  # the reference itself
    assert np.all(got[0][0] == np.inf) and np.all(np.isfinite(got[0][1:]))
    for x, r, name in zip(got[1:], ref[1:], NAMES):
        assert torch.isfinite(x).all() and torch.isfinite(r).all(), name
    check_vs_yardstick(got, ref, T, S)
    assert got[4][other] == 0 and torch.all(got[3][other] == 0)


# 7. bitwise reproducibility
@pytest.mark.parametrize("H,V", [(128, 64), (512, 256), (640, 130)])
def test_bitwise_reproducible(jm, dev, H, V):
    case = JC.make_case(26 + H, [(70, 20), (33, 33), (12, 0)], H, V)
    al = make_paths(jm, dev, case, 9)
    wts = weights(3, 9)
    same_bits(run(jm, dev, case, al, wts), run(jm, dev, case, al, wts))


# 8. capturable
def _step(jm, leaves, lab, T, S, al, up, capturable):
    for x in leaves:
        x.grad = None
    pc = jm.monotonic_rnnt_joint_path_loss(*leaves, lab, T, S, al, capturable=capturable)
    pc.backward(up)
    return (pc.detach().clone(),) + tuple(x.grad.clone() for x in leaves)


@pytest.mark.parametrize("H,V", [(256, 128), (640, 130)])
def test_capturable_and_graph_capture_replay(jm, dev, H, V):
    case = JC.make_case(31 + H, [(50, 12), (20, 20), (33, 0), (41, 7)], H, V)
    al = torch.from_numpy(make_paths(jm, dev, case, 5)).to(dev)
    up = torch.from_numpy(weights(4, 5)).to(dev)
    enc, pred, w, bias, lab, T, S = on(dev, *case)
    leaves = [x.requires_grad_(True) for x in (enc, pred, w, bias)]
    eager_cap = _step(jm, leaves, lab, T, S, al, up, True)
    eager = _step(jm, leaves, lab, T, S, al, up, False)
    assert torch.equal(eager_cap[0], eager[0])
    for a, b, name in zip(eager_cap[1:], eager[1:], NAMES):
        JC.close(a, b.double().cpu(), name)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any device-to-host read in the capturable step raises
    try:
        _step(jm, leaves, lab, T, S, al, up, True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    # capture (warm-up on a side stream first, as torch.cuda.graph asks), then replay on new inputs
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _step(jm, leaves, lab, T, S, al, up, None)
    torch.cuda.current_stream().wait_stream(s)
    for x in leaves:
        x.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pc = jm.monotonic_rnnt_joint_path_loss(*leaves, lab, T, S, al)  # capturable inside capture
        pc.backward(up)
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(2):
        with torch.no_grad():
            leaves[0].copy_(torch.randn(enc.shape, device=dev, generator=gen).to(enc.dtype))
            leaves[1].copy_(torch.randn(pred.shape, device=dev, generator=gen).to(pred.dtype))
        g.replay()
        torch.cuda.synchronize()
        got = (pc.detach().clone(),) + tuple(x.grad.clone() for x in leaves)
        fresh = [x.detach().clone().requires_grad_(True) for x in leaves]
        ref = _step(jm, fresh, lab, T, S, al, up, True)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


# 9. the clamp of the device count by the host bound
@pytest.mark.parametrize("H", [256, 640])
def test_backward_never_writes_past_the_host_bound(jm, dev, H):
    """mrnnt_joint_path_backward with live_count_dev set and n_rows SMALLER than the device count: the count is clamped
    to the bound, so nothing at or past row n_rows changes. (G / Hact are allocated for the whole count: no access is
    out of bounds either way.)"""
    import _mrnnt_lib as L
    V = 64
    case = JC.make_case(40 + H, [(130, 40), (100, 20)], H, V)
    enc, pred, w, bias, lab, T, S = on(dev, *case)
    al = torch.from_numpy(make_paths(jm, dev, case, 9)).to(dev)
    prep = jm._JointPrepared(enc, pred, w, bias, lab, T, S, 0)
    _, ws = prep.path_forward(al)
    cnt = prep.path_rows(ws, al, None)
    count = int(cnt.item())
    n_rows = 100
    assert count > 256 + n_rows  # more than one workgroup's rows lie past the bound
    canary = 0x7B7B  # a finite bf16 pattern
    G = torch.full((count, V), canary, dtype=torch.int16, device=dev)
    Hact = torch.full((count, H), canary, dtype=torch.int16, device=dev)
    prep.problem.live_count_dev = cnt.data_ptr()
    prep.problem.hact_ld = H
    prep.problem.dbias = None
    L.check(L.load().mrnnt_joint_path_backward(ctypes.byref(prep.problem), ctypes.c_void_p(ws.data_ptr()), n_rows,
                                               ctypes.c_void_p(G.data_ptr()), ctypes.c_void_p(Hact.data_ptr()), None,
                                               None, prep.stream()), "mrnnt_joint_path_backward")
    torch.cuda.synchronize()
    assert torch.all(G[n_rows:] == canary) and torch.all(Hact[n_rows:] == canary)
    assert not torch.all(G[:n_rows] == canary) and not torch.all(Hact[:n_rows] == canary)  # (the pass did run)
