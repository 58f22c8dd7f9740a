"""The factorised-blank (HAT) loss under the fused joint on the GPU (monotonic_rnnt_joint_hat_loss, mrnnt_joint_hat_*),
against the host reference of tests/_joint_hat_checks.py: the fp64 joint logits of the bf16 operands, transformed
(_hat_checks.hat_transform), through the oracle and back.

Shapes: B = 3, T <= 24, S <= 8, one S = 0 utterance, grad_scale = [1, -0.5, 2]. Tolerances are the joint's own
(tests/test_gpu_joint.py): costs 1e-5 max(1, |c|), gradients 1.5e-2 max |ref| + 1e-5 per tensor.

(H, V): (128, 64) the ones-column dbias; (256, 100) / (384, 96) / (512, 256) / (256, 1000) the in-pass dbias of the
16x16x32 gradient kernel; (640, 130) the 32x32x16 gradient kernel; V = 100 / 130 / 1000 a partial last chunk, V = 130
not a multiple of 4 (scalar stores). Blank: 0, V - 1, 21 (inside a chunk, in the upper lane half of the 32x32 tile /
lane group 1 of the 16x16 one), and an index in the partial last chunk where V has one.

The "sum everything, subtract exp(z_b)" mutant of the forward fails the dominant-blank cases of this file:
profiles/joint_hat/subtract_the_blank_mutant.txt."""
import numpy as np
import pytest
import torch

import _joint_hat_checks as JH
import _joint_lattice_cases as C
from _parity import knobs

pytestmark = pytest.mark.gpu

SHAPES = [(128, 64), (256, 100), (384, 96), (512, 256), (640, 130), (256, 1000)]


def blanks(V):
    out = [0, V - 1, 21]
    if V % 32 and (V // 32) * 32 + 1 < V - 1:
        out.append((V // 32) * 32 + (V % 32) // 2)  # inside the partial last chunk, not V - 1
    elif V % 32:
        out.append((V // 32) * 32)  # the chunk's first entry (V = 130: 128)
    return out


PARITY = [(H, V, b) for H, V in SHAPES for b in blanks(V)]


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("H,V,blank", PARITY)
def test_parity(J, dev, H, V, blank):
    case = JH.hat_case(H + V, H, V, blank)
    enc, pred, w, bias, labels, T, S = case
    assert (S == 0).any() and (S > 0).any()
    ref = JH.host_reference(*case, blank, scale=JH.SCALE, key=("parity", H, V, blank))
    got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
    what = f"H={H} V={V} blank={blank}"
    JH.assert_costs(got[0], ref["costs"], what)
    JH.assert_grads(got, ref, T, S, what)
    JH.assert_blank_dbias(got[4].double().cpu(), ref, blank, what)


@pytest.mark.parametrize("H,V,blank", [(512, 256, 21), (512, 256, 255), (512, 256, 0), (640, 130, 21), (640, 130, 128)])
def test_blank_column_of_dbias(J, dev, H, V, blank):
    """The blank column of d_bias by itself (the in-pass column sums at H = 512 hold sc * gb there through the policy's
    e-dependent correction; H = 640 sums the stored G), on longer utterances than the parity cases: more than one
    workgroup of 256 rows."""
    case = JH.hat_case(3 * H + V + blank, H, V, blank, Trange=(20, 24), Smax=8, B=3)
    ref = JH.host_reference(*case, blank, scale=JH.SCALE, key=("dbias", H, V, blank))
    got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
    JH.assert_costs(got[0], ref["costs"], "dbias")
    JH.assert_blank_dbias(got[4].double().cpu(), ref, blank, f"H={H} V={V} blank={blank}")
    JH.close(got[4], ref["d_b"], name="d_bias")


def _weight_bound(w, bias):
    """max_v (sum_h |W[v, h]| + |bias[v]|) of the bf16 weights, as joint_wbound_kernel forms it (fp64 here)."""
    return float((w.double().abs().sum(1) + bias.double().abs()).max())


def _blank_logit_case(H, V, blank, zb, route):
    """Weights scaled to max_v ||W_v||_1 = 8, bias[blank] = zb, the other biases about -5."""
    enc, pred, w, bias, labels, T, S = JH.hat_case(5 * H + V + blank, H, V, blank)
    l1 = float(w.double().abs().sum(1).max())
    w = (w.float() * (8.0 / l1) * 0.99).to(torch.bfloat16)
    bias = (-5.0 + bias).clone()
    bias[blank] = zb
    bound = _weight_bound(w, bias)
    print(f"    weight bound {bound:.3f}")
    if route == "max":
        assert bound > 64.0, bound  # the running-max epilogue must run
    else:
        assert bound <= 64.0, bound  # the plain exp-sum runs
    return enc, pred, w, bias, labels, T, S


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("route", ["plain", "plain_unscaled", "max"])
@pytest.mark.parametrize("H,V,blank", [(512, 256, 21), (256, 100, 98), (640, 130, 0)])
def test_dominant_and_suppressed_blank(J, dev, H, V, blank, route, sign):
    """bias[blank] = +-55 inside the +-64 weight bound (the plain exp-sum, with the prescaled bias row and -- the
    development build's joint_opt = 1 -- without it) and +-100 outside it (the running max): finite costs within
    tolerance, finite gradients. At z_b = +55 a sum over the whole row minus exp(z_b) cancels to nothing."""
    zb = sign * (100.0 if route == "max" else 55.0)
    case = _blank_logit_case(H, V, blank, zb, route)
    ref = JH.host_reference(*case, blank, scale=JH.SCALE, key=("zb", H, V, blank, zb))
    assert np.all(np.isfinite(ref["costs"]))
    if route == "plain_unscaled":
        with knobs(joint_opt=1):
            got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
    else:
        got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
    JH.assert_costs(got[0], ref["costs"], f"z_b={zb} {route}")
    for x, name in zip(got[1:], ("d_enc", "d_pred", "d_weight", "d_bias")):
        assert torch.isfinite(x).all(), name


def test_matches_the_materialised_acts_path(J, dev):
    """The fused op equals monotonic_rnnt_hat_loss on fp32 logits formed in torch from the same bf16 operands (the
    tolerance of test_gpu_joint.test_joint_matches_materialised_acts_path: 1e-3 relative)."""
    import monotonic_rnnt_op as op
    H, V, blank = 256, 256, 21
    enc, pred, w, bias, labels, T, S = JH.make_case(11, 4, (5, 40), 12, H, V)
    labels = np.where(labels == blank, blank + 1, labels).astype(np.int32)
    c_fused = J.monotonic_rnnt_joint_hat_loss(enc.to(dev), pred.to(dev), w.to(dev), bias.to(dev),
                                              torch.from_numpy(labels).to(dev), torch.from_numpy(T),
                                              torch.from_numpy(S), blank).cpu().double().numpy()
    rows = []
    for b in range(len(T)):
        e = enc[b, : T[b]].to(dev).float()
        p = pred[b, : S[b] + 1].to(dev).float()
        h = torch.tanh(e[:, None] + p[None]).to(torch.bfloat16).float()
        rows.append((h @ w.to(dev).float().T + bias.to(dev)).reshape(-1, V))
    acts = torch.cat(rows).contiguous()
    c_acts = op.monotonic_rnnt_hat_loss(acts, torch.from_numpy(labels).to(dev), torch.from_numpy(T),
                                        torch.from_numpy(S), None, 0, blank).cpu().double().numpy()
    print(f"    fused {c_fused} materialised {c_acts}")
    assert np.all(np.isfinite(c_fused))
    assert np.all(np.abs(c_fused - c_acts) <= 1e-3 * np.maximum(1.0, np.abs(c_acts))), (c_fused, c_acts)


@pytest.mark.parametrize("k", [0, 2])
def test_alignment_restricted(J, dev, k):
    """alignment / max_distance_from_alignment, the alignment from monotonic_rnnt_joint_align(blank_factorized=True)."""
    H, V, blank = 256, 64, 21
    case = JH.hat_case(50 + k, H, V, blank, Trange=(10, 24))
    enc, pred, w, bias, labels, T, S = case
    al, _ = J.monotonic_rnnt_joint_align(enc.to(dev), pred.to(dev), w.to(dev), bias.to(dev),
                                         torch.from_numpy(labels).to(dev), torch.from_numpy(T), torch.from_numpy(S),
                                         blank, blank_factorized=True)
    al = al.cpu().numpy()
    ref = JH.host_reference(*case, blank, scale=JH.SCALE, alignment=al, k=k, key=("aligned", k))
    got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE, alignment=al, k=k)
    JH.assert_costs(got[0], ref["costs"], f"k={k}")
    JH.assert_grads(got, ref, T, S, f"k={k}")


def _non_finite_case():
    H, V, blank = 256, 100, 98
    enc, pred, w, bias, labels, T, S = JH.hat_case(77, H, V, blank, Trange=(6, 24))
    return H, V, blank, enc, pred, w, bias, labels, T, S


def test_non_finite_inputs(J, dev):
    """A NaN in one utterance's enc row: its cost NaN, the others bit-identical to a clean call. bias[label] = -inf:
    +inf. bias[blank] = -inf: +inf where T > S. Every non-blank bias -inf: the S = 0 utterance keeps its finite cost
    -sum_t log sigmoid(z_b), the others +inf."""
    H, V, blank, enc, pred, w, bias, labels, T, S = _non_finite_case()

    def costs(enc_=enc, bias_=bias):
        return J.monotonic_rnnt_joint_hat_loss(enc_.to(dev), pred.to(dev), w.to(dev), bias_.to(dev),
                                               torch.from_numpy(labels).to(dev), torch.from_numpy(T),
                                               torch.from_numpy(S), blank).cpu().numpy()
    clean = costs()
    assert np.all(np.isfinite(clean))
    bad = enc.clone()
    b_nan = int(np.argmax(S > 0))
    bad[b_nan, 0, 3] = float("nan")
    c = costs(enc_=bad)
    assert np.isnan(c[b_nan]), c
    for o in range(len(T)):
        if o != b_nan:
            assert c[o].tobytes() == clean[o].tobytes(), (o, c, clean)
    b_lab = int(np.argmax(S > 0))
    bl = bias.clone()
    bl[int(labels[b_lab, 0])] = -float("inf")
    c = costs(bias_=bl)
    assert c[b_lab] == np.inf, c
    bb = bias.clone()
    bb[blank] = -float("inf")
    c = costs(bias_=bb)
    assert (T > S).any()
    assert np.all(c[T > S] == np.inf), (c, T, S)
    ba = torch.full_like(bias, -float("inf"))
    ba[blank] = bias[blank]
    c = costs(bias_=ba)
    z, _ = JH.joint_logits(enc, pred, w, bias, T, S)
    off = np.concatenate([[0], np.cumsum(T.astype(np.int64) * (S + 1))])
    for b in range(len(T)):
        if S[b] == 0:
            want = -float(torch.nn.functional.logsigmoid(z[off[b]:off[b + 1], blank]).sum())
            print(f"    all labels masked, S = 0 utterance {b}: cost {c[b]} closed form {want}")
            assert np.isfinite(c[b]) and abs(c[b] - want) <= JH.COST_REL * max(1.0, abs(want)), (b, c[b], want)
        else:
            assert c[b] == np.inf, (b, c)


def test_all_labels_masked_no_gradient_is_nan(J, dev):
    """Every non-blank bias -inf, (costs * grad_scale).sum().backward(): no gradient is NaN. The utterances with S > 0
    have no path (cost +inf); the fused factorised-blank gradient pass gives such an utterance exact zeros (a NaN there
    would spread into d_weight and d_bias, which sum over the batch), so their d_enc / d_pred rows are 0 and the
    gradients that remain are the S = 0 utterance's."""
    H, V, blank, enc, pred, w, bias, labels, T, S = _non_finite_case()
    ba = torch.full_like(bias, -float("inf"))
    ba[blank] = bias[blank]
    got = JH.run_hat(J, dev, enc, pred, w, ba, labels, T, S, blank, scale=JH.SCALE)
    for x, name in zip(got[1:], ("d_enc", "d_pred", "d_weight", "d_bias")):
        print(f"    {name}: {int(torch.isnan(x).sum())} NaN of {x.numel()}")
    for x, name in zip(got[1:], ("d_enc", "d_pred", "d_weight", "d_bias")):
        assert not torch.isnan(x).any(), name
    for b in range(len(T)):
        if S[b] > 0:
            assert got[0][b] == np.inf and torch.all(got[1][b] == 0) and torch.all(got[2][b] == 0), b
        else:
            assert np.isfinite(got[0][b]) and bool((got[1][b, : T[b]] != 0).any()), b
    assert bool((got[4] != 0).any())  # d_bias[blank] of the S = 0 utterance


@pytest.mark.parametrize("H,V,blank", [(128, 64, 21), (256, 1000, 995), (512, 256, 255), (640, 130, 128)])
def test_bitwise_reproducible(J, dev, H, V, blank):
    case = JH.hat_case(7 + H, H, V, blank, Trange=(10, 24))
    ref = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
    for _ in range(2):
        got = JH.run_hat(J, dev, *case, blank, scale=JH.SCALE)
        assert np.array_equal(ref[0], got[0])
        for a, b in zip(ref[1:], got[1:]):
            assert torch.equal(a, b)


def _step(J, enc, pred, w, bias, labels, T, S, blank, capturable):
    for x in (enc, pred, w, bias):
        x.grad = None
    costs = J.monotonic_rnnt_joint_hat_loss(enc, pred, w, bias, labels, T, S, blank, capturable=capturable)
    costs.sum().backward()
    return (costs.detach().clone(), enc.grad.clone(), pred.grad.clone(), w.grad.clone(), bias.grad.clone())


@pytest.mark.parametrize("H,V,blank", [(256, 128, 21), (640, 130, 128)])
def test_step_graph_capture_replay(J, dev, H, V, blank):
    """A captured capturable step (live_count_dev: no host read, the tail of G / Hact zeroed) replays bit for bit what
    an eager capturable step computes, agrees with the default step within the gradient tolerance, and makes no
    device-to-host synchronisation (torch's sync debug mode set to error)."""
    enc0, pred0, w0, bias0, labels, T, S = JH.hat_case(31 + H, H, V, blank, Trange=(12, 24), B=3)
    enc = enc0.to(dev).requires_grad_(True)
    pred = pred0.to(dev).requires_grad_(True)
    w = w0.to(dev).requires_grad_(True)
    bias = bias0.to(dev).requires_grad_(True)
    lab, Tt, St = torch.from_numpy(labels).to(dev), torch.from_numpy(T), torch.from_numpy(S)
    eager_cap = _step(J, enc, pred, w, bias, lab, Tt, St, blank, True)
    eager = _step(J, enc, pred, w, bias, lab, Tt, St, blank, False)
    assert torch.equal(eager_cap[0], eager[0])
    for a, b, name in zip(eager_cap[1:], eager[1:], ("d_enc", "d_pred", "d_weight", "d_bias")):
        JH.close(a, b.double().cpu(), name=name)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # any device-to-host read in the step raises
    try:
        _step(J, enc, pred, w, bias, lab, Tt, St, blank, True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _step(J, enc, pred, w, bias, lab, Tt, St, blank, None)
    torch.cuda.current_stream().wait_stream(s)
    for x in (enc, pred, w, bias):
        x.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        costs = J.monotonic_rnnt_joint_hat_loss(enc, pred, w, bias, lab, Tt, St, blank)  # capturable inside capture
        costs.sum().backward()
    gen = torch.Generator(device=dev).manual_seed(3)
    for i in range(2):
        with torch.no_grad():
            enc.copy_(torch.randn(enc.shape, device=dev, generator=gen).to(enc.dtype))
            pred.copy_(torch.randn(pred.shape, device=dev, generator=gen).to(pred.dtype))
        g.replay()
        torch.cuda.synchronize()
        got = (costs.detach().clone(), enc.grad.clone(), pred.grad.clone(), w.grad.clone(), bias.grad.clone())
        e2, p2 = enc.detach().clone().requires_grad_(True), pred.detach().clone().requires_grad_(True)
        w2, b2 = w.detach().clone().requires_grad_(True), bias.detach().clone().requires_grad_(True)
        ref = _step(J, e2, p2, w2, b2, lab, Tt, St, blank, True)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


# ---- align / posteriors / sample with blank_factorized=True, against the materialised read-outs on the reference
# logits (the rules of test_gpu_joint_align / _posteriors / _sample; the two smallest cases of _joint_lattice_cases) ----

LATTICE = ["w1", "ragged"]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(C.DEV)


def _a_prime(c):
    """a' (fp32) of the case's reference logits: log-probabilities whose rows sum to 1, so the softmax helpers of the
    other test files (the oracle, np_sample) take them as acts."""
    from _hat_checks import hat_transform
    return hat_transform(torch.from_numpy(c.acts.astype(np.float64)), c.blank).numpy().astype(np.float32)


@pytest.mark.parametrize("name", LATTICE)
def test_align_blank_factorized(J, name):
    import _align_checks as A
    import monotonic_rnnt_op as op
    import oracle
    c = C.case(name)
    al, costs = J.monotonic_rnnt_joint_align(*C.dev_args(c), blank_factorized=True)
    al, costs = al.cpu().numpy(), costs.cpu().numpy()
    A.check_valid(al, c.labels, c.T, c.S, blank=c.blank)
    _, mc = op.monotonic_rnnt_align(_dev(c.acts), _dev(c.labels), torch.from_numpy(c.T), torch.from_numpy(c.S), None, 0,
                                    c.blank, blank_factorized=True)
    dev_ = C.rel_dev(costs, mc.cpu().numpy())
    print(f"MEASURED hat align {name} vs materialised: {dev_:.3e}")
    assert dev_ <= 1e-5, (name, costs, mc)
    own, _ = oracle.oracle_rnnt(_a_prime(c), c.labels, c.T, c.S, blank=c.blank, alignment=al, max_shift=0, grads=False)
    assert C.rel_dev(costs, own) <= 1e-5, (name, costs, own)
    plain, _ = J.monotonic_rnnt_joint_align(*C.dev_args(c))
    assert torch.equal(plain, J.monotonic_rnnt_joint_align(*C.dev_args(c), blank_factorized=False)[0])


@pytest.mark.parametrize("name", LATTICE)
def test_posteriors_blank_factorized(J, name):
    import _posterior_checks as P
    import monotonic_rnnt_op as op
    c = C.case(name)
    out = J.monotonic_rnnt_joint_posteriors(*C.dev_args(c), blank_factorized=True)
    res = P.Posteriors(*(x.cpu().numpy() for x in out))
    pk = P.Posteriors(C.gather_packed(res.blank, c.T, c.S), C.gather_packed(res.label, c.T, c.S), res.emit,
                      res.label_time, res.costs)
    P.check_invariants(pk, c.T, c.S)
    m = op.monotonic_rnnt_posteriors(_dev(c.acts), _dev(c.labels), torch.from_numpy(c.T), torch.from_numpy(c.S),
                                     blank_label=c.blank, blank_factorized=True)
    m = P.Posteriors(*(x.cpu().numpy() for x in m))
    ref = P.Posteriors(m.blank, m.label, [m.emit[b, :Tb] for b, Tb in enumerate(c.T)],
                       [m.label_time[b, :Sb] for b, Sb in enumerate(c.S)], m.costs.astype(np.float64))
    P.compare(pk, ref, c.T, c.S, name)
    pad = C.padding_mask(res.blank.shape, c.T, c.S)
    assert np.all(res.blank[pad] == 0.0) and np.all(res.label[pad] == 0.0)
    loss = J.monotonic_rnnt_joint_hat_loss(*C.dev_args(c)).cpu().numpy()
    assert res.costs.tobytes() == loss.tobytes()  # the costs are the hat loss, bit for bit


@pytest.mark.parametrize("name", LATTICE)
def test_sample_blank_factorized(J, name):
    import _sample_checks as S
    import monotonic_rnnt_op as op
    K, SEED, CAP = 64, 2, 0.10  # tests/test_gpu_joint_sample.py
    c = C.case(name)
    e, p, w, bias, lab, T, S_, blank = C.dev_args(c)
    out = J.monotonic_rnnt_joint_sample(e, p, w, bias, lab, T, S_, K, SEED, blank_label=blank, blank_factorized=True)
    S.check_types(out, len(c.T), K)
    res = S.Samples(*(x.cpu().numpy() for x in out))
    for k in range(K):
        S.check_valid(res.alignments[:, k, :], c.labels, c.T, c.S, blank=c.blank)
    a32 = _a_prime(c)
    ref = S.np_sample(a32, c.labels, c.T, c.S, K, SEED, blank=c.blank)
    tol = 1e-5 * np.maximum(1.0, np.abs(ref.costs))
    close = S.np_sample(a32, c.labels, c.T, c.S, K, SEED, tol=tol, blank=c.blank).close
    print(f"MEASURED hat joint sample {name}: close {int(close.sum())} of {close.size}")
    assert close.mean() <= CAP, (name, float(close.mean()))
    mat = op.monotonic_rnnt_sample(_dev(c.acts), _dev(c.labels), torch.from_numpy(c.T), torch.from_numpy(c.S), K, SEED,
                                   blank_label=c.blank, blank_factorized=True)
    mat_al = mat.alignments.cpu().numpy()
    assert res.alignments.shape == mat_al.shape
    assert np.array_equal(res.alignments[~close], mat_al[~close]), name
    S.assert_costs(res.path_costs[~close], mat.path_costs.cpu().numpy()[~close].astype(np.float64))
    S.assert_costs(res.costs, mat.costs.cpu().numpy().astype(np.float64))
