"""monotonic_rnnt_expected_cost(blank_factorized=True) on the GPU (mrnnt_hat_expect_forward / mrnnt_hat_expect_backward,
HatExpectRows in csrc/mrnnt_expect.hip): the shared checks of tests/_hat_weight_checks.py on GPU tensors, and what only
the GPU path has: bf16 / fp16 acts, device-resident lengths, the tracked backward, results equal to the host
implementation's, and HIP-graph capture.

Row lengths and the gradient kernels they take (f32): V = 5 the scalar kernel, 64 the staged kernel with U = 1, 512
U = 2, 1024 U = 4; bf16 / fp16 at V = 2048 (256 vectors: U = 4)."""
import numpy as np
import pytest
import torch

import _expect_checks as E
import _hat_checks as H
import _hat_weight_checks as C
import _path_checks as P

pytestmark = pytest.mark.gpu

VS = [5, 64, 512, 1024]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return C.Dev("cuda:0")


@pytest.mark.parametrize("V,blank", [(V, b) for V in VS for b in H.blank_positions(V)])
def test_parity_with_the_dp_yardstick(dev, V, blank):
    C.check_expect_parity(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, b) for b in H.blank_positions(5)])
def test_parity_with_path_enumeration(dev, V, blank):
    C.check_expect_brute(dev, V, blank)


@pytest.mark.parametrize("dtype,eps", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
@pytest.mark.parametrize("blank", H.blank_positions(2048))
def test_reduced_precision_acts(dev, blank, dtype, eps):
    """The yardstick on the upcast values, plus one rounding of the output type."""
    C.check_expect_parity(dev, 2048, blank, dtype=dtype, eps=eps)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 47), (1024, 1023)])
def test_non_finite_logits(dev, V, blank):
    C.check_expect_non_finite(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63), (1024, 767), (100, 98), (1028, 1024)])
def test_consistency_with_posteriors_and_the_hat_loss(dev, V, blank):
    C.check_expect_consistency(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 0)])
def test_restricting_alignment(dev, V, blank):
    C.check_restriction(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 47)])
def test_reproducible_independent_and_equal_to_the_host_implementation(dev, V, blank):
    (acts, labels, T, S, wb, we, ge, gc), (e, c, g) = C.check_expect_reproducible(dev, V, blank)
    he, hc, hg = C.Dev("cpu").expect(acts, labels, T, S, wb, we, ge, gc, blank)
    Wb = E.cost_bound(wb, we, T, S)
    E.assert_expected(e, he.astype(np.float64), Wb)
    C.assert_costs(c, hc.astype(np.float64))
    E.assert_grads(g, hg.astype(np.float64), E.grad_tol(T, S, Wb, ge, gc))


@pytest.mark.parametrize("padded", [False, True])
def test_tracked_backward_equals_untracked(dev, padded):
    """mrnnt_hat_expect_backward_tracked == mrnnt_hat_expect_backward, itself again on a second call into the same
    buffer, and it keeps a valid row state."""
    import monotonic_rnnt_op as op
    V, blank = 1024, 767
    acts, labels, T, S, wb, we, ge, gc = C.expect_problem(V, blank, seed=19)
    shape = C.pad_shape(T, S)
    pad = (lambda x: P.pack_to_padded(x, T, S, *shape, np.nan)) if padded else (lambda x: x)
    a = dev.t(pad(acts))
    wbd, wed = dev.t(pad(wb[:, None])[..., 0]), dev.t(pad(we[:, None])[..., 0])
    ged, gcd = dev.t(ge), dev.t(gc)
    prep = op._Prepared(a, dev.t(labels), torch.from_numpy(T), torch.from_numpy(S), None, 0, blank)
    ws = prep.workspace(expect=True)
    op._call(prep, "hat_expect_forward", op._ptr(ws), ws.numel(), op._ptr(wbd), op._ptr(wed), None, None, 1)
    plain = torch.full_like(a, 7.0)
    op._call(prep, "hat_expect_backward", op._ptr(ws), ws.numel(), op._ptr(wbd), op._ptr(wed), op._ptr(ged),
             op._ptr(gcd), op._ptr(plain), lengths=False)
    rows = a.numel() // V
    state = torch.zeros(rows, dtype=torch.uint8, device=a.device)
    buf = torch.full_like(a, 5.0)
    for _ in range(2):
        op._call(prep, "hat_expect_backward_tracked", op._ptr(ws), ws.numel(), op._ptr(wbd), op._ptr(wed), op._ptr(ged),
                 op._ptr(gcd), op._ptr(buf), op._ptr(state), rows, lengths=False)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    st = state.cpu().numpy()
    zero_rows = (buf.reshape(rows, V) == 0).all(dim=1).cpu().numpy()
    assert set(np.unique(st)) <= {0, 1} and st.max() == 1
    assert np.all(zero_rows[st == 1])  # a row the state calls zero is zero


def test_graph_capture_equals_eager(dev):
    """One torch.cuda.graph capture and replay of forward + backward with device lengths equals eager, bit for bit."""
    import monotonic_rnnt_op as op
    V, blank = 1024, 767
    acts, labels, T, S, wb, we, ge, gc = C.expect_problem(V, blank, seed=21)
    other = np.random.default_rng(23).standard_normal(acts.shape).astype(np.float32)
    a = dev.t(acts).requires_grad_(True)
    lab, Td, Sd, wbd, wed, ged, gcd = (dev.t(x) for x in (labels, T, S, wb, we, ge, gc))

    def step():
        e, c = op.monotonic_rnnt_expected_cost(a, lab, Td, Sd, wbd, wed, None, 0, blank, blank_factorized=True)
        torch.autograd.backward((e, c), (ged, gcd))
        return e, c

    side = torch.cuda.Stream(dev.device)  # warm-up on a side stream, as torch.cuda.graph asks
    side.wait_stream(torch.cuda.current_stream(dev.device))
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = None
            step()
    torch.cuda.current_stream(dev.device).wait_stream(side)
    a.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        se, sc = step()
    with torch.no_grad():
        a.copy_(dev.t(other))
    graph.replay()
    torch.cuda.synchronize()
    e, c, g = dev.expect(other, labels, T, S, wb, we, ge, gc, blank, device_lengths=True)
    assert se.detach().cpu().numpy().tobytes() == e.tobytes() and sc.detach().cpu().numpy().tobytes() == c.tobytes()
    assert a.grad.cpu().numpy().tobytes() == g.tobytes()
    op.check_lengths()
