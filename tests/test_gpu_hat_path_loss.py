"""monotonic_rnnt_path_loss(blank_factorized=True) on the GPU (mrnnt_hat_path_forward / mrnnt_hat_path_backward,
HatPathRows in csrc/mrnnt_path.hip): the shared checks of tests/_hat_weight_checks.py on GPU tensors, and what only the
GPU path has: bf16 / fp16 acts, device-resident lengths, the tracked backward, results equal to the host
implementation's, and HIP-graph capture.

Row lengths and the gradient kernels they take (f32): V = 5 the scalar kernel, 64 the staged kernel with U = 1, 512
U = 2, 1024 U = 4; bf16 / fp16 at V = 2048 (256 vectors: U = 4)."""
import numpy as np
import pytest
import torch

import _hat_checks as H
import _hat_weight_checks as C
import _path_checks as P

pytestmark = pytest.mark.gpu

VS = [5, 64, 512, 1024]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return C.Dev("cuda:0")


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("V,blank", [(V, b) for V in VS for b in H.blank_positions(V)])
def test_parity_with_the_yardstick(dev, V, blank, K):
    C.check_path_parity(dev, V, blank, K)


@pytest.mark.parametrize("dtype,eps", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
@pytest.mark.parametrize("blank", H.blank_positions(2048))
def test_reduced_precision_acts(dev, blank, dtype, eps):
    """The yardstick on the upcast values, plus one rounding of the output type."""
    C.check_path_parity(dev, 2048, blank, 5, dtype=dtype, eps=eps)


@pytest.mark.parametrize("V,blank", [(5, 2), (1024, 767)])
def test_transform_identity(dev, V, blank):
    C.check_transform_identity(dev, V, blank)


def test_signed_weights(dev):
    C.check_signed_weights(dev)         # V = 7: the scalar kernel
    C.check_signed_weights(dev, 64, 9)  # the staged kernel


@pytest.mark.parametrize("zb", [60.0, 100.0, -60.0, -100.0])
@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63), (1024, 0)])
def test_dominant_and_suppressed_blank(dev, V, blank, zb):
    C.check_blank_logit(dev, V, blank, zb)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 47), (1024, 1023)])
def test_non_finite_logits(dev, V, blank):
    C.check_path_non_finite(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 4), (64, 0), (100, 98), (1028, 1024)])
def test_consistency_with_sample_and_align(dev, V, blank):
    C.check_path_consistency(dev, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 47)])
def test_reproducible_independent_and_equal_to_the_host_implementation(dev, V, blank):
    (acts, labels, T, S, al, w), (c, g) = C.check_path_reproducible(dev, V, blank)
    hc, hg = C.Dev("cpu").path(acts, labels, T, S, al, w, blank)
    C.assert_costs(c, hc.astype(np.float64))
    _, _, visited, wsum = C.path_yardstick(acts, labels, T, S, al, w, blank)
    P.assert_path_grads(g, hg.astype(np.float64), wsum)
    assert np.all(g[~visited] == 0.0) and np.all(hg[~visited] == 0.0)


@pytest.mark.parametrize("padded", [False, True])
def test_tracked_backward_equals_untracked(dev, padded):
    """mrnnt_hat_path_backward_tracked == mrnnt_hat_path_backward, itself again on a second call into the same buffer,
    and it keeps a valid row state (rows outside the hull and padding rows are known zeros after the first call)."""
    import monotonic_rnnt_op as op
    V, blank, K = 1024, 767, 5
    acts, labels, T, S = C.problem(V, blank, seed=19)
    al = C.make_paths(labels, T, S, K, blank)
    w = dev.t(np.random.default_rng(20).standard_normal((len(T), K)).astype(np.float32))
    x = P.pack_to_padded(acts, T, S, *C.pad_shape(T, S), np.nan) if padded else acts
    a, ald = dev.t(x), dev.t(al)
    prep = op._Prepared(a, dev.t(labels), torch.from_numpy(T), torch.from_numpy(S), None, 0, blank)
    ws = prep.workspace(num_paths=K)
    L = al.shape[2]
    op._call(prep, "hat_path_forward", op._ptr(ws), ws.numel(), op._ptr(ald), K, L, None)
    plain = torch.full_like(a, 7.0)
    op._call(prep, "hat_path_backward", op._ptr(ws), ws.numel(), op._ptr(ald), K, L, op._ptr(w), op._ptr(plain),
             lengths=False)
    rows = a.numel() // V
    state = torch.zeros(rows, dtype=torch.uint8, device=a.device)
    buf = torch.full_like(a, 5.0)
    for _ in range(2):
        op._call(prep, "hat_path_backward_tracked", op._ptr(ws), ws.numel(), op._ptr(ald), K, L, op._ptr(w),
                 op._ptr(buf), op._ptr(state), rows, lengths=False)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    st = state.cpu().numpy()
    zero_rows = (buf.reshape(rows, V) == 0).all(dim=1).cpu().numpy()
    assert set(np.unique(st)) <= {0, 1} and st.max() == 1
    assert np.all(zero_rows[st == 1])  # a row the state calls zero is zero


def test_graph_capture_equals_eager(dev):
    """One torch.cuda.graph capture and replay of forward + backward with device lengths equals eager, bit for bit."""
    import monotonic_rnnt_op as op
    V, blank, K = 1024, 767, 5
    acts, labels, T, S = C.problem(V, blank, seed=21)
    al = C.make_paths(labels, T, S, K, blank)
    w = np.random.default_rng(22).standard_normal((len(T), K)).astype(np.float32)
    other = np.random.default_rng(23).standard_normal(acts.shape).astype(np.float32)
    a = dev.t(acts).requires_grad_(True)
    lab, Td, Sd, ald, wd = dev.t(labels), dev.t(T), dev.t(S), dev.t(al), dev.t(w)

    def step():
        pc = op.monotonic_rnnt_path_loss(a, lab, Td, Sd, ald, blank_label=blank, blank_factorized=True)
        pc.backward(wd)
        return pc

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
        static = step()
    with torch.no_grad():
        a.copy_(dev.t(other))
    graph.replay()
    torch.cuda.synchronize()
    c_eager, g_eager = dev.path(other, labels, T, S, al, w, blank, device_lengths=True)
    assert static.detach().cpu().numpy().tobytes() == c_eager.tobytes()
    assert a.grad.cpu().numpy().tobytes() == g_eager.tobytes()
    op.check_lengths()
