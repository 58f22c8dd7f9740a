"""The factorised-blank (HAT) loss and its read-outs on the GPU (mrnnt_hat_*), against the fp64 oracle on transformed
logits (tests/_hat_checks.py: reference, tolerances, shapes).

Row lengths and the kernels they take: V = 5 the scalar kernels; 64 and 256 (f32) the 16-lane log-softmax rows and the
staged gradient with U = 1; 512 / 1024 single-chunk rows, U = 2 / 4; 2048 f32 rows of two chunks (the interior blank
index 1535 lies in the second). bf16 rows are half as many vectors: 512 takes the 16-lane rows, 2048 a single chunk."""
import numpy as np
import pytest
import torch

import _hat_checks as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import monotonic_rnnt_op
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return H.Runner(monotonic_rnnt_op, torch.device("cuda:0"))


VS = [5, 64, 256, 512, 1024, 2048]
CASES = [(V, b) for V in VS for b in H.blank_positions(V)]


@pytest.mark.parametrize("V,blank", CASES)
def test_parity_f32(run, V, blank):
    H.check_parity(run, V, blank, layouts=(False, True), lengths=(False, True))


@pytest.mark.parametrize("V,blank", CASES)
def test_parity_bf16(run, V, blank):
    """(gradients: 1e-4 absolute + one rounding of the bf16 output, as tests/test_gpu_parity.py)"""
    H.check_parity(run, V, blank, dtype=torch.bfloat16, layouts=(False, True), lengths=(False, True), rel=2.0 ** -8)


@pytest.mark.parametrize("zb", [60.0, 100.0, -60.0, -100.0])
@pytest.mark.parametrize("V,blank", [(5, 2), (256, 255), (1024, 0), (2048, 1535)])
def test_dominant_and_suppressed_blank(run, V, blank, zb):
    H.check_blank_logit(run, V, blank, zb)


@pytest.mark.parametrize("V,blank", [(5, 4), (256, 0), (1024, 767), (2048, 1535)])
def test_label_shift(run, V, blank):
    H.check_label_shift(run, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 63), (1024, 767), (2048, 1535)])
def test_closed_form(run, V, blank):
    H.check_closed_form(run, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 0), (256, 191), (1024, 1023), (2048, 1535)])
def test_non_finite(run, V, blank):
    H.check_non_finite(run, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (1024, 767)])
def test_bitwise(run, V, blank):
    """Two runs give the same bits; padding rows of the 4-D layout are 0; .sum().backward() (a stride-0 upstream
    gradient) equals an explicit ones vector."""
    acts, labels = H.problem(V, blank, seed=8)
    c1, g1, raw1 = run.loss(acts, labels, blank, padded=True, device_lengths=True)
    c2, g2, raw2 = run.loss(acts, labels, blank, padded=True, device_lengths=True)
    assert c1.tobytes() == c2.tobytes() and raw1.tobytes() == raw2.tobytes()
    mask = np.ones(raw1.shape[:3], bool)
    for b, (Tb, Sb) in enumerate(H.SHAPES):
        mask[b, :Tb, :Sb + 1] = False
    assert np.all(raw1[mask] == 0.0)
    c3, g3, _ = run.loss(acts, labels, blank)  # packed, host lengths: the same bits row for row
    assert c3.tobytes() == c1.tobytes() and g3.tobytes() == g1.tobytes()
    c4, g4, _ = run.loss(acts, labels, blank, summed=True)
    assert c4.tobytes() == c3.tobytes() and g4.tobytes() == g3.tobytes()


@pytest.mark.parametrize("V,blank,padded", [(5, 2, False), (1024, 767, False), (1024, 767, True)])
def test_tracked_backward_equals_untracked(run, V, blank, padded):
    """mrnnt_hat_backward_tracked == mrnnt_hat_backward, and itself again on a second call into the same buffer."""
    import monotonic_rnnt_op as op
    acts, labels = H.problem(V, blank, seed=9)
    a = run.acts(acts, padded=padded)
    lab, T, S = run.tensors(labels, False)
    prep = op._Prepared(a, lab, T, S, None, 0, blank)
    _, ws = op._forward(prep, with_beta=True, hat=True)
    plain = op._backward(prep, ws, None, torch.full_like(a, 7.0), hat=True)
    rows = a.numel() // V
    state = torch.zeros(rows, dtype=torch.uint8, device=a.device)
    buf = torch.full_like(a, 5.0)
    for _ in range(2):
        op._call(prep, "hat_backward_tracked", op._ptr(ws), None, op._ptr(buf), op._ptr(state), rows, lengths=False)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    # the staged kernel keeps the row state (out-of-band and padding rows are known zeros after the first call);
    # the scalar kernel (V = 5) keeps none: every byte stays "unknown"
    assert int(state.max()) == (1 if V % 4 == 0 else 0)


@pytest.mark.parametrize("V,blank,masked", H.MASKED_CASES, ids=[f"{v}-{b}" for v, b, _ in H.MASKED_CASES])
def test_masked_non_label_entries(run, V, blank, masked):
    H.check_masked_entries(run, V, blank, masked)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 0)])
def test_align_is_best_path(run, V, blank):
    H.check_align(run, V, blank)


def _tensors(run, acts, labels):
    lab, T, S = run.tensors(labels, True)
    return run.acts(acts), lab, T, S


@pytest.mark.parametrize("V,blank", [(5, 2), (1024, 767)])
def test_posteriors(run, V, blank):
    def post(acts, labels, blank):
        r = run.op.monotonic_rnnt_posteriors(*_tensors(run, acts, labels), blank_label=blank, max_input_length=12,
                                             blank_factorized=True)
        return type(r)(*[x.cpu().numpy() for x in r])
    H.check_posteriors(post, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (1024, 767)])
def test_sample_path_costs(run, V, blank):
    def sample(acts, labels, blank, K):
        r = run.op.monotonic_rnnt_sample(*_tensors(run, acts, labels), num_samples=K, seed=11, blank_label=blank,
                                         max_input_length=12, blank_factorized=True)
        return type(r)(*[x.cpu().numpy() for x in r])
    H.check_sample(sample, V, blank)


def test_graph_capture_equals_eager(run):
    """One torch.cuda.graph capture and replay of forward + backward with device lengths equals eager, bit for bit."""
    V, blank = 1024, 767
    acts, labels = H.problem(V, blank, seed=10)
    op = run.op
    lab, T, S = run.tensors(labels, True)
    other = np.random.default_rng(12).standard_normal(acts.shape).astype(np.float32)
    a = run.acts(acts).requires_grad_(True)

    def step():
        costs = op.monotonic_rnnt_hat_loss(a, lab, T, S, None, 0, blank)
        costs.sum().backward()
        return costs

    side = torch.cuda.Stream(run.device)  # warm-up on a side stream, as torch.cuda.graph asks
    side.wait_stream(torch.cuda.current_stream(run.device))
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = None
            step()
    torch.cuda.current_stream(run.device).wait_stream(side)
    a.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    with torch.no_grad():
        a.copy_(run.acts(other))
    graph.replay()
    torch.cuda.synchronize()
    c_eager, g_eager, _ = run.loss(other, labels, blank, device_lengths=True, summed=True)
    assert static.detach().cpu().numpy().astype(np.float64).tobytes() == c_eager.tobytes()
    assert a.grad.cpu().numpy().tobytes() == g_eager.tobytes()
    op.check_lengths()
