"""monotonic_rnnt_path_loss on the MI355X (mrnnt_path_forward / mrnnt_path_backward, csrc/mrnnt_path.hip): the shared
checks of tests/_path_checks.py on GPU tensors, and what only the GPU path has: bf16 / fp16 acts, an unaligned acts
pointer (the scalar kernels), results equal to the host implementation's, utterance order, device-resident lengths,
their validation and HIP-graph capture."""
import numpy as np
import pytest
import torch

import _path_checks as C
import _sample_checks as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def op():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _d(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gpu(acts, labels, T, S, al, w=None, dtype=None, device_lengths=False, unaligned=False):
    import monotonic_rnnt_op as op
    a = _d(acts) if dtype is None else _d(acts).to(dtype)
    if unaligned:  # rows that start 4 bytes past a 16-byte boundary: the scalar kernels
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
        buf[1:].copy_(a.reshape(-1))
        a = buf[1:].view(a.shape)
        assert a.data_ptr() % 16 != 0 and a.is_contiguous()
    a.requires_grad_(True)
    Tt, St = (_d(T), _d(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))
    pc = op.monotonic_rnnt_path_loss(a, _d(labels), Tt, St, _d(al), blank_label=C.BLANK)
    assert pc.is_cuda and pc.dtype == torch.float32 and tuple(pc.shape) == tuple(al.shape[:2]) and pc.requires_grad
    pc.backward(torch.ones_like(pc) if w is None else _d(np.asarray(w, np.float32)))
    assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
    return pc.detach().cpu().numpy(), a.grad.float().cpu().numpy()


def _same(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


@pytest.mark.parametrize("name", [c[0] for c in C.EDGE_CASES])
def test_edge_shapes_against_the_yardstick(op, name):
    C.check_edge_case(run_gpu, name)


@pytest.mark.parametrize("dtype,eps", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
@pytest.mark.parametrize("name", ["scalar_v5_k3", "v32_k64", "v1024_k3"])
def test_reduced_precision_acts(op, name, dtype, eps):
    """bf16 / fp16 acts and grads: the yardstick on the upcast values, plus one rounding of the output type. V = 5 is
    the scalar path (V % 8 != 0), V = 32 / 1024 the vector path."""
    acts, labels, T, S, al, w = C.edge_problem(name)
    up = torch.from_numpy(acts).to(dtype).to(torch.float32).numpy()
    C.check_against_yardstick(run_gpu, acts, labels, T, S, al, w, eps=eps, yard_acts=up, dtype=dtype)


def test_unaligned_acts_take_the_scalar_path(op):
    acts, labels, T, S, al, w = C.edge_problem("v32_k64")
    C.check_against_yardstick(run_gpu, acts, labels, T, S, al, w, unaligned=True)


def test_signed_weights_and_cancellation(op):
    C.check_signed_weights(run_gpu)


def test_invalid_rows(op):
    C.check_invalid_rows(run_gpu)


@pytest.mark.parametrize("V", [12, 7])
def test_padded_layout_bit_identical_to_packed(op, V):
    C.check_padded(run_gpu, V)


def _align_gpu(acts, labels, T, S):
    import monotonic_rnnt_op as op
    al, c = op.monotonic_rnnt_align(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S))
    return al.cpu().numpy(), c.cpu().numpy()


def _sample_gpu(acts, labels, T, S, K, seed):
    import monotonic_rnnt_op as op
    out = op.monotonic_rnnt_sample(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S), K, seed)
    return SC.Samples(*(x.cpu().numpy() for x in out))


def _loss_grad_gpu(acts, labels, T, S, al):
    import monotonic_rnnt_op as op
    a = _d(acts).requires_grad_(True)
    op.monotonic_rnnt_loss(a, _d(labels), torch.from_numpy(T), torch.from_numpy(S), _d(al), 0).sum().backward()
    return a.grad.cpu().numpy().astype(np.float64)


def test_consistency_with_align_sample_and_the_restricted_loss(op):
    C.check_consistency(run_gpu, _align_gpu, _sample_gpu, _loss_grad_gpu)


def test_non_finite_logits(op):
    C.check_non_finite(run_gpu)


def test_reproducible_permutable_and_equal_to_the_host_implementation(op):
    acts, labels, T, S, al, w, c, g = C.check_reproducible(run_gpu)
    # the utterances in another order: the same bits
    perm = [2, 0, 3, 1]
    off = C.offsets(T, S)
    pa = np.concatenate([acts[off[b]:off[b + 1]] for b in perm])
    pc, pg = run_gpu(pa, labels[perm], T[perm], S[perm], np.ascontiguousarray(al[perm]), w[perm])
    assert pc.tobytes() == c[perm].tobytes()
    assert pg.tobytes() == np.concatenate([g[off[b]:off[b + 1]] for b in perm]).tobytes()
    # the host implementation: within the tolerances of the yardstick
    hc, hg = C.run_cpu(acts, labels, T, S, al, w)
    C.assert_costs(c, hc.astype(np.float64))
    _, _, visited, wsum = C.yardstick(acts, labels, T, S, al, w)
    C.assert_path_grads(g, hg.astype(np.float64), wsum)
    assert np.all(g[~visited] == 0.0) and np.all(hg[~visited] == 0.0)


def test_device_lengths_give_the_host_lengths_bits(op):
    for name in ("scalar_v5_k3", "v32_k64"):
        acts, labels, T, S, al, w = C.edge_problem(name)
        assert _same(run_gpu(acts, labels, T, S, al, w, device_lengths=True), run_gpu(acts, labels, T, S, al, w))
    acts, labels, T, S, al, w = C.small_problem(seed=28)
    pad = C.pack_to_padded(acts, T, S, 31, 19, np.nan)
    assert _same(run_gpu(pad, labels, T, S, al, w, device_lengths=True), run_gpu(pad, labels, T, S, al, w))
    op.check_lengths()


@pytest.mark.parametrize("case", ["T_above_path_stride", "T_below_S"])
def test_invalid_device_lengths_fail_closed(op, case):
    op.check_lengths()  # nothing pending
    acts, labels, T, S, al, w = C.small_problem(seed=29)
    if case == "T_above_path_stride":
        al = np.ascontiguousarray(al[:, :, :29])  # T_3 = 30
        Tb, Sb, a = T, S, acts
    else:
        Tb, Sb = np.array([2, 4], np.int32), np.array([3, 2], np.int32)  # S_0 > T_0
        a, labels, al, w = acts[:20], labels[:2], np.ascontiguousarray(al[:2]), w[:2]
    x = _d(a).requires_grad_(True)
    pc = op.monotonic_rnnt_path_loss(x, _d(labels), _d(Tb), _d(Sb), _d(al))
    pc.backward(_d(w))
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    assert bool(torch.isnan(pc).all()) and bool(torch.isnan(x.grad).all())
    op.check_lengths()  # reported once


def test_graph_capture_with_device_lengths(op):
    """Forward + backward with device-resident lengths captured once and replayed twice on new logits (the default
    queue settings): the replayed costs and gradients are the eager bits."""
    acts, labels, T, S, al, w = C.small_problem(seed=30, K=5, V=16)
    other = np.random.default_rng(31).standard_normal(acts.shape).astype(np.float32)
    a = _d(acts).requires_grad_(True)
    lab, Td, Sd, ald, wd = _d(labels), _d(T), _d(S), _d(al), _d(w)

    def step():
        pc = op.monotonic_rnnt_path_loss(a, lab, Td, Sd, ald)
        pc.backward(wd)
        return pc

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = None
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    a.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    with torch.no_grad():
        a.copy_(_d(other))
    eager = run_gpu(other, labels, T, S, al, w, device_lengths=True)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert _same((static.detach().cpu().numpy(), a.grad.cpu().numpy()), eager)
    op.check_lengths()
