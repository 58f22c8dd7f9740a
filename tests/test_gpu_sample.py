"""monotonic_rnnt_sample on the MI355X (mrnnt_sample, csrc/mrnnt_sample.hip): the shared checks of
tests/_sample_checks.py on GPU tensors, the kernel's boundaries -- samples per wave, the 16-frame chunk and the 4-frame
Philox block, the 96 staged label positions and the fallback beyond them, one utterance with one sample -- and what
only the GPU path has: paths equal to the host implementation's, the padded layout, bf16 acts, device-resident lengths
and their validation, a stride shorter than an utterance, and HIP-graph capture."""
import ctypes

import numpy as np
import pytest
import torch

import _posterior_checks as P
import _sample_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def op():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _d(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gpu(acts, labels, T, S, K, seed, first_sample=0, alignment=None, k=0, max_input_length=None,
            device_lengths=False, dtype=None):
    import monotonic_rnnt_op as op
    a = _d(acts) if dtype is None else _d(acts).to(dtype)
    Tt, St = (_d(T), _d(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))
    out = op.monotonic_rnnt_sample(a, _d(labels), Tt, St, K, seed, first_sample=first_sample, alignment=_d(alignment),
                                   max_distance_from_alignment=k, blank_label=C.BLANK,
                                   max_input_length=max_input_length)
    C.check_types(out, len(T), K)
    assert all(x.is_cuda for x in out)
    return C.Samples(*(x.cpu().numpy() for x in out))


def _post_gpu(acts, labels, T, S):
    import monotonic_rnnt_op as op
    out = op.monotonic_rnnt_posteriors(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S))
    return P.Posteriors(*(x.cpu().numpy() for x in out))


def _same_bits(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


def test_validity_and_path_cost(op):
    C.check_validity_and_cost(run_gpu)


@pytest.mark.parametrize("W", [33, 96, 97])
def test_exact_paths_free_and_restricted(op, W):
    """S + 1 = W: 33 (T <= 40), and 96 | 97 either side of the staged window; K = 64, free and restricted."""
    C.check_exact_paths(run_gpu, W)


def test_exact_paths_beyond_the_staged_window(op):
    """A two-mode posterior: samples of one wave stand 100 label positions apart, more than the 96 staged ones, so
    lanes take p_label from global memory. K = 130: two full waves and one of 2 samples. Observed close samples of the
    yardstick (seed 5): 3 of 260, 1.2 %."""
    acts, labels, T, S = C.bimodal_problem()
    res, _ = C.check_exact(run_gpu, acts, labels, T, S, 130, 5)
    ends = (res.alignments[0, :, :100] != C.BLANK).sum(axis=1)
    assert (ends >= 97).sum() >= 10 and (ends <= 3).sum() >= 10
    few = run_gpu(acts, labels, T, S, 3, 5, first_sample=64)  # another wave composition, the same samples
    assert np.array_equal(few.alignments, res.alignments[:, 64:67])
    assert few.path_costs.tobytes() == res.path_costs[:, 64:67].tobytes()


# T either side of the 16-frame chunk (15 | 16 | 17, 31 | 32 | 33) and of a multiple of 4 (19 | 20 | 21), with S = 0,
# S = T and T = 1 mixed in. Observed close samples of the yardstick (seed 8): K = 1: 0 of 11, 63: 3 of 693, 64: 3 of
# 704, 65: 3 of 715, 130: 3 of 1430.
_FRAME_SHAPES = [(15, 4), (16, 16), (17, 0), (19, 7), (20, 3), (21, 20), (31, 9), (32, 30), (33, 12), (1, 1), (3, 1)]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_samples_per_wave_and_frame_chunks(op, K):
    acts, labels, T, S = C.ragged(np.random.default_rng(50), _FRAME_SHAPES, 6)
    C.check_exact(run_gpu, acts, labels, T, S, K, 8)


def test_one_utterance_one_sample(op):
    """B = 1, K = 1: a grid of one wave with one live lane; the path cost against the oracle."""
    acts, labels, T, S = C.ragged(np.random.default_rng(51), [(18, 5)], 6)
    res, _ = C.check_exact(run_gpu, acts, labels, T, S, 1, 22)
    C.check_path_costs(res, acts, labels, T, S)


def test_path_frequencies(op):
    C.check_path_frequencies(run_gpu)


def test_arc_marginals(op):
    C.check_arc_marginals(run_gpu, _post_gpu)


def test_determinism_and_indexing(op):
    C.check_determinism(run_gpu)


def test_gpu_paths_equal_cpu_paths(op):
    """The same integer stream and decision rule on both devices: every sample that is not close is the host
    implementation's, element for element (the two states differ by rounding only). Close samples of the yardstick
    (seed 17): 1 of 320."""
    acts, labels, T, S = C.ragged(np.random.default_rng(31), [(40, 15), (38, 30), (12, 0), (7, 7), (36, 3)], 12)
    g = run_gpu(acts, labels, T, S, 64, 17)
    c = C.run_cpu(acts, labels, T, S, 64, 17)
    exact = ~C.np_sample(acts, labels, T, S, 64, 17).close
    assert exact.mean() >= 1.0 - C.CLOSE_CAP
    assert np.array_equal(g.alignments[exact], c.alignments[exact])
    C.assert_costs(g.path_costs[exact], c.path_costs[exact].astype(np.float64))


def test_value_domain(op):
    C.check_value_domain(run_gpu)


def test_strides(op):
    C.check_strides(run_gpu)
    acts, labels, T, S = C.ragged(np.random.default_rng(8), [(9, 4), (14, 6), (5, 0)], 8)
    with pytest.raises(RuntimeError, match="alignments row stride"):
        run_gpu(acts, labels, T, S, 4, 1, max_input_length=13)


def _pack_to_padded(acts, T, S, pad_T, pad_S1, fill):
    off = C.offsets(T, S)
    out = np.full((len(T), pad_T, pad_S1, acts.shape[1]), fill, np.float32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    return out


def test_padded_layout_gives_the_packed_samples(op):
    """4-D acts [B, 27, 15, V]: L = 27; the samples of the packed call, exact where no sample is close."""
    acts, labels, T, S = C.ragged(np.random.default_rng(10), [(19, 7), (25, 11), (6, 0), (13, 13)], 16)

    def run_padded(a, lab, T_, S_, K, seed, **kw):
        out = op.monotonic_rnnt_sample(_d(_pack_to_padded(a, T_, S_, 27, 15, 3.0)), _d(lab), torch.from_numpy(T_),
                                       torch.from_numpy(S_), K, seed, blank_label=C.BLANK)
        assert tuple(out.alignments.shape) == (4, K, 27)
        return C.Samples(*(x.cpu().numpy() for x in out))
    res, _ = C.check_exact(run_padded, acts, labels, T, S, 64, 14)
    packed = run_gpu(acts, labels, T, S, 64, 14, max_input_length=27)
    exact = ~C.np_sample(acts, labels, T, S, 64, 14).close
    assert np.array_equal(res.alignments[exact], packed.alignments[exact])


def test_bf16_acts_give_the_samples_of_the_upcast_values(op):
    acts, labels, T, S = C.ragged(np.random.default_rng(11), [(31, 12), (38, 35), (9, 0)], 24)
    up = torch.from_numpy(acts).to(torch.bfloat16).to(torch.float32).numpy()  # the values the kernel sees
    res, _ = C.check_exact(run_gpu, acts, labels, T, S, 64, 15, state_acts=up, dtype=torch.bfloat16)
    f32 = run_gpu(up, labels, T, S, 64, 15)
    exact = ~C.np_sample(up, labels, T, S, 64, 15).close
    assert np.array_equal(res.alignments[exact], f32.alignments[exact])


def test_device_lengths_give_the_host_lengths_samples(op):
    acts, labels, T, S = C.ragged(np.random.default_rng(12), [(33, 9), (80, 70), (5, 0), (21, 21)], 12)
    res = run_gpu(acts, labels, T, S, 20, 6, max_input_length=80)
    assert _same_bits(run_gpu(acts, labels, T, S, 20, 6, max_input_length=80, device_lengths=True), res)
    given = C.random_alignment(np.random.default_rng(13), labels, T, S)
    r = run_gpu(acts, labels, T, S, 20, 6, alignment=given, k=2)
    dr = run_gpu(acts, labels, T, S, 20, 6, alignment=given, k=2, device_lengths=True)  # L from alignment.size(1)
    assert dr.alignments.shape == (4, 20, 80) and _same_bits(dr, r)
    op.check_lengths()
    with pytest.raises(RuntimeError, match="max_input_length"):
        op.monotonic_rnnt_sample(_d(acts), _d(labels), _d(T), _d(S), 4, 1)


def test_invalid_device_lengths_fail_closed(op):
    op.check_lengths()  # nothing pending
    acts = torch.randn(8 + 12, 5, device=DEV)
    lab = torch.ones(2, 3, dtype=torch.int32, device=DEV)
    out = op.monotonic_rnnt_sample(acts, lab, torch.tensor([2, 4], device=DEV), torch.tensor([3, 2], device=DEV), 70, 1,
                                   max_input_length=6)  # S_0 > T_0
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    assert tuple(out.alignments.shape) == (2, 70, 6)
    assert bool((out.alignments == -1).all()) and bool(torch.isnan(out.path_costs).all())
    assert bool(torch.isnan(out.costs).all())
    op.check_lengths()  # reported once


def test_device_lengths_with_a_short_stride(op):
    """An out_stride below a T_b (device-resident lengths: the host cannot check it): that utterance's rows are -1 and
    its path costs NaN, the others are unaffected, nothing is written past the buffer (a guard region follows it) and
    the status word is raised."""
    import _mrnnt_lib as L
    op.check_lengths()
    acts, labels, T, S = C.ragged(np.random.default_rng(14), [(9, 3), (14, 6), (5, 0)], 8)
    K, stride, guard = 5, 10, 64
    full = run_gpu(acts, labels, T, S, K, 9)
    prep = op._Prepared(_d(acts), _d(labels), _d(T), _d(S), None, 0, C.BLANK)
    assert prep.dyn
    _, ws = op._forward(prep, with_beta=True)
    out = torch.full((3 * K * stride + guard,), 7, dtype=torch.int32, device=DEV)
    pc = torch.full((3 * K + guard,), 7.0, dtype=torch.float32, device=DEV)
    vp = ctypes.c_void_p
    st = L.load().mrnnt_sample(ctypes.byref(prep.problem), vp(ws.data_ptr()), K, 9, 0, vp(out.data_ptr()), stride,
                               vp(pc.data_ptr()), prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    o, c = out.cpu().numpy(), pc.cpu().numpy()
    assert np.all(o[3 * K * stride:] == 7) and np.all(c[3 * K:] == 7.0)
    o, c = o[:3 * K * stride].reshape(3, K, stride), c[:3 * K].reshape(3, K)
    assert np.all(o[1] == -1) and np.all(np.isnan(c[1]))
    for b in (0, 2):
        assert np.array_equal(o[b], full.alignments[b, :, :stride]) and c[b].tobytes() == full.path_costs[b].tobytes()
    op.check_lengths()


def test_graph_capture_with_device_lengths(op):
    """Forward + sample with device-resident lengths captured once and replayed twice on new logits (the default queue
    settings): the replayed result is the eager one."""
    rng = np.random.default_rng(15)
    acts, labels, T, S = C.ragged(rng, [(20, 6), (14, 14), (9, 0)], 16)
    other = rng.standard_normal(acts.shape).astype(np.float32)
    a, lab, Td, Sd = _d(acts), _d(labels), _d(T), _d(S)

    def step():
        return op.monotonic_rnnt_sample(a, lab, Td, Sd, 70, 33, max_input_length=20)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    a.copy_(_d(other))
    eager = run_gpu(other, labels, T, S, 70, 33, max_input_length=20, device_lengths=True)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert _same_bits([x.cpu().numpy() for x in static], eager)
    op.check_lengths()
