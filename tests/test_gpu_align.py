"""monotonic_rnnt_align on the MI355X (mrnnt_align, csrc/mrnnt_viterbi.hip): the shared checks of
tests/_align_checks.py on GPU tensors -- every dispatch boundary of the Viterbi launch, a path longer than one
backtrace chunk -- and what only the GPU path has: the padded layout, bf16 / fp16 acts, device-resident lengths,
their validation, HIP-graph capture, and the align -> restricted-loss round trip."""
import numpy as np
import pytest
import torch

import _align_checks as A
from _parity import assert_costs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def op():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _d(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gpu(acts, labels, T, S, alignment=None, k=0, max_input_length=None, device_lengths=False, dtype=None):
    import monotonic_rnnt_op as op
    a = _d(acts) if dtype is None else _d(acts).to(dtype)
    Tt, St = (_d(T), _d(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))
    al, costs = op.monotonic_rnnt_align(a, _d(labels), Tt, St, alignment=_d(alignment),
                                        max_distance_from_alignment=k, blank_label=A.BLANK,
                                        max_input_length=max_input_length)
    assert al.dtype == torch.int32 and costs.dtype == torch.float32 and al.is_cuda and costs.is_cuda
    return al.cpu().numpy(), costs.cpu().numpy()


def test_valid_and_cost_is_the_paths(op):
    rng = np.random.default_rng(1)
    acts, labels, T, S = A.ragged(rng, [(12, 4), (7, 0), (9, 9), (70, 64), (1, 1), (1, 0)], 8)
    al, _ = A.check_all(run_gpu, acts, labels, T, S)
    assert al.shape == (6, 70)


def test_optimal_against_the_oracle_tiny(op):
    A.check_optimal_tiny(run_gpu)


@pytest.mark.parametrize("W", [64, 65, 129, 257, 513, 1025])
def test_optimal_at_dispatch_boundaries(op, W):
    A.check_boundary(run_gpu, W)


@pytest.mark.parametrize("W", [1100, 1537])
def test_optimal_with_three_and_four_cells_per_lane(op, W):
    A.check_boundary(run_gpu, W, V=4)


def test_long_utterance_many_backtrace_chunks(op):
    """The backtrace has one form (64-frame chunks staged through LDS): 4200 frames are 66 of them, the last partial."""
    acts, labels, T, S = A.ragged(np.random.default_rng(9), [(4200, 64), (130, 3)], 4)
    al, costs = A.check_all(run_gpu, acts, labels, T, S)
    ref, _ = A.np_viterbi(acts, labels, T, S)
    assert_costs(costs, ref)


@pytest.mark.parametrize("T1,S1", [(40, 20), (150, 129)])
def test_exact_planted_path_and_cpu_identity(op, T1, S1):
    al, costs = A.check_exact_path(run_gpu, T1, S1)
    acts, labels, T, S, _ = A.planted_problem(T1, S1)
    cal, ccosts = A.run_cpu(acts, labels, T, S)
    assert np.array_equal(al, cal)
    assert_costs(costs, ccosts.astype(np.float64))


def test_restricting_alignment(op):
    A.check_restriction(run_gpu)


def test_value_domain(op):
    A.check_value_domain(run_gpu)


def test_strides(op):
    A.check_strides(run_gpu)


def _pack_to_padded(acts, T, S, pad_T, pad_S1, fill):
    off = A.offsets(T, S)
    out = np.full((len(T), pad_T, pad_S1, acts.shape[1]), fill, np.float32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    return out


def test_padded_layout_bit_identical_to_packed(op):
    rng = np.random.default_rng(10)
    acts, labels, T, S = A.ragged(rng, [(19, 7), (25, 11), (6, 0), (13, 13)], 16)
    al, costs = run_gpu(acts, labels, T, S, max_input_length=27)
    padded = _pack_to_padded(acts, T, S, 27, 15, 3.0)
    pal, pcosts = op.monotonic_rnnt_align(_d(padded), _d(labels), torch.from_numpy(T), torch.from_numpy(S))
    assert tuple(pal.shape) == (4, 27)
    assert np.array_equal(pal.cpu().numpy(), al) and pcosts.cpu().numpy().tobytes() == costs.tobytes()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_acts(op, dtype):
    rng = np.random.default_rng(11)
    acts, labels, T, S = A.ragged(rng, [(31, 12), (70, 66), (9, 0)], 24)
    low = torch.from_numpy(acts).to(dtype)
    up = low.to(torch.float32).numpy()  # the yardstick sees the inputs the kernel sees
    al, costs = run_gpu(acts, labels, T, S, dtype=dtype)
    A.check_valid(al, labels, T, S)
    ref, _ = A.np_viterbi(up, labels, T, S)
    assert_costs(costs, ref)
    A.check_cost_is_the_paths(al, costs, up, labels, T, S)


def test_device_lengths_bit_identical_to_host_lengths(op):
    rng = np.random.default_rng(12)
    acts, labels, T, S = A.ragged(rng, [(33, 9), (80, 70), (5, 0), (21, 21)], 12)
    al, costs = run_gpu(acts, labels, T, S, max_input_length=80)
    dal, dcosts = run_gpu(acts, labels, T, S, max_input_length=80, device_lengths=True)
    assert np.array_equal(dal, al) and dcosts.tobytes() == costs.tobytes()
    given = al.copy()  # restricted, and L taken from alignment.size(1)
    ral, rcosts = run_gpu(acts, labels, T, S, alignment=given, k=1)
    dral, drcosts = run_gpu(acts, labels, T, S, alignment=given, k=1, device_lengths=True)
    assert dral.shape == ral.shape == (4, 80)
    assert np.array_equal(dral, ral) and drcosts.tobytes() == rcosts.tobytes()
    op.check_lengths()
    with pytest.raises(RuntimeError, match="max_input_length"):
        op.monotonic_rnnt_align(_d(acts), _d(labels), _d(T), _d(S))


def test_invalid_device_lengths_fail_closed(op):
    op.check_lengths()  # nothing pending
    acts = torch.randn(8 + 12, 5, device=DEV)
    lab = torch.ones(2, 3, dtype=torch.int32, device=DEV)
    al, costs = op.monotonic_rnnt_align(acts, lab, torch.tensor([2, 4], device=DEV), torch.tensor([3, 2], device=DEV),
                                        max_input_length=6)  # S_0 > T_0
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    assert torch.isnan(costs).all() and bool((al == -1).all())
    op.check_lengths()  # reported once


def test_graph_capture_with_device_lengths(op):
    rng = np.random.default_rng(13)
    acts, labels, T, S = A.ragged(rng, [(20, 6), (14, 14), (9, 0)], 16)
    other = rng.standard_normal(acts.shape).astype(np.float32)
    a, lab, Td, Sd = _d(acts), _d(labels), _d(T), _d(S)

    def step():
        return op.monotonic_rnnt_align(a, lab, Td, Sd, max_input_length=20)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        al_static, c_static = step()
    a.copy_(_d(other))
    g.replay()
    torch.cuda.synchronize()
    eal, ec = run_gpu(other, labels, T, S, max_input_length=20, device_lengths=True)
    assert np.array_equal(al_static.cpu().numpy(), eal) and c_static.cpu().numpy().tobytes() == ec.tobytes()
    op.check_lengths()


def test_c_level_setup_kernel_null_costs_and_in_place(op):
    """mrnnt_align called directly: without a host-built lattice (the setup kernel builds the offsets), with
    costs_dev = NULL, and with p->alignment and alignment_out_dev the same buffer (documented as safe)."""
    import ctypes

    import _mrnnt_lib as L
    rng = np.random.default_rng(15)
    acts, labels, T, S = A.ragged(rng, [(23, 9), (17, 17), (12, 0)], 8)
    ref_al, _ = run_gpu(acts, labels, T, S)
    band_al, band_c = run_gpu(acts, labels, T, S, alignment=ref_al, k=1)
    a, lab, Tt, St = _d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S)
    vp = ctypes.c_void_p
    prep = op._Prepared(a, lab, Tt, St, None, 0, A.BLANK)
    prep.problem.lattice = None
    ws = prep.workspace()
    out = torch.full((3, 23), 7, dtype=torch.int32, device=DEV)
    st = L.load().mrnnt_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(out.data_ptr()), 23, None,
                              prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref_al)
    prep = op._Prepared(a, lab, Tt, St, out, 1, A.BLANK)
    assert prep.alignment.data_ptr() == out.data_ptr()
    prep.problem.lattice = None
    ws = prep.workspace()
    costs = torch.empty(3, dtype=torch.float32, device=DEV)
    st = L.load().mrnnt_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(out.data_ptr()), 23,
                              vp(costs.data_ptr()), prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), band_al) and costs.cpu().numpy().tobytes() == band_c.tobytes()
    st = L.load().mrnnt_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(out.data_ptr()), 22, None,
                              prep.stream())
    assert st == L.RNNT_STATUS_INVALID_VALUE and b"row stride" in L.load().mrnnt_last_error()


def test_round_trip_into_the_restricted_loss(op):
    """The loop the feature closes: the alignment fed back as alignment= with k = 0 leaves that one path, whose loss
    is the align call's cost."""
    rng = np.random.default_rng(14)
    acts, labels, T, S = A.ragged(rng, [(40, 15), (90, 80), (12, 0), (7, 7)], 32)
    a, lab, Tt, St = _d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S)
    al, costs = op.monotonic_rnnt_align(a, lab, Tt, St)
    loss = op.monotonic_rnnt_loss(a, lab, Tt, St, alignment=al, max_distance_from_alignment=0)
    assert_costs(loss.cpu().numpy(), costs.cpu().numpy().astype(np.float64))
    full = op.monotonic_rnnt_loss(a, lab, Tt, St)
    assert bool((full <= costs + 1e-4 * costs.abs().clamp(min=1)).all())
