"""monotonic_rnnt_posteriors on the MI355X (mrnnt_posteriors, csrc/mrnnt_posterior.hip): the shared checks of
tests/_posterior_checks.py on GPU tensors -- the width boundaries of the column and label-time workgroups, a long thin
utterance -- and what only the GPU path has: parity with the host implementation, the padded layout, bf16 / fp16
acts, device-resident lengths, their validation, output strides shorter than an utterance, run-to-run bit identity and
HIP-graph capture."""
import ctypes

import numpy as np
import pytest
import torch

import _posterior_checks as P
from _parity import GRAD_TOL, assert_costs

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
    out = op.monotonic_rnnt_posteriors(a, _d(labels), Tt, St, alignment=_d(alignment), max_distance_from_alignment=k,
                                       blank_label=P.BLANK, max_input_length=max_input_length)
    assert out._fields == P.Posteriors._fields
    assert all(x.dtype == torch.float32 and x.is_cuda and not x.requires_grad for x in out)
    assert out.blank.shape == a.shape[:-1] and out.label.shape == a.shape[:-1]
    return P.Posteriors(*(x.cpu().numpy() for x in out))


def _same_bits(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


def test_brute_force_on_tiny_shapes(op):
    P.check_brute_force_tiny(run_gpu)


def test_gradient_identity_against_the_oracle(op):
    P.check_gradient_identity(run_gpu)


@pytest.mark.parametrize("W", [2, 64, 65, 257, 1025])
def test_width_boundaries(op, W):
    """S + 1 = W around the 64 lanes of a column's wave and the 16-label tiles of the label sums; each batch has
    T = S + 3 and short utterances with S = 0 and S = T."""
    P.check_boundary(run_gpu, W)


def test_long_thin_utterance(op):
    """(300, 5) with (1, 0) and (1, 1): 296 frames per label sum, more than the 64 frame groups of a workgroup."""
    P.check_all(run_gpu, *P.long_thin_problem())


def test_restricting_alignment(op):
    P.check_restriction(run_gpu)


def test_value_domain(op):
    P.check_value_domain(run_gpu)


def test_strides(op):
    P.check_strides(run_gpu)


def test_gpu_equals_cpu_within_the_tolerances(op):
    acts, labels, T, S = P.ragged(np.random.default_rng(31), [(40, 15), (90, 80), (12, 0), (7, 7), (130, 3)], 32)
    g = run_gpu(acts, labels, T, S)
    c = P.run_cpu(acts, labels, T, S)
    assert np.abs(g.blank - c.blank).max() <= GRAD_TOL and np.abs(g.label - c.label).max() <= GRAD_TOL
    assert np.abs(g.emit - c.emit).max() <= GRAD_TOL
    for b, Tb in enumerate(T):
        assert np.abs(g.label_time[b] - c.label_time[b]).max() <= GRAD_TOL * max(1, int(Tb))
    assert np.array_equal(g.label_time == -1.0, c.label_time == -1.0)
    assert_costs(g.costs, c.costs.astype(np.float64))


def test_two_identical_calls_are_bitwise_equal(op):
    acts, labels, T, S = P.ragged(np.random.default_rng(32), [(200, 70), (64, 64), (33, 0), (90, 17)], 16)
    assert _same_bits(run_gpu(acts, labels, T, S), run_gpu(acts, labels, T, S))


def _pack_to_padded(acts, T, S, pad_T, pad_S1, fill):
    off = P.offsets(T, S)
    out = np.full((len(T), pad_T, pad_S1, acts.shape[1]), fill, np.float32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        out[b, :Tb, :Sb + 1] = acts[off[b]:off[b + 1]].reshape(Tb, Sb + 1, -1)
    return out


def test_padded_layout_identical_to_packed_and_zero_on_padding(op):
    acts, labels, T, S = P.ragged(np.random.default_rng(10), [(19, 7), (25, 11), (6, 0), (13, 13)], 16)
    res = run_gpu(acts, labels, T, S, max_input_length=27)
    off = P.offsets(T, S)
    padded = _pack_to_padded(acts, T, S, 27, 15, 3.0)
    out = op.monotonic_rnnt_posteriors(_d(padded), _d(labels), torch.from_numpy(T), torch.from_numpy(S))
    assert tuple(out.blank.shape) == (4, 27, 15) and tuple(out.emit.shape) == (4, 27)
    for name in ("blank", "label"):
        got, want = getattr(out, name).cpu().numpy(), np.zeros((4, 27, 15), np.float32)
        for b, (Tb, Sb) in enumerate(zip(T, S)):
            want[b, :Tb, :Sb + 1] = getattr(res, name)[off[b]:off[b + 1]].reshape(Tb, Sb + 1)
        assert got.tobytes() == want.tobytes(), name
    assert out.emit.cpu().numpy().tobytes() == res.emit.tobytes()
    assert out.label_time.cpu().numpy().tobytes() == res.label_time.tobytes()
    assert out.costs.cpu().numpy().tobytes() == res.costs.tobytes()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_acts(op, dtype):
    acts, labels, T, S = P.ragged(np.random.default_rng(11), [(31, 12), (70, 66), (9, 0)], 24)
    up = torch.from_numpy(acts).to(dtype).to(torch.float32).numpy()  # the yardstick sees the inputs the kernel sees
    res = run_gpu(acts, labels, T, S, dtype=dtype)
    ref, _ = P.np_posteriors(up, labels, T, S)
    P.compare(res, ref, T, S)
    P.check_invariants(res, T, S)


def test_device_lengths_bit_identical_to_host_lengths(op):
    acts, labels, T, S = P.ragged(np.random.default_rng(12), [(33, 9), (80, 70), (5, 0), (21, 21)], 12)
    res = run_gpu(acts, labels, T, S, max_input_length=80)
    assert _same_bits(run_gpu(acts, labels, T, S, max_input_length=80, device_lengths=True), res)
    given = np.full((4, 80), P.BLANK, np.int32)
    rng = np.random.default_rng(13)
    for b in range(4):
        given[b, np.sort(rng.choice(int(T[b]), int(S[b]), replace=False))] = labels[b, :S[b]]
    r = run_gpu(acts, labels, T, S, alignment=given, k=2)
    dr = run_gpu(acts, labels, T, S, alignment=given, k=2, device_lengths=True)  # L from alignment.size(1)
    assert dr.emit.shape == (4, 80) and _same_bits(dr, r)
    op.check_lengths()
    with pytest.raises(RuntimeError, match="max_input_length"):
        op.monotonic_rnnt_posteriors(_d(acts), _d(labels), _d(T), _d(S))


def test_invalid_device_lengths_fail_closed(op):
    op.check_lengths()  # nothing pending
    acts = torch.randn(8 + 12, 5, device=DEV)
    lab = torch.ones(2, 3, dtype=torch.int32, device=DEV)
    out = op.monotonic_rnnt_posteriors(acts, lab, torch.tensor([2, 4], device=DEV), torch.tensor([3, 2], device=DEV),
                                       max_input_length=6)  # S_0 > T_0
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    assert tuple(out.blank.shape) == (20,) and tuple(out.emit.shape) == (2, 6) and tuple(out.label_time.shape) == (2, 3)
    assert all(bool(torch.isnan(x).all()) for x in out)
    op.check_lengths()  # reported once


def test_device_lengths_with_a_short_emit_stride(op):
    """An emit row stride below a T_b (device-resident lengths: the host cannot check it): that utterance's row is NaN,
    the others are unaffected, nothing is written past the buffer (a guard region follows it) and the status word is
    raised."""
    import _mrnnt_lib as L
    op.check_lengths()
    acts, labels, T, S = P.ragged(np.random.default_rng(14), [(9, 3), (14, 6), (5, 0)], 8)
    full = run_gpu(acts, labels, T, S)
    a, lab = _d(acts), _d(labels)
    prep = op._Prepared(a, lab, _d(T), _d(S), None, 0, P.BLANK)
    assert prep.dyn
    _, ws = op._forward(prep, with_beta=True)
    stride, guard = 10, 64
    emit = torch.full((3 * stride + guard,), 7.0, dtype=torch.float32, device=DEV)
    ltime = torch.full((3 * 6 + guard,), 7.0, dtype=torch.float32, device=DEV)
    vp = ctypes.c_void_p
    st = L.load().mrnnt_posteriors(ctypes.byref(prep.problem), vp(ws.data_ptr()), None, None, vp(emit.data_ptr()),
                                   stride, vp(ltime.data_ptr()), 6, prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    e, lt = emit.cpu().numpy(), ltime.cpu().numpy()
    assert np.all(e[3 * stride:] == 7.0) and np.all(lt[18:] == 7.0)
    e = e[:3 * stride].reshape(3, stride)
    assert np.all(np.isnan(e[1]))
    assert e[0].tobytes() == full.emit[0, :stride].tobytes() and e[2].tobytes() == full.emit[2, :stride].tobytes()
    assert lt[:18].tobytes() == full.label_time.tobytes()
    op.check_lengths()


def test_graph_capture_with_device_lengths(op):
    rng = np.random.default_rng(15)
    acts, labels, T, S = P.ragged(rng, [(20, 6), (14, 14), (9, 0)], 16)
    other = rng.standard_normal(acts.shape).astype(np.float32)
    a, lab, Td, Sd = _d(acts), _d(labels), _d(T), _d(S)

    def step():
        return op.monotonic_rnnt_posteriors(a, lab, Td, Sd, max_input_length=20)

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
    g.replay()
    torch.cuda.synchronize()
    eager = run_gpu(other, labels, T, S, max_input_length=20, device_lengths=True)
    assert _same_bits([x.cpu().numpy() for x in static], eager)
    op.check_lengths()
