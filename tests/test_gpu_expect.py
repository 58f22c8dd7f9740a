"""monotonic_rnnt_expected_cost on the MI355X (mrnnt_expect_forward / mrnnt_expect_backward, csrc/mrnnt_expect.hip): the
shared checks of tests/_expect_checks.py on GPU tensors, and what only the GPU path has: bf16 / fp16 acts, an unaligned
acts pointer (the scalar kernels), device-resident lengths and their validation, HIP-graph capture, results equal to
the host implementation's, and the tracked backward (the row state of mrnnt_backward_tracked)."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import _expect_checks as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def op():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _d(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gpu(acts, labels, T, S, wb, we, ge=None, gc=None, alignment=None, k=0, dtype=None, device_lengths=False,
            unaligned=False):
    import monotonic_rnnt_op as op
    a = _d(acts) if dtype is None else _d(acts).to(dtype)
    if unaligned:  # rows that start 4 bytes past a 16-byte boundary: the scalar kernels
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=DEV)
        buf[1:].copy_(a.reshape(-1))
        a = buf[1:].view(a.shape)
        assert a.data_ptr() % 16 != 0 and a.is_contiguous()
    a.requires_grad_(True)
    Tt, St = (_d(T), _d(S)) if device_lengths else (torch.from_numpy(T), torch.from_numpy(S))
    e, c = op.monotonic_rnnt_expected_cost(a, _d(labels), Tt, St, _d(wb), _d(we), _d(alignment), k, C.BLANK)
    B = len(T)
    assert e.is_cuda and c.is_cuda and e.dtype == torch.float32 and c.dtype == torch.float32
    assert e.shape == (B,) and c.shape == (B,) and e.requires_grad and c.requires_grad
    one = torch.ones(B, device=DEV)
    torch.autograd.backward((e, c), (one if ge is None else _d(np.asarray(ge, np.float32)),
                                     one if gc is None else _d(np.asarray(gc, np.float32))))
    assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
    return e.detach().cpu().numpy(), c.detach().cpu().numpy(), a.grad.float().cpu().numpy()


Post = collections.namedtuple("Post", ["blank", "label"])


def posteriors_gpu(acts, labels, T, S, alignment=None, k=0):
    import monotonic_rnnt_op as op
    p = op.monotonic_rnnt_posteriors(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S), _d(alignment), k,
                                     C.BLANK)
    return Post(p.blank.cpu().numpy(), p.label.cpu().numpy())


def loss_gpu(acts, labels, T, S, gc):
    import monotonic_rnnt_op as op
    a = _d(acts).requires_grad_(True)
    c = op.monotonic_rnnt_loss(a, _d(labels), torch.from_numpy(T), torch.from_numpy(S), None, 0, C.BLANK)
    c.backward(_d(np.asarray(gc, np.float32)))
    return c.detach().cpu().numpy(), a.grad.cpu().numpy().astype(np.float64)


def _same(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


@pytest.mark.parametrize("V", [5, 8])
def test_brute_force(op, V):
    C.check_brute(run_gpu, V)


@pytest.mark.parametrize("name", [c[0] for c in C.EDGE_CASES])
def test_edge_shapes_against_the_yardstick(op, name):
    C.check_edge_case(run_gpu, name)


@pytest.mark.parametrize("dtype,eps", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
@pytest.mark.parametrize("name", ["scalar_v5", "v32", "v1024"])
def test_reduced_precision_acts(op, name, dtype, eps):
    """bf16 / fp16 acts and grads: the yardstick on the upcast values, plus one rounding of the output type. V = 5 is
    the scalar path (V % 8 != 0), V = 32 / 1024 the vector path."""
    acts, labels, T, S, wb, we, ge, gc = C.edge_problem(name)
    up = torch.from_numpy(acts).to(dtype).to(torch.float32).numpy()
    C.check_against_yardstick(run_gpu, acts, labels, T, S, wb, we, ge, gc, eps=eps, yard_acts=up, dtype=dtype)


def test_unaligned_acts_take_the_scalar_path(op):
    C.check_against_yardstick(run_gpu, *C.edge_problem("v32"), unaligned=True)


def test_expected_is_the_posteriors_weighted_cost(op):
    C.check_posteriors_identity(run_gpu, posteriors_gpu)


def test_costs_output_is_the_loss(op):
    C.check_costs_identity(run_gpu, loss_gpu)


def test_constant_costs(op):
    C.check_constant_costs(run_gpu)


def test_negated_costs(op):
    C.check_negation(run_gpu)


def test_two_upstreams_in_one_pass(op):
    C.check_two_upstreams(run_gpu)


def test_restricting_alignment(op):
    C.check_restriction(run_gpu, posteriors_gpu)


def test_non_finite_logits(op):
    C.check_non_finite(run_gpu)


@pytest.mark.parametrize("V", [12, 7])
def test_padded_layout_bit_identical_to_packed(op, V):
    C.check_padded(run_gpu, V)


def test_reproducible_batch_independent_and_equal_to_the_host_implementation(op):
    acts, labels, T, S, wb, we, ge, gc, (e, c, g) = C.check_reproducible(run_gpu)
    he, hc, hg = C.run_cpu(acts, labels, T, S, wb, we, ge, gc)
    Wb = C.cost_bound(wb, we, T, S)
    C.assert_expected(e, he.astype(np.float64), Wb)
    C.assert_costs(c, hc.astype(np.float64))
    C.assert_grads(g, hg.astype(np.float64), C.grad_tol(T, S, Wb, ge, gc))


def test_forward_without_a_gradient_and_absent_cost_arrays(op):
    """Without requires_grad only the A direction runs (no beta, no Bk): the same values. A cost array that is None is
    an array of zeros, bit for bit."""
    acts, labels, T, S, wb, we = C.small_problem(seed=85)
    ref = run_gpu(acts, labels, T, S, wb, we)
    e, c = op.monotonic_rnnt_expected_cost(_d(acts), _d(labels), torch.from_numpy(T), torch.from_numpy(S), _d(wb), _d(we))
    assert not e.requires_grad and not c.requires_grad
    C.assert_expected(e.cpu().numpy(), ref[0].astype(np.float64), C.cost_bound(wb, we, T, S))
    C.assert_costs(c.cpu().numpy(), ref[1].astype(np.float64))
    zero = np.zeros_like(wb)
    for x, y, xz, yz in ((None, we, zero, we), (wb, None, wb, zero), (None, None, zero, zero)):
        r = run_gpu(acts, labels, T, S, x, y)
        assert _same(r, run_gpu(acts, labels, T, S, xz, yz))
    assert np.all(r[0] == 0.0)


def test_device_lengths_give_the_host_lengths_bits(op):
    for name in ("scalar_v5", "v32", "waves_v8"):
        prob = C.edge_problem(name)
        assert _same(run_gpu(*prob, device_lengths=True), run_gpu(*prob))
    acts, labels, T, S, wb, we = C.small_problem(seed=80)
    pad = lambda x: C.pack_to_padded(x, T, S, 31, 19, np.nan)  # noqa: E731
    args = (pad(acts), labels, T, S, pad(wb[:, None])[..., 0], pad(we[:, None])[..., 0])
    assert _same(run_gpu(*args, device_lengths=True), run_gpu(*args))
    op.check_lengths()


def test_invalid_device_lengths_fail_closed(op):
    op.check_lengths()  # nothing pending
    acts, labels, T, S, wb, we = C.small_problem(seed=81)
    Tb, Sb = np.array([2, 4], np.int32), np.array([3, 2], np.int32)  # S_0 > T_0
    x = _d(acts[:20]).requires_grad_(True)
    e, c = op.monotonic_rnnt_expected_cost(x, _d(labels[:2]), _d(Tb), _d(Sb), _d(wb[:20]), _d(we[:20]))
    (e + c).sum().backward()
    with pytest.raises(RuntimeError, match="failed validation"):
        op.check_lengths()
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(c).all()) and bool(torch.isnan(x.grad).all())
    op.check_lengths()  # reported once


def test_graph_capture_with_device_lengths(op):
    """Forward + backward with device-resident lengths captured once and replayed twice on new logits (the default
    queue settings): the replayed values and gradients are the eager bits."""
    acts, labels, T, S, wb, we = C.small_problem(seed=82, V=16)
    ge, gc = C.upstreams(np.random.default_rng(83), len(T))
    other = np.random.default_rng(84).standard_normal(acts.shape).astype(np.float32)
    a = _d(acts).requires_grad_(True)
    lab, Td, Sd, wbd, wed, ged, gcd = _d(labels), _d(T), _d(S), _d(wb), _d(we), _d(ge), _d(gc)

    def step():
        e, c = op.monotonic_rnnt_expected_cost(a, lab, Td, Sd, wbd, wed)
        torch.autograd.backward((e, c), (ged, gcd))
        return e, c

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
        se, sc = step()
    with torch.no_grad():
        a.copy_(_d(other))
    eager = run_gpu(other, labels, T, S, wb, we, ge, gc, device_lengths=True)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert _same((se.detach().cpu().numpy(), sc.detach().cpu().numpy(), a.grad.cpu().numpy()), eager)
    op.check_lengths()


# ---- the tracked backward (in the form of tests/test_gpu_zero_rows.py) ------------------------------------------------

SENTINEL = 0x7FC0BEEF  # a NaN no kernel writes


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Case:
    """One problem after mrnnt_expect_forward: plain() / tracked() call the C entries on it."""

    def __init__(self, op, lengths, V, seed, peak=30.0, pad=None):
        import _mrnnt_lib as L
        self.op, self.L, self.V = op, L, V
        self.T, self.S = (np.asarray(x, np.int32) for x in lengths)
        rng = np.random.default_rng(seed)
        shapes = list(zip(self.T.tolist(), self.S.tolist()))
        acts, labels, _, _ = C.ragged(rng, shapes, V)
        acts *= peak  # peaked logits: dead rows inside the band
        wb, we = C.random_costs(rng, self.T, self.S)
        self.pad = pad
        if pad is not None:
            fill = lambda x: C.pack_to_padded(x, self.T, self.S, pad[0], pad[1], np.nan)  # noqa: E731
            acts, wb, we = fill(acts), fill(wb[:, None])[..., 0], fill(we[:, None])[..., 0]
        self.acts, self.wb, self.we = _d(acts), _d(wb), _d(we)
        self.ge, self.gc = (_d(x) for x in C.upstreams(rng, len(self.T)))
        self.prep = op._Prepared(self.acts, _d(labels), torch.from_numpy(self.T), torch.from_numpy(self.S), None, 0, 0)
        self.rows = int(self.prep.problem.num_rows)
        self.ws = self.prep.workspace(expect=True)
        op._call(self.prep, "expect_forward", vp(self.ws), self.ws.numel(), vp(self.wb), vp(self.we), None, None, 1,
                 pending=True)

    def _run(self, grads, state, state_len):
        p, lib = ctypes.byref(self.prep.problem), self.L.load()
        args = [p, vp(self.ws), self.ws.numel(), vp(self.wb), vp(self.we), vp(self.ge), vp(self.gc), vp(grads)]
        if state is None:
            st = lib.mrnnt_expect_backward(*args, self.prep.stream())
        else:
            st = lib.mrnnt_expect_backward_tracked(*args, vp(state), state_len, self.prep.stream())
        torch.cuda.synchronize()
        return st

    def plain(self):
        g = torch.empty(self.rows, self.V, dtype=torch.float32, device=DEV)
        self.L.check(self._run(g, None, 0), "expect_backward")
        return g.view(torch.int32).cpu().numpy()

    def tracked(self, ibuf, state):
        self.L.check(self._run(ibuf, state, state.numel()), "expect_backward_tracked")

    def out_of_band(self):
        """Per row of grads: outside the monotonic band (padding rows included)."""
        out = []
        pT, pS1 = self.pad if self.pad is not None else (0, 0)
        for Tb, Sb in zip(self.T, self.S):
            t, s = np.meshgrid(np.arange(pT or Tb), np.arange(pS1 or Sb + 1), indexing="ij")
            inb = (t < Tb) & (s <= Sb) & (s >= np.maximum(0, t - (Tb - Sb))) & (s <= np.minimum(t, Sb))
            out.append(~inb.reshape(-1))
        return np.concatenate(out)


def _protocol(c1, c2):
    rows = max(c1.rows, c2.rows) + 3
    ibuf = torch.full((rows, c1.V), SENTINEL, dtype=torch.int32, device=DEV)
    state = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    # 1. nothing vouched for: the plain result, a truthful state, nothing touched past the rows covered
    c1.tracked(ibuf, state)
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    assert np.array_equal(got[:c1.rows], c1.plain())
    assert np.all(got[c1.rows:] == SENTINEL) and np.all(st[c1.rows:] == 0)
    assert np.all(got[:c1.rows][st[:c1.rows] == 1] == 0) and np.all(st <= 1)
    oob = c1.out_of_band()
    assert oob.any() and np.all(st[:c1.rows][oob] == 1), "out-of-band rows without a state: nothing would be skipped"
    live = st[:c1.rows] == 0
    assert live.any() and np.any(got[:c1.rows][live] != 0)
    assert np.any((st[:c1.rows] == 1) & ~oob), "no dead row inside the band: the case does not exercise it"
    # 2. vandalise every row the state vouches for, then another problem into the same buffer
    before = st.copy()
    ibuf[torch.from_numpy(before != 0).to(DEV)] = SENTINEL
    snap = ibuf.cpu().numpy()
    c2.tracked(ibuf, state)
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    ref, n = c2.plain(), c2.rows
    kept = (before != 0) & (st == before)
    kept[n:] = False
    assert kept.any(), "no row kept its state: the case does not exercise the skip"
    assert np.all(got[kept] == SENTINEL), "a row the state vouched for was stored again"
    assert np.all(ref[kept[:n]] == 0), "a skipped row is not the zero plain writes"
    assert np.array_equal(got[:n][~kept[:n]], ref[~kept[:n]])
    assert np.array_equal(got[n:], snap[n:]) and np.array_equal(st[n:], before[n:])
    assert np.all(got[:n][(st[:n] == 1) & ~kept[:n]] == 0)


@pytest.mark.parametrize("V", [1024, 256])
def test_tracked_backward_is_the_plain_one_and_keeps_the_row_state(op, V):
    _protocol(Case(op, ((9, 5, 12), (3, 5, 0)), V, seed=90), Case(op, ((10, 6, 8), (4, 2, 1)), V, seed=91))


def test_tracked_backward_across_the_256_row_segment_and_padded(op):
    _protocol(Case(op, ((262,), (260,)), 64, seed=92), Case(op, ((261,), (257,)), 64, seed=93))
    _protocol(Case(op, ((9, 5, 12), (3, 5, 0)), 256, seed=94, pad=(13, 7)),
              Case(op, ((10, 6, 8), (4, 2, 1)), 256, seed=95, pad=(13, 7)))


def test_row_state_too_short_is_refused(op):
    import _mrnnt_lib as L
    c = Case(op, ((9, 5, 12), (3, 5, 0)), 256, seed=96)
    ibuf = torch.full((c.rows, c.V), SENTINEL, dtype=torch.int32, device=DEV)
    state = torch.zeros(c.rows, dtype=torch.uint8, device=DEV)
    assert c._run(ibuf, state, c.rows - 1) == L.RNNT_STATUS_INVALID_VALUE
    assert torch.all(ibuf == SENTINEL) and int(state.sum()) == 0  # before any device call
