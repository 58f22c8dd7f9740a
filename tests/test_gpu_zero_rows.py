"""mrnnt_backward_tracked / mrnnt_path_backward_tracked on the MI355X: the gradient into a buffer whose rows the caller
vouches for (one state byte per row: 0 unknown, 1 all +0.0, 2 all -0.0). The yardstick is mrnnt_backward into a fresh
buffer, compared bitwise on integer views (signs of zero and NaN payloads included).

Protocol, on one buffer and one state (protocol()):
  1. state all 0, buffer filled with a NaN sentinel: the result equals plain, the state is truthful.
  2. every row with a non-zero state is overwritten with the sentinel (the state kept), and another problem -- other
     lengths and logits, so the band and the dead set move -- runs into the same buffer: a row whose state is the same
     non-zero code before and after still holds the sentinel (a build that ignores the state fails here) and plain has
     the zero the code names there; every other row equals plain.
  3. after each launch: state 1 => the row is all 0x0, state 2 => all sign bits, every out-of-band row of an utterance
     with a finite log-likelihood and a finite scale has a non-zero state, bytes past the rows covered are untouched.

Shapes: every case holds out-of-band, dead (peaked logits: 1000 * N(0, 1)) and live rows, asserted with
mrnnt_grad_live_rows. B = 3, T = (9, 5, 12), S = (3, 5, 0): a wide band, the S = T diagonal and S = 0; f32 V = 1024 /
512 / 256 are the three (vectors per lane, rows per wave) ladders of the staged kernel (1, 2 and 4 rows per wave: live
and skipped rows in one wave iteration, ragged tails), bf16 V = 1024; T = 262, S = 260, V = 64 crosses the 256-row
segment."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SENTINEL = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FC1}  # NaNs no kernel writes
NEG_ZERO = {torch.float32: -(1 << 31), torch.bfloat16: -(1 << 15)}
WIDE = ((9, 5, 12), (3, 5, 0))
WIDE2 = ((10, 6, 8), (4, 2, 1))  # other lengths: 84 rows against 78


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


@pytest.fixture(scope="module")
def L():
    import _mrnnt_lib
    return _mrnnt_lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Case:
    """One problem after its forward: plain() / tracked() call the C entries on it."""

    def __init__(self, op, L, dev, lengths, V, dtype=torch.float32, seed=0, peak=1000.0, pad=None, device_lengths=None,
                 no_path=None, path_late=None):
        self.op, self.L, self.dev, self.dtype, self.V = op, L, dev, dtype, V
        self.T, self.S = (np.asarray(x, np.int32) for x in lengths)
        B = self.T.size
        g = torch.Generator().manual_seed(seed)
        n = int(np.sum(self.T * (self.S + 1)))
        acts = torch.randn(n, V, generator=g) * peak
        if no_path is not None:  # every path of this utterance needs a blank (T > S): none survives, ll = -inf
            off = np.concatenate([[0], np.cumsum(self.T * (self.S + 1))])
            acts[off[no_path]:off[no_path + 1], 0] = float("-inf")
        self.labels = torch.randint(1, V, (B, max(1, int(self.S.max()))), generator=g, dtype=torch.int32)
        self.pad = pad
        if pad is not None:  # the padded layout, NaN in every padding row
            pT, pS1 = pad
            full = torch.full((B, pT, pS1, V), float("nan"))
            o = 0
            for b in range(B):
                Tb, Sb = int(self.T[b]), int(self.S[b])
                full[b, :Tb, :Sb + 1] = acts[o:o + Tb * (Sb + 1)].view(Tb, Sb + 1, V)
                o += Tb * (Sb + 1)
            acts = full
        self.acts = acts.to(dtype).to(dev)
        Tt, St = torch.from_numpy(self.T), torch.from_numpy(self.S)
        if device_lengths is not None:  # GPU-resident lengths (possibly not the ones acts was laid out for)
            Tt, St = (torch.tensor(x, dtype=torch.int32, device=dev) for x in device_lengths)
        self.prep = op._Prepared(self.acts, self.labels.to(dev), Tt, St, None, 0, 0)
        self.rows = int(self.prep.problem.num_rows)
        self.paths = None
        if path_late is None:
            _, self.ws = op._forward(self.prep, with_beta=True)
        else:  # path scores of one alignment per utterance: [B, 1, L] alignment rows
            self.paths = _paths(self.T, self.S, self.labels, path_late).to(dev).contiguous()
            K, Lp = self.paths.size(1), self.paths.size(2)
            self.ws = self.prep.workspace(num_paths=K)
            op._call(self.prep, "path_forward", vp(self.ws), self.ws.numel(), vp(self.paths), K, Lp, None, pending=True)

    def _run(self, grads, scale, state, state_len):
        p, lib = ctypes.byref(self.prep.problem), self.L.load()
        sc = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=self.dev)
        if self.paths is not None:
            K, Lp = self.paths.size(1), self.paths.size(2)
            sc = None if sc is None else sc.view(-1, 1).expand(-1, K).contiguous()
            if state is None:
                st = lib.mrnnt_path_backward(p, vp(self.ws), self.ws.numel(), vp(self.paths), K, Lp, vp(sc), vp(grads),
                                             self.prep.stream())
            else:
                st = lib.mrnnt_path_backward_tracked(p, vp(self.ws), self.ws.numel(), vp(self.paths), K, Lp, vp(sc),
                                                     vp(grads), vp(state), state_len, self.prep.stream())
        elif state is None:
            st = lib.mrnnt_backward(p, vp(self.ws), vp(sc), vp(grads), self.prep.stream())
        else:
            st = lib.mrnnt_backward_tracked(p, vp(self.ws), vp(sc), vp(grads), vp(state), state_len, self.prep.stream())
        torch.cuda.synchronize()
        return st

    def plain(self, scale=None):
        """The yardstick: mrnnt_backward into a fresh buffer, as [rows, V] integers."""
        g = torch.empty(self.rows, self.V, dtype=self.dtype, device=self.dev)
        self.L.check(self._run(g, scale, None, 0), "backward")
        return g.view(INT[self.dtype]).cpu().numpy()

    def tracked(self, ibuf, state, scale=None):
        assert ibuf.is_contiguous() and ibuf.size(0) >= self.rows and state.numel() == ibuf.size(0)
        self.L.check(self._run(ibuf, scale, state, state.numel()), "backward_tracked")

    def live_rows(self):
        cnt = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.L.check(self.L.load().mrnnt_grad_live_rows(ctypes.byref(self.prep.problem), vp(self.ws), vp(cnt),
                                                        self.prep.stream()), "grad_live_rows")
        return int(cnt.item())

    def geometry(self):
        """Per row of grads: its utterance (-1: a padding row) and whether it lies in the monotonic band."""
        utt, band = [], []
        B = self.T.size
        pT, pS1 = self.pad if self.pad is not None else (0, 0)
        for b in range(B):
            Tb, Sb = int(self.T[b]), int(self.S[b])
            t, s = np.meshgrid(np.arange(pT or Tb), np.arange(pS1 or Sb + 1), indexing="ij")
            real = (t < Tb) & (s <= Sb)
            utt.append(np.where(real, b, -1).reshape(-1))
            band.append((real & (s >= np.maximum(0, t - (Tb - Sb))) & (s <= np.minimum(t, Sb))).reshape(-1))
        return np.concatenate(utt), np.concatenate(band)

    def assert_mixed(self):
        """The case holds out-of-band, dead and live rows."""
        utt, band = self.geometry()
        live, inband = self.live_rows(), int(band.sum())
        print(f"rows {self.rows}: in band {inband}, live {live}")
        assert 0 < live < inband < int((utt >= 0).sum())


def new_buffer(dev, rows, V, dtype):
    ibuf = torch.full((rows, V), SENTINEL[dtype], dtype=INT[dtype], device=dev)
    return ibuf, torch.zeros(rows, dtype=torch.uint8, device=dev)


def assert_truthful(case, rows_np, st, finite=None, skip=None):
    """State 1 / 2 name what the row holds; out-of-band (and padding) rows of finite utterances have a state."""
    n = case.rows
    dt = case.dtype
    chk = np.ones(n, bool) if skip is None else ~skip[:n]
    assert np.all(rows_np[:n][chk & (st[:n] == 1)] == 0)
    assert np.all(rows_np[:n][chk & (st[:n] == 2)] == NEG_ZERO[dt])
    assert np.all(st[:n] <= 2)
    utt, band = case.geometry()
    fin = np.ones(case.T.size, bool) if finite is None else np.asarray(finite)
    oob = (utt >= 0) & ~band & fin[np.maximum(utt, 0)]
    assert oob.any() and np.all(st[:n][oob] != 0), "out-of-band rows without a state: nothing would be skipped"
    assert np.all(st[:n][utt < 0] == 1)  # padding rows hold +0


def protocol(c1, c2, scale1=None, scale2=None, finite=None):
    rows = max(c1.rows, c2.rows) + 3
    ibuf, state = new_buffer(c1.dev, rows, c1.V, c1.dtype)
    sent = SENTINEL[c1.dtype]
    # 1. nothing vouched for
    c1.tracked(ibuf, state, scale1)
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    assert np.array_equal(got[:c1.rows], c1.plain(scale1))
    assert np.all(got[c1.rows:] == sent) and np.all(st[c1.rows:] == 0)
    assert_truthful(c1, got, st, finite=finite)
    # 2. vandalise every row the state vouches for, then another problem into the same buffer
    before = st.copy()
    ibuf[torch.from_numpy(before != 0).to(ibuf.device)] = sent
    snap = ibuf.cpu().numpy()
    c2.tracked(ibuf, state, scale2)
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    ref = c2.plain(scale2)
    n = c2.rows
    kept = (before != 0) & (st == before)
    kept[n:] = False
    print(f"rows {n}: {int(kept.sum())} skipped, {int((st[:n] != 0).sum())} zero rows")
    assert kept.any(), "no row kept its state: the case does not exercise the skip"
    assert np.all(got[kept] == sent), "a row the state vouched for was stored again"
    want = np.where(st[kept] == 1, 0, NEG_ZERO[c1.dtype])
    assert np.all(ref[kept[:n]] == want[:, None]), "a skipped row is not the zero plain writes"
    other = ~kept[:n]
    assert np.array_equal(got[:n][other], ref[other])
    assert np.array_equal(got[n:], snap[n:]) and np.array_equal(st[n:], before[n:])  # rows past the call: left alone
    assert_truthful(c2, got, st, finite=finite, skip=kept)
    return got, st


@pytest.mark.parametrize("V,dtype", [(1024, torch.float32), (512, torch.float32), (256, torch.float32),
                                     (1024, torch.bfloat16)], ids=["f32_v1024", "f32_v512", "f32_v256", "bf16_v1024"])
def test_wide_band_diagonal_and_s0(op, L, dev, V, dtype):
    c1 = Case(op, L, dev, WIDE, V, dtype, seed=1)
    c2 = Case(op, L, dev, WIDE2, V, dtype, seed=2)
    c1.assert_mixed()
    c2.assert_mixed()
    protocol(c1, c2)
    protocol(c2, c1, scale1=[0.5, 2.0, 1.0])


def test_across_the_256_row_segment(op, L, dev):
    c1 = Case(op, L, dev, ((262,), (260,)), 64, seed=3)
    c2 = Case(op, L, dev, ((261,), (257,)), 64, seed=4)
    c1.assert_mixed()
    c2.assert_mixed()
    protocol(c1, c2)


def test_negative_then_positive_scale(op, L, dev):
    """0 * a negative scale is -0: rows of -0 (state 2) are rewritten when the next scale is positive, kept when it
    is negative again; a non-finite scale makes the zero rows NaN (state 0)."""
    c = Case(op, L, dev, WIDE, 256, seed=5)
    c.assert_mixed()
    ibuf, state = new_buffer(dev, c.rows, c.V, c.dtype)
    utt, band = c.geometry()
    for scale, codes in (([-1.0, -2.0, -0.5], (2, 2, 2)), ([1.0, -2.0, 3.0], (1, 2, 1)), ([1.0, 1.0, 1.0], (1, 1, 1)),
                         ([float("inf"), 1.0, -1.0], (0, 1, 2)), ([1.0, 1.0, 1.0], (1, 1, 1))):
        c.tracked(ibuf, state, scale)
        got, st = ibuf.cpu().numpy(), state.cpu().numpy()
        assert np.array_equal(got, c.plain(scale)), scale
        assert np.array_equal(st[~band], np.asarray(codes, np.uint8)[utt[~band]]), scale
        assert_truthful(c, got, st, finite=np.isfinite(scale))


def test_utterance_without_a_path(op, L, dev):
    """ll = -inf: every row of the utterance is NaN and its state 0, run after run; the others are skipped as usual."""
    c1 = Case(op, L, dev, WIDE, 512, seed=6, no_path=0)
    c2 = Case(op, L, dev, WIDE, 512, seed=7, no_path=0)
    got, st = protocol(c1, c2, finite=[False, True, True])
    utt, _ = c2.geometry()
    assert np.all(st[:c2.rows][utt == 0] == 0)
    nan = got[:c2.rows][utt == 0].view(np.float32)
    assert np.all(np.isnan(nan))


def test_failed_device_lengths(op, L, dev):
    """Device lengths that fail validation (S_1 > T_1): the whole buffer is NaN -- as plain writes it -- and every
    state byte 0, whatever the state claimed."""
    c = Case(op, L, dev, WIDE, 256, seed=8, device_lengths=((9, 5, 12), (3, 6, 0)))
    ibuf = torch.zeros(c.rows, c.V, dtype=torch.int32, device=dev)
    state = torch.ones(c.rows, dtype=torch.uint8, device=dev)
    c.tracked(ibuf, state)
    got = ibuf.cpu().numpy()
    assert np.array_equal(got, c.plain()) and np.all(np.isnan(got.view(np.float32)))
    assert int(state.sum()) == 0
    with pytest.raises(L.MrnntError):
        op.check_lengths()  # (and the status word is clear again for the tests that follow)


def test_padded_layout(op, L, dev):
    pad = (13, 7)
    c1 = Case(op, L, dev, WIDE, 256, seed=9, pad=pad)
    c2 = Case(op, L, dev, WIDE2, 256, seed=10, pad=pad)
    c1.assert_mixed()
    c2.assert_mixed()
    protocol(c1, c2)


def test_scalar_kernel_leaves_the_state_unknown(op, L, dev):
    """V = 1023 takes the scalar kernel, which writes every row: equal to plain, and no row is vouched for
    afterwards, whatever the state claimed before."""
    c = Case(op, L, dev, WIDE, 1023, seed=11)
    c.assert_mixed()
    ibuf, state = new_buffer(dev, c.rows + 2, c.V, c.dtype)
    state.fill_(1)
    for _ in range(2):
        c.tracked(ibuf, state)
        got, st = ibuf.cpu().numpy(), state.cpu().numpy()
        assert np.array_equal(got[:c.rows], c.plain()) and np.all(got[c.rows:] == SENTINEL[c.dtype])
        assert np.all(st[:c.rows] == 0) and np.all(st[c.rows:] == 1)


def _paths(T, S, labels, late):
    """One valid alignment per utterance: the labels on the first (or last) S_b frames, blank elsewhere."""
    al = torch.zeros(len(T), 1, int(max(T)), dtype=torch.int32)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        first = int(Tb - Sb) if late else 0
        al[b, 0, first:first + int(Sb)] = labels[b, :int(Sb)]
    return al


def test_path_loss_backward(op, L, dev):
    """mrnnt_path_backward_tracked: only the rows the paths visit are live; all the others are +0 and skipped."""
    lengths = ((9, 6, 12), (3, 5, 0))
    c1 = Case(op, L, dev, lengths, 512, seed=12, path_late=False)
    c2 = Case(op, L, dev, lengths, 512, seed=13, path_late=True)
    ibuf, state = new_buffer(dev, c1.rows, c1.V, c1.dtype)
    sent = SENTINEL[c1.dtype]
    c1.tracked(ibuf, state, [1.0, -2.0, 0.5])
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    assert np.array_equal(got, c1.plain([1.0, -2.0, 0.5]))
    assert np.all(got[st == 1] == 0) and np.all(st <= 1) and 0 < int((st == 0).sum()) <= int(np.sum(c1.T))
    before = st.copy()
    ibuf[torch.from_numpy(before != 0).to(dev)] = sent
    c2.tracked(ibuf, state)
    got, st = ibuf.cpu().numpy(), state.cpu().numpy()
    ref = c2.plain()
    kept = (before == 1) & (st == 1)
    assert kept.any() and np.all(got[kept] == sent) and np.all(ref[kept] == 0)
    assert np.array_equal(got[~kept], ref[~kept])
    assert np.any((before == 1) & (st == 0)) and np.any((before == 0) & (st == 1))  # the visited rows moved


def test_row_state_too_short_is_refused(op, L, dev):
    c = Case(op, L, dev, WIDE, 256, seed=14)
    ibuf, state = new_buffer(dev, c.rows, c.V, c.dtype)
    assert c._run(ibuf, None, state, c.rows - 1) == L.RNNT_STATUS_INVALID_VALUE
    assert torch.all(ibuf == SENTINEL[c.dtype]) and int(state.sum()) == 0  # before any device call


def test_surface_steps_with_changing_inputs(op, dev, monkeypatch):
    """Four backward() calls with changing inputs through a GradsArena with a small threshold against the
    placement-off path, bitwise; an in-place acts.grad.add_(1) before the gradient is dropped takes the reset path."""
    import _grads_placement as GP
    # 2970 rows each, other bands: 12 MB of gradient, a segment of its own in the caching allocator (a smaller block
    # is carved out of a shared segment, merges with its free neighbours when the arena lets go of it, and the
    # allocator may then hand back another address: a miss, and nothing to test)
    shapes = [((60, 40, 70), (20, 40, 0)), ((70, 60, 40), (0, 20, 40)), ((40, 70, 60), (40, 0, 20)),
              ((60, 40, 70), (20, 40, 0))]
    V = 1024
    g = torch.Generator().manual_seed(15)
    inputs = []
    for T, S in shapes:
        n = int(np.sum(np.asarray(T) * (np.asarray(S) + 1)))
        inputs.append(((torch.randn(n, V, generator=g) * 1000.0).to(dev).requires_grad_(True),
                       torch.randint(1, V, (3, 40), generator=g, dtype=torch.int32).to(dev),
                       torch.tensor(T, dtype=torch.int32), torch.tensor(S, dtype=torch.int32)))

    def steps():
        out = []
        for i, (a, lab, T, S) in enumerate(inputs):  # (no allocation of the gradient's size between the steps: a
            # free block of that size beside the kept one could be handed back in its place, a miss)
            (op.monotonic_rnnt_loss(a, lab, T, S) * (1.0 if i != 2 else -1.0)).sum().backward()
            torch.cuda.synchronize()
            out.append(a.grad.view(torch.int32).cpu().numpy().copy())
            if i == 1:
                a.grad.add_(1)  # a write through torch: the next step must not trust the state
            a.grad = None
        return out

    ar = GP.GradsArena(min_bytes=1 << 16, max_candidates=1)
    monkeypatch.setattr(GP, "ARENA", ar)
    tracked = steps()
    print(ar.stats, ar.track_stats)
    assert ar.stats["reuse_hits"] == 3 and ar.track_stats == {"tickets": 4, "vouched": 2}
    monkeypatch.setenv("MRNNT_GRADS_PLACEMENT", "0")
    plain = steps()
    assert ar.track_stats["tickets"] == 4
    for i, (x, y) in enumerate(zip(tracked, plain)):
        assert np.array_equal(x, y), i
