"""Fused joint network + monotonic RNN-T loss (extension).

    costs = monotonic_rnnt_joint_loss(enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label=0)

computes the loss of `monotonic_rnnt_loss(acts, ...)` for the packed logits

    acts[(b, t, s), :] = weight @ tanh(enc[b, t] + pred[b, s]) + bias      (t < T_b, s <= S_b)

without materialising them: the HIP kernels of `mrnnt_joint.hip` form each tile of logits on the matrix cores
(bf16 operands, fp32 accumulation) inside the log-softmax pass and again, for the live lattice rows only,
inside the gradient pass. Backward returns gradients for enc, pred, weight and bias: the fused kernel writes
the logit gradient G and the activations tanh(enc + pred) of the live rows (bf16); dweight = G^T Hact (split-K
batched GEMM, fp32 out; Hact carries a ones column when dbias is needed, so dbias = sum G comes out of the same
GEMM) is a library GEMM over those rows (hipBLASLt through torch); dH = G weight is a library GEMM too by default,
and mrnnt_joint_reduce multiplies it by (1 - Hact^2) as it folds dpre into denc (sum over s) and dpred (sum over t) in
one pass. MRNNT_JOINT_DH=mfma (H = 256 / 512, V % 8 == 0) forms dpre in one hand-written MFMA pass instead
(mrnnt_joint_dpre, then mrnnt_joint_reduce_pre): opt-in while it is slower than the GEMM it replaces.

    alignment, costs = monotonic_rnnt_joint_align(enc, pred, weight, bias, labels, input_lengths, label_lengths)
    post = monotonic_rnnt_joint_posteriors(enc, pred, weight, bias, labels, input_lengths, label_lengths)

are monotonic_rnnt_align / monotonic_rnnt_posteriors of the same never-stored logits: the joint log-softmax pass, then
the Viterbi launch in the recursion's place, or the recursion with beta and the posterior read-out.

    path_costs = monotonic_rnnt_joint_path_loss(enc, pred, weight, bias, labels, input_lengths, label_lengths, alignments)

is monotonic_rnnt_path_loss of those logits: -log p of K given alignments per utterance, differentiable in enc, pred,
weight and bias. Its forward computes the lattice rows between the lowest and the highest path of each frame and
nothing else; its backward runs the chain above over the rows the paths stand on (at most K * T_b per utterance).

Shapes: enc [B, T_slots >= max T, H], pred [B, S_slots >= max S + 1, H], weight [V, H] (torch.nn.Linear
layout), bias [V] or None; H in {128, 256, 384, 512, 640}. Inputs of other floating dtypes are cast to bf16
(the cast is differentiable, so their gradients come back in their own dtype). Costs are fp32 on the device.
There is no CPU or eager fallback.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np
import torch

try:
    from . import _mrnnt_lib as _L
    from .monotonic_rnnt_op import (Posteriors, Samples, _check_labels, _lengths, _path_alignments, _sample_args,
                                    _upstream)
except ImportError:
    import _mrnnt_lib as _L
    from monotonic_rnnt_op import (Posteriors, Samples, _check_labels, _lengths, _path_alignments, _sample_args,
                                   _upstream)

_L.load()

JOINT_H = (128, 256, 384, 512, 640)


def _vp(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _JointPrepared:
    def __init__(self, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label, alignment=None,
                 max_shift=0, hat=False):
        # hat: the factorised-blank (HAT) calls mrnnt_joint_hat_forward / _align / _backward in place of the softmax
        # ones; every other call (workspace size, live rows, posteriors, sample, dpre, reduce) is shared
        self.hat = bool(hat)
        for name, x in (("enc", enc), ("pred", pred), ("weight", weight)):
            if not x.is_cuda:
                raise RuntimeError(f"monotonic_rnnt_joint: {name} must be a GPU tensor (no CPU implementation)")
            if x.dtype != torch.bfloat16:
                raise RuntimeError(f"monotonic_rnnt_joint: {name} must be bfloat16 here")
        if enc.dim() != 3 or pred.dim() != 3 or weight.dim() != 2:
            raise RuntimeError("monotonic_rnnt_joint: expected enc [B, T, H], pred [B, S+1, H], weight [V, H]")
        B, _, H = enc.shape
        V = weight.size(0)
        if pred.size(0) != B or pred.size(2) != H or weight.size(1) != H:
            raise RuntimeError(f"monotonic_rnnt_joint: shape mismatch enc {tuple(enc.shape)}, "
                               f"pred {tuple(pred.shape)}, weight {tuple(weight.shape)}")
        if H not in JOINT_H:
            raise RuntimeError(f"monotonic_rnnt_joint: H = {H} not supported (one of {JOINT_H})")
        dev = enc.device
        self.enc = enc.contiguous()
        self.pred = pred.contiguous()
        self.weight = weight.contiguous()
        self.bias = None if bias is None else bias.detach().to(dev, torch.float32).contiguous()
        ln = _lengths(input_lengths, label_lengths)
        self.T_host, self.S_host = ln.T, ln.S
        if self.T_host.size != B or self.S_host.size != B:
            raise RuntimeError(f"monotonic_rnnt_joint: expected {B} input/label lengths")
        if B and (self.T_host.max() > enc.size(1) or self.S_host.max() + 1 > pred.size(1)):
            raise RuntimeError("monotonic_rnnt_joint: enc/pred have fewer frames/label positions than the lengths")
        self.T_dev, self.S_dev, _ = ln.on(dev)
        if not labels.is_cuda:
            _check_labels(labels, self.S_host, V)
        lab = labels.detach().to(dev, torch.int32)
        if lab.dim() == 1:
            lab = lab.view(B, -1)
        self.labels = lab.contiguous() if lab.numel() else torch.zeros(B, 1, dtype=torch.int32, device=dev)
        p = _L.MrnntJointProblem()
        p.B, p.V, p.H, p.blank = B, V, H, int(blank_label)
        p.T_host, p.S_host = ln.T_ptr, ln.S_ptr
        p.T_dev, p.S_dev = self.T_dev.data_ptr(), self.S_dev.data_ptr()
        p.labels, p.label_stride = self.labels.data_ptr(), self.labels.size(1)
        p.enc, p.enc_stride = self.enc.data_ptr(), self.enc.size(1) * H
        p.pred, p.pred_stride = self.pred.data_ptr(), self.pred.size(1) * H
        p.weight = self.weight.data_ptr()
        p.bias = self.bias.data_ptr() if self.bias is not None else None
        self.alignment = None
        if alignment is not None:
            al = alignment.detach().to(dev, torch.int32)
            self.alignment = (al.view(B, -1) if al.dim() == 1 else al).contiguous()
            p.alignment, p.align_stride = self.alignment.data_ptr(), self.alignment.size(1)
            p.align_blank, p.max_shift = int(blank_label), int(max_shift)
        self.problem = p
        self.device = dev
        self.B, self.V, self.H = B, V, H

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, size, name, *args):
        """A fresh workspace of size(problem, *args, &bytes) bytes."""
        n = ctypes.c_size_t(0)
        _L.check(size(ctypes.byref(self.problem), *args, ctypes.byref(n)), name)
        return torch.empty(max(1, n.value), dtype=torch.uint8, device=self.device)

    def forward(self, with_beta: bool):
        lib = _L.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.mrnnt_joint_workspace_size, "joint_workspace_size")
            costs = torch.empty(self.B, dtype=torch.float32, device=self.device)
            fwd, name = ((lib.mrnnt_joint_hat_forward, "mrnnt_joint_hat_forward") if self.hat
                         else (lib.mrnnt_joint_forward, "mrnnt_joint_forward"))
            _L.check(fwd(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(costs), 1 if with_beta else 0,
                         self.stream()), name)
        return costs, ws

    def align(self, L: int):
        """(alignment int32 [B, L], costs [B]): mrnnt_joint_align on a workspace of its own."""
        lib = _L.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.mrnnt_joint_workspace_size, "joint_workspace_size")
            out = torch.empty((self.B, L), dtype=torch.int32, device=self.device)
            costs = torch.empty(self.B, dtype=torch.float32, device=self.device)
            align, name = ((lib.mrnnt_joint_hat_align, "mrnnt_joint_hat_align") if self.hat
                           else (lib.mrnnt_joint_align, "mrnnt_joint_align"))
            _L.check(align(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(out), L, _vp(costs), self.stream()),
                     name)
        return out, costs

    def posteriors(self, label_width: int) -> Posteriors:
        """The forward with beta, then mrnnt_joint_posteriors on its workspace (the grid of enc / pred slots)."""
        costs, ws = self.forward(with_beta=True)
        Tg, Sg = self.enc.size(1), self.pred.size(1)
        with torch.cuda.device(self.device):
            blank = torch.empty((self.B, Tg, Sg), dtype=torch.float32, device=self.device)
            label = torch.empty_like(blank)
            emit = torch.empty((self.B, Tg), dtype=torch.float32, device=self.device)
            label_time = torch.empty((self.B, label_width), dtype=torch.float32, device=self.device)
            _L.check(_L.load().mrnnt_joint_posteriors(ctypes.byref(self.problem), _vp(ws), _vp(blank), _vp(label), Tg,
                                                      Sg, _vp(emit), Tg, _vp(label_time), label_width,
                                                      self.stream()), "mrnnt_joint_posteriors")
        return Posteriors(blank, label, emit, label_time, costs)

    def sample(self, K: int, seed: int, first: int, L: int) -> Samples:
        """The forward with beta, then mrnnt_joint_sample on its workspace."""
        costs, ws = self.forward(with_beta=True)
        with torch.cuda.device(self.device):
            out = torch.empty((self.B, K, L), dtype=torch.int32, device=self.device)
            path_costs = torch.empty((self.B, K), dtype=torch.float32, device=self.device)
            _L.check(_L.load().mrnnt_joint_sample(ctypes.byref(self.problem), _vp(ws), K, seed, first, _vp(out), L,
                                                  _vp(path_costs), self.stream()), "mrnnt_joint_sample")
        return Samples(out, path_costs, costs)

    def backward_rows(self, ws, grad_scale, with_index=False, bias_column=False, dbias=None, capturable=False):
        """The fused gradient pass over the live rows: (G [n, V], Hact [n, H]) and, with_index, the enc / pred
        row of each live row (bt_idx, bs_idx). bias_column: Hact is [n, _HACT_LD[H]] with column H = 1 (and zeros
        after it), so G^T Hact carries dbias = sum_i G[i] in column H (no separate pass over G).
        capturable: no device-to-host read -- n is the host-known bound on the live rows (mrnnt_joint_row_bound: the
        in-band rows), the kernels take the live count from the device (ABI v12 live_count_dev) and rows past it are
        zeros, so the step can be captured in a HIP graph; the GEMMs downstream then run over the bound."""
        lib = _L.load()
        with torch.cuda.device(self.device):
            cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
            _L.check(lib.mrnnt_joint_live_rows(ctypes.byref(self.problem), _vp(ws), _vp(cnt), self.stream()),
                     "mrnnt_joint_live_rows")
            bwd, name = ((lib.mrnnt_joint_hat_backward, "mrnnt_joint_hat_backward") if self.hat
                         else (lib.mrnnt_joint_backward, "mrnnt_joint_backward"))
            return self._rows_backward(ws, cnt, self.row_bound() if capturable else None, bwd, name,
                                       (_vp(_upstream(grad_scale, self)),), with_index, bias_column, dbias)

    def row_bound(self):
        nb = ctypes.c_int64(0)
        _L.check(_L.load().mrnnt_joint_row_bound(ctypes.byref(self.problem), ctypes.byref(nb)), "joint_row_bound")
        return nb.value

    def _rows_backward(self, ws, cnt, bound, bwd, name, lead=(), with_index=False, bias_column=False, dbias=None):
        """The gradient pass bwd (entry point `name`) over the rows of the last list built, cnt (int64 [1], on the
        device) of them: sizes and fills the row buffers (G [n, V], Hact [n, H or _HACT_LD[H]] and, with_index,
        bt_idx / bs_idx [n]). bound
        None: one 8-byte read-back of cnt is n; else n is that host-known bound, the kernels take the count from the
        device and the rows past it are zeros. lead: the entry point's arguments between n and G. Runs on the
        caller's current device."""
        if bound is not None:
            n = bound
            self.live_count = cnt  # referenced by the problem until the backward's last kernel is queued
            self.problem.live_count_dev = cnt.data_ptr()
        else:
            n = int(cnt.item())  # one 8-byte read-back sizes the row buffers
            self.problem.live_count_dev = None
        G = torch.empty(max(1, n), self.V, dtype=torch.bfloat16, device=self.device)
        ld = _HACT_LD[self.H] if bias_column else self.H
        self.problem.hact_ld = ld  # mrnnt_joint_reduce reads Hact with the same stride
        Hact = torch.empty(max(1, n), ld, dtype=torch.bfloat16, device=self.device)
        bt = bs = None
        if with_index:
            bt = torch.empty(max(1, n), dtype=torch.int64, device=self.device)
            bs = torch.empty(max(1, n), dtype=torch.int64, device=self.device)
        self.problem.dbias = _vp(dbias)  # the gradient pass adds sum_i G[i] into it (zeroed by the caller)
        _L.check(bwd(ctypes.byref(self.problem), _vp(ws), n, *lead, _vp(G), _vp(Hact), _vp(bt), _vp(bs), self.stream()),
                 name)
        if with_index:
            return G[:n], Hact[:n], bt[:n], bs[:n]
        return G[:n], Hact[:n]

    def path_forward(self, al):
        """(path_costs [B, K], workspace): mrnnt_joint_path_forward of the alignment rows al (int32 [B, K, L],
        contiguous, on the device) on a workspace of mrnnt_joint_path_workspace_size bytes."""
        lib = _L.load()
        K, L = al.size(1), al.size(2)
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.mrnnt_joint_path_workspace_size, "joint_path_workspace_size", K)
            costs = torch.empty((self.B, K), dtype=torch.float32, device=self.device)
            _L.check(lib.mrnnt_joint_path_forward(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(al), K, L,
                                                  _vp(costs), self.stream()), "mrnnt_joint_path_forward")
        return costs, ws

    def path_rows(self, ws, al, w):
        """After path_forward: the path weights w (fp32 [B, K] on the device, or None = 1) become Wb / We, and the
        path-live rows are listed; returns their count (int64 [1], on the device)."""
        with torch.cuda.device(self.device):
            cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
            _L.check(_L.load().mrnnt_joint_path_rows(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(al),
                                                     al.size(1), al.size(2), _vp(w), _vp(cnt), self.stream()),
                     "mrnnt_joint_path_rows")
        return cnt

    def path_row_bound(self, K):
        nb = ctypes.c_int64(0)
        _L.check(_L.load().mrnnt_joint_path_row_bound(ctypes.byref(self.problem), K, ctypes.byref(nb)),
                 "joint_path_row_bound")
        return nb.value

    def path_backward_rows(self, ws, al, w, bias_column=False, dbias=None, capturable=False):
        """backward_rows for the path scores: (G [n, V], Hact [n, H or _HACT_LD[H]]) over the path-live rows. By
        default one 8-byte read-back of their count sizes the buffers; capturable: they are sized by the host-known
        bound sum_b min(K T_b, in-band rows) (mrnnt_joint_path_row_bound), the kernels take the count from the device
        and the rows past it are zeros."""
        cnt = self.path_rows(ws, al, w)
        with torch.cuda.device(self.device):
            return self._rows_backward(ws, cnt, self.path_row_bound(al.size(1)) if capturable else None,
                                       _L.load().mrnnt_joint_path_backward, "mrnnt_joint_path_backward",
                                       bias_column=bias_column, dbias=dbias)

    def cost_grid(self, blank_costs, label_costs):
        """The two per-arc cost arrays as mrnnt_joint_expect_* take them: (wb, we, grid_T, grid_S1), fp32 [B, grid_T,
        grid_S1] on the device or None."""
        out, shape = [], None
        need = (self.B, int(self.T_host.max(initial=1)), int(self.S_host.max(initial=0)) + 1)
        for what, x in (("blank_costs", blank_costs), ("label_costs", label_costs)):
            if x is None:
                out.append(None)
                continue
            if x.dim() != 3 or x.size(0) != self.B or x.size(1) < need[1] or x.size(2) < need[2]:
                raise RuntimeError(f"monotonic_rnnt_joint_expected_cost: {what} must be [B, grid_T, grid_S1] with "
                                   f"B = {need[0]}, grid_T >= {need[1]}, grid_S1 >= {need[2]}, got {tuple(x.shape)}")
            if shape is not None and tuple(x.shape) != shape:
                raise RuntimeError("monotonic_rnnt_joint_expected_cost: blank_costs and label_costs must have the "
                                   f"same shape, got {shape} and {tuple(x.shape)}")
            shape = tuple(x.shape)
            out.append(x.detach().to(self.device, torch.float32).contiguous())
        gT, gS1 = (shape[1], shape[2]) if shape is not None else (0, 0)
        return out[0], out[1], gT, gS1

    def expect_forward(self, wb, we, gT, gS1, with_grad: bool):
        """(expected [B], costs [B], workspace): mrnnt_joint_expect_forward on a workspace of
        mrnnt_joint_expect_workspace_size bytes."""
        lib = _L.load()
        with torch.cuda.device(self.device):
            ws = self._workspace(lib.mrnnt_joint_expect_workspace_size, "joint_expect_workspace_size")
            expected = torch.empty(self.B, dtype=torch.float32, device=self.device)
            costs = torch.empty(self.B, dtype=torch.float32, device=self.device)
            _L.check(lib.mrnnt_joint_expect_forward(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(wb), _vp(we),
                                                    gT, gS1, _vp(expected), _vp(costs), 1 if with_grad else 0,
                                                    self.stream()), "mrnnt_joint_expect_forward")
        return expected, costs, ws

    def expect_rows(self, ws, wb, we, gT, gS1, ge, gc):
        """After expect_forward(with_grad=True): the row weights of sum_b ge expected + gc costs and the list of the
        expect-live rows; returns their count (int64 [1], on the device)."""
        with torch.cuda.device(self.device):
            cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
            _L.check(_L.load().mrnnt_joint_expect_rows(ctypes.byref(self.problem), _vp(ws), ws.numel(), _vp(wb),
                                                       _vp(we), gT, gS1, _vp(ge), _vp(gc), _vp(cnt), self.stream()),
                     "mrnnt_joint_expect_rows")
        return cnt

    def expect_backward_rows(self, ws, wb, we, gT, gS1, ge, gc, bias_column=False, dbias=None, capturable=False):
        """backward_rows for the expected cost: (G [n, V], Hact [n, H or _HACT_LD[H]]) over the expect-live rows. By
        default one 8-byte read-back of their count sizes the buffers; capturable: they are sized by the in-band rows
        (mrnnt_joint_row_bound), the kernels take the count from the device and the rows past it are zeros."""
        cnt = self.expect_rows(ws, wb, we, gT, gS1, ge, gc)
        with torch.cuda.device(self.device):
            return self._rows_backward(ws, cnt, self.row_bound() if capturable else None,
                                       _L.load().mrnnt_joint_expect_backward, "mrnnt_joint_expect_backward",
                                       bias_column=bias_column, dbias=dbias)

    def dpre(self, G, Hact):
        """dpre = (G weight) * (1 - Hact^2), bf16 [n, H], on the library's hand-written MFMA tiles (mrnnt_joint_dpre)."""
        n = G.shape[0]
        wt = self.weight.t().contiguous()  # [H, V]: k = v contiguous, as G's rows (1 MB at H = 512, V = 1024)
        out = torch.empty(max(1, n), self.H, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _L.check(_L.load().mrnnt_joint_dpre(ctypes.byref(self.problem), n, _vp(G), _vp(wt), _vp(Hact), _vp(out),
                                                self.stream()), "mrnnt_joint_dpre")
        return out[:n]

    def reduce(self, ws, dH, Hact, need_enc, need_pred, scratch=None):
        """d_enc / d_pred (fp32) from dH = G weight over the live rows (mrnnt_joint_reduce); Hact None: dH is already
        dpre (mrnnt_joint_dpre), summed by mrnnt_joint_reduce_pre. scratch: a dead device buffer (G, once dH exists) for the blocked form; a fresh one is
        allocated when it is too small."""
        d_enc = torch.zeros(self.enc.shape, dtype=torch.float32, device=self.device)
        d_pred = torch.zeros(self.pred.shape, dtype=torch.float32, device=self.device)
        need = ctypes.c_size_t(0)
        _L.check(_L.load().mrnnt_joint_reduce_scratch_bytes(ctypes.byref(self.problem), ctypes.byref(need)),
                 "joint_reduce_scratch_bytes")
        if scratch is None or scratch.numel() * scratch.element_size() < need.value:
            scratch = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        self.problem.reduce_scratch = scratch.data_ptr()
        self.problem.reduce_scratch_bytes = scratch.numel() * scratch.element_size()
        with torch.cuda.device(self.device):
            if Hact is None:  # dH holds dpre (mrnnt_joint_dpre)
                _L.check(_L.load().mrnnt_joint_reduce_pre(ctypes.byref(self.problem), _vp(ws), dH.shape[0], _vp(dH),
                                                          _vp(d_enc), _vp(d_pred), self.stream()),
                         "mrnnt_joint_reduce_pre")
            else:
                _L.check(_L.load().mrnnt_joint_reduce(ctypes.byref(self.problem), _vp(ws), dH.shape[0], _vp(dH),
                                                      _vp(Hact), _vp(d_enc), _vp(d_pred), self.stream()),
                         "mrnnt_joint_reduce")
        return d_enc if need_enc else None, d_pred if need_pred else None


_BIAS_SUM = os.environ.get("MRNNT_JOINT_BIAS_SUM") == "1"
_CAPTURABLE = os.environ.get("MRNNT_JOINT_CAPTURABLE") == "1"
# dH: a library GEMM (hipBLASLt) and the reduce's own multiply by default; MRNNT_JOINT_DH=mfma takes the library's
# hand-written MFMA kernel with the tanh derivative fused (mrnnt_joint_dpre: H = 256 / 512, V % 8 == 0) -- opt-in
# while it is slower than the GEMM it replaces (4.84 vs 3.77 ms at H = 512, profiles/r06/final2/dpre_bench.json)
_DH_BLAS = os.environ.get("MRNNT_JOINT_DH", "blas") != "mfma"


def _dpre_ok(H, V):
    return not _DH_BLAS and H in (256, 512) and V % 8 == 0
# dbias source per H: the 16x16x32 gradient pass sums G's columns at H = 256, 384, 512 (measured faster than the
# ones column at 256 / 384, profiles/r03/joint/dbias/); the ones column stays at H = 128 (the pass's column sums cost
# more there) and H = 640 (32x32x16 gradient pass). MRNNT_JOINT_DBIAS=pass / column forces one (A/B).
_DBIAS_MODE = os.environ.get("MRNNT_JOINT_DBIAS", "")


def _dbias_lds_fits(H, V):
    """The gradient pass keeps one column-sum row per wave (8) beside two weight tiles and the bias row in the CU's
    160 KiB of LDS (mrnnt_joint.hip joint_dbias_lds_bytes)."""
    return 2 * 32 * H * 2 + 9 * 4 * ((V + 31) // 32 * 32) <= 160 * 1024


def _dbias_in_pass(H, V):
    if _DBIAS_MODE == "column" and H in _HACT_LD:
        return False
    if not _bwd_sums_columns(H) or not _dbias_lds_fits(H, V):
        return False
    return _DBIAS_MODE == "pass" or H >= 256


def _bwd_sums_columns(H):
    """Whether the gradient pass runs on the 16x16x32 tile, which can add sum_i G[i] into dbias: H <= 512 (the
    product library always; the development build unless its joint_bwd_mfma knob selects the 32x32x16 tile)."""
    if H > 512:
        return False
    lib = _L.load()
    if hasattr(lib, "mrnnt_tune") and lib.mrnnt_tune.restype is ctypes.c_int:
        return _L.tune("joint_bwd_mfma") == 16
    return True
# Hact row stride when it carries the dbias ones column: the widths at which hipBLASLt's split-K dW GEMM (n = 3.9 M
# live rows, V = 1024) costs least over the plain H-wide one -- some widths pick much slower kernels
# (profiles/r01/joint_bias_column_gemm.json). H = 512 keeps the separate G.sum: its cheapest wider GEMM (640) costs
# +1.3 ms against 1.5 ms for G.sum, and the wider Hact store takes the rest (joint step +0.4 ms measured).
_HACT_LD = {128: 192, 256: 288, 384: 392, 640: 656}


def _split_k_weight_grad(G, Hact, chunks=32):
    """dW = G^T Hact over n live rows (K = n, output [V, H]): split K into batched GEMMs with fp32 outputs, then
    sum (a single long-K GEMM leaves most of the chip idle)."""
    n = G.shape[0]
    m = n // chunks
    if m < 1024:
        return torch.mm(G.t(), Hact, out_dtype=torch.float32)
    head = chunks * m
    part = torch.bmm(G[:head].view(chunks, m, -1).transpose(1, 2), Hact[:head].view(chunks, m, -1),
                     out_dtype=torch.float32).sum(0)
    if head < n:
        part += torch.mm(G[head:].t(), Hact[head:], out_dtype=torch.float32)
    return part


def _cast(x):
    """x as the joint kernels take it (bfloat16); the cast is differentiable"""
    return x if x is None or x.dtype == torch.bfloat16 else x.to(torch.bfloat16)


def _loss_forward(ctx, hat, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label, alignment,
                  max_distance_from_alignment, capturable):
    """The forward of MonotonicRNNTJointFunction (hat = False) and MonotonicRNNTJointHatFunction (hat = True)."""
    prep = _JointPrepared(enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label, alignment,
                          max_distance_from_alignment, hat=hat)
    need = any(ctx.needs_input_grad[:4])
    costs, ws = prep.forward(with_beta=need)
    if need:
        # the workspace is a saved tensor: freed after the last backward, kept under retain_graph=True
        ctx.save_for_backward(enc, pred, weight, ws)
        ctx.prep = prep
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.capturable = capturable
    return costs


class MonotonicRNNTJointFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label=0, alignment=None,
                max_distance_from_alignment=0, capturable=None):
        return _loss_forward(ctx, False, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label,
                             alignment, max_distance_from_alignment, capturable)

    @staticmethod
    def backward(ctx, grad_costs):
        prep, ws = ctx.prep, ctx.saved_tensors[3]
        bias_col, fused_b, db = _dbias_plan(ctx, prep)
        G, Hact = prep.backward_rows(ws, grad_costs, bias_column=bias_col, dbias=db, capturable=_capturable(ctx))
        return _grads_from_rows(ctx, prep, ws, G, Hact, bias_col, fused_b, db) + (None,) * 7


class MonotonicRNNTJointHatFunction(MonotonicRNNTJointFunction):
    """The factorised-blank (HAT) loss under the fused joint, with gradients for enc, pred, weight and bias
    (mrnnt_joint_hat_forward / mrnnt_joint_live_rows / mrnnt_joint_hat_backward, include/mrnnt.h): the arguments, the
    dbias plan and the chain from the gradient pass's rows (_grads_from_rows) of MonotonicRNNTJointFunction, whose
    backward it inherits (the prepared problem calls the factorised-blank gradient pass)."""

    @staticmethod
    def forward(ctx, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label=0, alignment=None,
                max_distance_from_alignment=0, capturable=None):
        return _loss_forward(ctx, True, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label,
                             alignment, max_distance_from_alignment, capturable)


def _capturable(ctx):
    """capturable (no host read of the row count): asked for, MRNNT_JOINT_CAPTURABLE=1, or inside HIP-graph capture"""
    if ctx.capturable is not None:
        return ctx.capturable
    return _CAPTURABLE or torch.cuda.is_current_stream_capturing()


def _dbias_plan(ctx, prep):
    """Where dbias comes from in a backward over row lists (the loss's and the path scores'): (bias_col, fused_b, db)."""
    need_b = ctx.bias_dtype is not None and ctx.needs_input_grad[3]
    # dbias rides on the dweight GEMM (a ones column in Hact); MRNNT_JOINT_BIAS_SUM=1: a separate G.sum (A/B)
    in_pass = need_b and not _BIAS_SUM and _dbias_in_pass(prep.H, prep.V)
    bias_col = need_b and ctx.needs_input_grad[2] and not _BIAS_SUM and prep.H in _HACT_LD and not in_pass
    # the 16x16x32 gradient pass (H <= 512, LDS permitting) sums G's columns itself: no separate pass over G
    fused_b = (need_b and not bias_col and not _BIAS_SUM and _bwd_sums_columns(prep.H)
               and _dbias_lds_fits(prep.H, prep.V))
    db = torch.zeros(prep.V, dtype=torch.float32, device=prep.device) if fused_b else None
    return bias_col, fused_b, db


def _grads_from_rows(ctx, prep, ws, G, Hact, bias_col, fused_b, db):
    """(d_enc, d_pred, d_weight, d_bias) from the gradient pass's rows G / Hact: the dweight GEMM, dbias, the dH GEMM
    (or mrnnt_joint_dpre) and the reduce over the last row list built in ws."""
    need_b = ctx.bias_dtype is not None and ctx.needs_input_grad[3]
    d_enc = d_pred = d_w = d_b = None
    H = prep.H
    if ctx.needs_input_grad[2]:
        dw = _split_k_weight_grad(G, Hact)  # [V, H] (+ dbias, zeros when Hact is wider)
        d_w = dw[:, :H].to(prep.weight.dtype)
        if bias_col:
            d_b = dw[:, H].to(ctx.bias_dtype)
    if fused_b:
        d_b = db.to(ctx.bias_dtype)
    elif need_b and not bias_col:
        d_b = G.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
        if _dpre_ok(H, prep.V):
            # dpre = (G W) * (1 - Hact^2) in one hand-written MFMA pass; the reduce then reads it alone
            dH, h_in = prep.dpre(G, Hact), None
        else:
            # [n, H] bf16 (hipBLASLt), with W^T stored [H, V] (1 MB copy): hipBLASLt's kernel for that layout runs
            # 3.9 vs 4.4 ms at H = 512 (profiles/r04/joint/gemm_probe.json)
            dH, h_in = G @ prep.weight.t().contiguous().t(), Hact
        # G is dead once dH exists (dweight / dbias came first): the reduce's scratch (stream-ordered after the GEMM)
        d_enc, d_pred = prep.reduce(ws, dH, h_in, ctx.needs_input_grad[0], ctx.needs_input_grad[1], scratch=G)
        del G
        d_enc = None if d_enc is None else d_enc.to(prep.enc.dtype)
        d_pred = None if d_pred is None else d_pred.to(prep.pred.dtype)
    return d_enc, d_pred, d_w, d_b


def monotonic_rnnt_joint_loss(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                              bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                              label_lengths: torch.Tensor, blank_label: int = 0,
                              alignment: Optional[torch.Tensor] = None,
                              max_distance_from_alignment: int = 0, capturable: Optional[bool] = None) -> torch.Tensor:
    """Monotonic RNN-T loss of the joint network tanh(enc + pred) @ weight.T + bias, fused (see module doc).
    alignment / max_distance_from_alignment restrict the paths as in monotonic_rnnt_loss. capturable: the backward
    reads no live-row count back to the host (row buffers and GEMMs sized by the in-band rows instead of the live
    ones: slower, graph-capturable); None = only inside HIP-graph capture (or MRNNT_JOINT_CAPTURABLE=1). A step
    captured with it replays bit for bit what an eager capturable=True step computes."""
    return MonotonicRNNTJointFunction.apply(_cast(enc), _cast(pred), _cast(weight), bias, labels, input_lengths,
                                            label_lengths, blank_label, alignment, max_distance_from_alignment,
                                            capturable)


def monotonic_rnnt_joint_hat_loss(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                                  bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                                  label_lengths: torch.Tensor, blank_label: int = 0,
                                  alignment: Optional[torch.Tensor] = None, max_distance_from_alignment: int = 0,
                                  capturable: Optional[bool] = None) -> torch.Tensor:
    """The factorised-blank (HAT, hybrid autoregressive transducer) loss of the joint network
    tanh(enc + pred) @ weight.T + bias, fused: monotonic_rnnt_hat_loss of the logits monotonic_rnnt_joint_loss never
    stores. Blank is a Bernoulli on its own logit, log p(blank) = log sigmoid(z_blank), and the labels a softmax over
    the other V - 1 logits, log p(v) = log sigmoid(-z_blank) + z_v - LSE_{u != blank} z_u -- what internal-LM
    subtraction needs -- on the fused path: no N x V logits, the same MFMA forward and gradient passes, dweight / dH
    GEMMs and reduce. Arguments, dtypes, gradients (enc, pred, weight, bias, each in its own dtype), `alignment` /
    `max_distance_from_alignment` and `capturable` as monotonic_rnnt_joint_loss; non-finite rules as
    monotonic_rnnt_hat_loss (a NaN / +inf logit or z_blank = +inf in an utterance's band: NaN cost; a label equal to
    blank_label, a -inf label logit, or a row whose non-blank logits are all -inf: no label arc). An utterance without a
    path (cost +inf) contributes exactly zero to every gradient, so d_weight / d_bias stay finite for the rest of the
    batch; a NaN cost keeps NaN gradients. Costs and gradients are bitwise reproducible. monotonic_rnnt_joint_align / _posteriors / _sample take blank_factorized=True for the same
    distribution; monotonic_rnnt_joint_path_loss / _expected_cost are softmax-only."""
    return MonotonicRNNTJointHatFunction.apply(_cast(enc), _cast(pred), _cast(weight), bias, labels, input_lengths,
                                               label_lengths, blank_label, alignment, max_distance_from_alignment,
                                               capturable)


class MonotonicRNNTJointPathFunction(torch.autograd.Function):
    """Scores of given alignments under the fused joint, with gradients for enc, pred, weight and bias
    (mrnnt_joint_path_forward / _rows / _backward, include/mrnnt.h): apply(enc, pred, weight, bias, labels,
    input_lengths, label_lengths, alignments [B, K, L], blank_label=0, capturable=None) -> path_costs [B, K]. The
    upstream gradient of path_costs is the kernels' signed weights w[b, k]."""

    @staticmethod
    def forward(ctx, enc, pred, weight, bias, labels, input_lengths, label_lengths, alignments, blank_label=0,
                capturable=None):
        prep = _JointPrepared(enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label)
        al = _path_alignments(alignments, prep.device, prep.B, "monotonic_rnnt_joint_path_loss")
        costs, ws = prep.path_forward(al)
        if any(ctx.needs_input_grad[:4]):
            # the workspace holds den of the hull rows, the hull and the paths' validity
            ctx.save_for_backward(enc, pred, weight, ws, al)
            ctx.prep = prep
            ctx.bias_dtype = None if bias is None else bias.dtype
            ctx.capturable = capturable
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        prep, ws, al = ctx.prep, ctx.saved_tensors[3], ctx.saved_tensors[4]
        w = _upstream(grad_costs, prep)
        bias_col, fused_b, db = _dbias_plan(ctx, prep)
        G, Hact = prep.path_backward_rows(ws, al, w, bias_column=bias_col, dbias=db, capturable=_capturable(ctx))
        if G.shape[0] == 0:  # no path-live row (all-zero weights, no valid path): every gradient is exactly zero
            return _zero_grads(ctx, prep) + (None,) * 6
        return _grads_from_rows(ctx, prep, ws, G, Hact, bias_col, fused_b, db) + (None,) * 6


def _zero_grads(ctx, prep):
    """(d_enc, d_pred, d_weight, d_bias) of a backward whose row list is empty: exact zeros, nothing launched."""
    need = ctx.needs_input_grad
    zero = lambda x, dt: torch.zeros(x.shape, dtype=dt, device=prep.device)  # noqa: E731
    d_b = zero(prep.bias, ctx.bias_dtype) if ctx.bias_dtype is not None and need[3] else None
    return (zero(prep.enc, prep.enc.dtype) if need[0] else None,
            zero(prep.pred, prep.pred.dtype) if need[1] else None,
            zero(prep.weight, prep.weight.dtype) if need[2] else None, d_b)


def monotonic_rnnt_joint_path_loss(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                                   bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                                   label_lengths: torch.Tensor, alignments: torch.Tensor, blank_label: int = 0,
                                   capturable: Optional[bool] = None) -> torch.Tensor:
    """Differentiable scores of given alignments under the joint network tanh(enc + pred) @ weight.T + bias, without
    materialising its logits: path_costs[b, k] = -log p(alignment (b, k)), monotonic_rnnt_path_loss of the acts
    monotonic_rnnt_joint_loss never stores, with gradients for enc, pred, weight and bias (each in its own dtype).
    What makes monotonic_rnnt_joint_align / monotonic_rnnt_joint_sample trainable -- Viterbi training (K = 1),
    risk-weighted / MWER / REINFORCE objectives over sampled paths (the upstream gradient of a path cost may have either
    sign), latency penalties:

        s = monotonic_rnnt_joint_sample(enc, pred, weight, bias, labels, T, S, num_samples=8, seed=step)
        pc = monotonic_rnnt_joint_path_loss(enc, pred, weight, bias, labels, T, S, s.alignments)   # [B, 8]
        (risk(s.alignments).detach() * torch.softmax(-pc, 1)).sum().backward()

    enc / pred / weight / bias / labels / lengths as monotonic_rnnt_joint_loss takes them (the bf16 cast, H in JOINT_H,
    GPU only). alignments: int [B, K, L] (returns [B, K]) or [B, L] (returns [B]), L >= every T_b, in the format
    monotonic_rnnt_joint_align / monotonic_rnnt_joint_sample return and monotonic_rnnt_path_loss consumes. A row that
    is no path of its utterance (a wrong or negative label, a -1 sentinel row, too few or too many labels) costs +inf
    and gets no gradient whatever its upstream gradient is. The forward computes only the lattice rows between the
    lowest and the highest path of each frame; the backward runs the joint's chain (MFMA gradient pass, dweight / dH
    GEMMs, reduce) over the rows some path with a non-zero weight stands on -- at most K * T_b per utterance -- and
    writes no dense logit gradient. capturable as in monotonic_rnnt_joint_loss: by default one 8-byte read-back of
    that row count sizes the row buffers; True (or inside HIP-graph capture) sizes them by the host-known bound
    sum_b min(K T_b, in-band rows). Costs and gradients are bitwise reproducible."""
    al = alignments.unsqueeze(1) if alignments.dim() == 2 else alignments
    out = MonotonicRNNTJointPathFunction.apply(_cast(enc), _cast(pred), _cast(weight), bias, labels, input_lengths,
                                               label_lengths, al, blank_label, capturable)
    return out.squeeze(1) if alignments.dim() == 2 else out


class MonotonicRNNTJointExpectedCostFunction(torch.autograd.Function):
    """Expected path costs and the loss under the fused joint, with gradients for enc, pred, weight and bias
    (mrnnt_joint_expect_forward / _rows / _backward, include/mrnnt.h): apply(enc, pred, weight, bias, labels,
    input_lengths, label_lengths, blank_costs, label_costs, blank_label=0, alignment=None,
    max_distance_from_alignment=0, capturable=None) -> (expected [B], costs [B]). The two upstream gradients go into one
    set of row coefficients: one row list, one gradient pass, one chain."""

    @staticmethod
    def forward(ctx, enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_costs=None, label_costs=None,
                blank_label=0, alignment=None, max_distance_from_alignment=0, capturable=None):
        prep = _JointPrepared(enc, pred, weight, bias, labels, input_lengths, label_lengths, blank_label, alignment,
                              max_distance_from_alignment)
        wb, we, gT, gS1 = prep.cost_grid(blank_costs, label_costs)
        need = any(ctx.needs_input_grad[:4])
        expected, costs, ws = prep.expect_forward(wb, we, gT, gS1, with_grad=need)
        if need:
            # the workspace holds the loss's state, den of the rows the forward computed, and A / Bk / R
            ctx.save_for_backward(enc, pred, weight, ws)
            ctx.prep, ctx.costs_grid = prep, (wb, we, gT, gS1)
            ctx.bias_dtype = None if bias is None else bias.dtype
            ctx.capturable = capturable
        return expected, costs

    @staticmethod
    def backward(ctx, grad_expected, grad_costs):
        prep, ws = ctx.prep, ctx.saved_tensors[3]
        bias_col, fused_b, db = _dbias_plan(ctx, prep)
        G, Hact = prep.expect_backward_rows(ws, *ctx.costs_grid, _upstream(grad_expected, prep),
                                            _upstream(grad_costs, prep), bias_column=bias_col, dbias=db,
                                            capturable=_capturable(ctx))
        if G.shape[0] == 0:  # no expect-live row (both upstreams zero, only single-path utterances under g_c = 0)
            return _zero_grads(ctx, prep) + (None,) * 9
        return _grads_from_rows(ctx, prep, ws, G, Hact, bias_col, fused_b, db) + (None,) * 9


def monotonic_rnnt_joint_expected_cost(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                                       bias: Optional[torch.Tensor], labels: torch.Tensor,
                                       input_lengths: torch.Tensor, label_lengths: torch.Tensor,
                                       blank_costs: Optional[torch.Tensor] = None,
                                       label_costs: Optional[torch.Tensor] = None, blank_label: int = 0,
                                       alignment: Optional[torch.Tensor] = None, max_distance_from_alignment: int = 0,
                                       capturable: Optional[bool] = None):
    """The exact expectation of an arc-additive path cost under the joint network tanh(enc + pred) @ weight.T + bias,
    and the loss of the same inputs, without materialising the logits: monotonic_rnnt_expected_cost of the acts
    monotonic_rnnt_joint_loss never stores, both outputs differentiable in enc, pred, weight and bias (each in its own
    dtype) -- a latency regulariser or a minimum-risk term for a model trained through the fused joint:

        t = torch.arange(enc.size(1), device=enc.device).view(1, -1, 1).expand(B, enc.size(1), pred.size(1))
        latency, costs = monotonic_rnnt_joint_expected_cost(enc, pred, weight, bias, labels, T, S, label_costs=t.float())
        (costs + 0.01 * latency).sum().backward()      # one row list, one gradient pass, one dweight / dH GEMM, one reduce

    enc / pred / weight / bias / labels / lengths / alignment / max_distance_from_alignment / capturable as
    monotonic_rnnt_joint_loss takes them (the bf16 cast, H in JOINT_H, GPU only); with `alignment` the expectation is
    under the restricted distribution. blank_costs / label_costs: float [B, grid_T, grid_S1], grid_T >= max T_b,
    grid_S1 >= max S_b + 1 -- the grid monotonic_rnnt_joint_posteriors returns blank / label on: the cost of the blank /
    label arc out of row (b, t, s); either may be None (all zeros), both given have the same shape; signed costs are
    fine; label_costs at s = S_b and anything at t >= T_b or s > S_b is ignored. The costs are not differentiated (their
    gradient is monotonic_rnnt_joint_posteriors' blank / label).

    Returns (expected, costs), float32 [B]; costs is monotonic_rnnt_joint_loss's, bit for bit. The backward of any
    function of the two is one chain over the rows whose coefficients are not both zero. An utterance without a finite
    cost has a NaN expected value and NaN gradients; the others' expected and costs are unaffected. Results are bitwise
    reproducible."""
    return MonotonicRNNTJointExpectedCostFunction.apply(_cast(enc), _cast(pred), _cast(weight), bias, labels,
                                                        input_lengths, label_lengths, blank_costs, label_costs,
                                                        blank_label, alignment, max_distance_from_alignment, capturable)


def _bf16(x):
    return _cast(x.detach())


def _frames(prep, max_input_length, who):
    """Row length of a per-frame output: max_input_length (>= 1), else the longest input length."""
    L = int(max_input_length) if max_input_length is not None else int(prep.T_host.max(initial=1))
    if L < 1:
        raise RuntimeError(f"{who}: max_input_length must be >= 1, got {L}")
    return L


def monotonic_rnnt_joint_align(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                               bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                               label_lengths: torch.Tensor, blank_label: int = 0,
                               alignment: Optional[torch.Tensor] = None, max_distance_from_alignment: int = 0,
                               max_input_length: Optional[int] = None, blank_factorized: bool = False):
    """Best-path (Viterbi) alignment under the joint network tanh(enc + pred) @ weight.T + bias, without materialising
    its logits (mrnnt_joint_align): monotonic_rnnt_align of the acts monotonic_rnnt_joint_loss never stores. Arguments
    as monotonic_rnnt_joint_loss; `alignment` with `max_distance_from_alignment` restricts the search to the band the
    restricted loss sums over.

    Returns (alignment, costs): alignment int32 [B, L], row b the label frame t emits or blank_label for t < T_b and
    blank_label from T_b on -- what `alignment=` of monotonic_rnnt_joint_loss consumes; costs float32 [B], the negative
    log-probability of that path (>= the loss). L is max T_b, or max_input_length (>= every T_b) when given.
    On a tie the frame emits blank. An utterance without a finite path has cost +inf and its row -1; a NaN / +inf logit
    in its band gives cost NaN and the row -1. blank_factorized: the best path under the factorised-blank probabilities
    of monotonic_rnnt_joint_hat_loss (mrnnt_joint_hat_align). Not differentiable: plain tensors are returned."""
    prep = _JointPrepared(_bf16(enc), _bf16(pred), _bf16(weight), bias, labels, input_lengths, label_lengths,
                          blank_label, alignment, max_distance_from_alignment, hat=blank_factorized)
    return prep.align(_frames(prep, max_input_length, "monotonic_rnnt_joint_align"))


def monotonic_rnnt_joint_posteriors(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                                    bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                                    label_lengths: torch.Tensor, blank_label: int = 0,
                                    alignment: Optional[torch.Tensor] = None,
                                    max_distance_from_alignment: int = 0,
                                    blank_factorized: bool = False) -> Posteriors:
    """Arc posteriors (the soft alignment) under the joint network, without materialising its logits: the fused
    forward with beta, then mrnnt_joint_posteriors on its workspace. Arguments as monotonic_rnnt_joint_loss; with
    `alignment` the posteriors are those of the restricted distribution.

    Returns monotonic_rnnt_posteriors' namedtuple (blank, label, emit, label_time, costs), float32, with the per-row
    values on the joint's own grid: blank, label [B, enc.size(1), pred.size(1)] (row (b, t, s); 0 for t >= T_b or
    s > S_b), emit [B, enc.size(1)] (0 for t >= T_b), label_time [B, labels.size(1)] (-1 for s >= S_b), costs [B] --
    bit for bit monotonic_rnnt_joint_loss of the same inputs. Rows no path reaches are exactly 0; an utterance
    without a finite cost has NaN in its own values only. blank_factorized: the posteriors (and costs) of
    monotonic_rnnt_joint_hat_loss's distribution. Not differentiable: plain tensors are returned."""
    prep = _JointPrepared(_bf16(enc), _bf16(pred), _bf16(weight), bias, labels, input_lengths, label_lengths,
                          blank_label, alignment, max_distance_from_alignment, hat=blank_factorized)
    return prep.posteriors(labels.size(1) if labels.dim() == 2 else prep.labels.size(1))


def monotonic_rnnt_joint_sample(enc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor,
                                bias: Optional[torch.Tensor], labels: torch.Tensor, input_lengths: torch.Tensor,
                                label_lengths: torch.Tensor, num_samples: int, seed: int, first_sample: int = 0,
                                blank_label: int = 0, alignment: Optional[torch.Tensor] = None,
                                max_distance_from_alignment: int = 0,
                                max_input_length: Optional[int] = None, blank_factorized: bool = False) -> Samples:
    """Alignments drawn from the path posterior under the joint network, without materialising its logits: the fused
    forward with beta, then mrnnt_joint_sample on its workspace. Arguments as monotonic_rnnt_joint_loss plus
    num_samples / seed / first_sample as monotonic_rnnt_sample, whose random numbers and decision rule it shares.

    Returns monotonic_rnnt_sample's namedtuple (alignments int32 [B, num_samples, L], path_costs float32
    [B, num_samples], costs float32 [B]); L is max T_b, or max_input_length (>= every T_b) when given. An utterance
    without a finite cost has its rows -1 and path costs +inf / NaN. blank_factorized: paths from the posterior of
    monotonic_rnnt_joint_hat_loss's distribution. Not differentiable: plain tensors are returned."""
    K, seed, first = _sample_args(num_samples, seed, first_sample, "monotonic_rnnt_joint_sample")
    prep = _JointPrepared(_bf16(enc), _bf16(pred), _bf16(weight), bias, labels, input_lengths, label_lengths,
                          blank_label, alignment, max_distance_from_alignment, hat=blank_factorized)
    L = _frames(prep, max_input_length, "monotonic_rnnt_joint_sample")
    if K < 1:
        raise RuntimeError(f"monotonic_rnnt_joint_sample: num_samples must be >= 1, got {K}")
    return prep.sample(K, seed, first, L)


__all__ = ["MonotonicRNNTJointFunction", "monotonic_rnnt_joint_loss", "monotonic_rnnt_joint_align",
           "monotonic_rnnt_joint_posteriors", "monotonic_rnnt_joint_sample", "MonotonicRNNTJointPathFunction",
           "monotonic_rnnt_joint_path_loss", "MonotonicRNNTJointExpectedCostFunction",
           "monotonic_rnnt_joint_expected_cost", "MonotonicRNNTJointHatFunction", "monotonic_rnnt_joint_hat_loss"]
