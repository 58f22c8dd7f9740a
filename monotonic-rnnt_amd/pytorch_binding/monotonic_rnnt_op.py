"""PyTorch autograd surface of the MI355X monotonic RNN-T loss.

Same public names, signatures and return conventions as the reference's
pytorch_binding/monotonic_rnnt_op.py:
  MonotonicRNNTFunction.apply(acts, labels, input_lengths, label_lengths,
                              alignment=None, max_distance_from_alignment=0, blank_label=0) -> costs [B]
  monotonic_rnnt_loss(...)                    (reference :121-163)
  MonotonicRNNTLoss(blank_label=0)            (reference :166-217)
  monotonic_rnnt_cpp.gpu_monotonic_rnnt(...) / .gpu_monotonic_rnnt_align_restrict(...)
                                              (reference pybind names, monotonic_rnnt.cu:81-152)

Execution goes through the C ABI of libmonotonic_rnnt_amd.so: GPU tensors run the HIP kernels on the current
torch stream; CPU tensors run the library's own multithreaded host implementation (mrnnt_cpu_*, the
reference's cpu_monotonic_rnnt path). There is no eager-PyTorch fallback.

Behavioural differences from the reference, all deliberate:
  * forward runs the log-softmax reduce and the alpha/beta recursion; the logit gradient is produced
    in backward with dL/dcost[b] fused into the kernel (the reference writes grads in forward into a
    zeros_like(acts) and rescales them in backward: 3 extra passes over an N x V tensor, :32-36, :96-118);
  * costs are computed on the device (the reference computes into a host tensor and copies, :37, :90);
  * labels / alignment use their true row strides (the reference assumes max(S) / max(T)); strides below
    max(S) / max(T), and (for host labels) labels outside [0, V), are rejected;
  * acts without requires_grad take the cost-only path on both devices (the reference's CPU path segfaults
    writing into its empty grads tensor);
  * MonotonicRNNTLoss.forward uses self.blank_label (the reference reads a missing self.blank, :214).

Extensions beyond the reference: bf16/fp16 acts (costs stay fp32) and the padded
[B, pad_T, pad_S1, V] acts layout, both read in place by the same kernels.

Lengths on the GPU (the reference's required form, monotonic_rnnt.cu:85-88) are never read back: the launch is
planned from acts.size(0) and labels.size(1) and the lattice is built and validated on the device (ABI v7
lengths_on_device), so a step makes no host synchronisation and can be captured in a HIP graph. Lengths that fail
that validation make the call's costs and gradients NaN and are reported by the next call (or check_lengths()),
as a RuntimeError, the way an asynchronous device error surfaces; MRNNT_SYNC_LENGTH_CHECK=1 checks every call
synchronously instead. Host (CPU) lengths plan the launch exactly, uploaded once per distinct shape.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
from typing import Optional

import numpy as np
import torch

try:
    from . import _mrnnt_lib as _L
    from . import _grads_placement as _GP
except ImportError:  # imported with pytorch_binding/ on sys.path, like the reference's tests do
    import _mrnnt_lib as _L
    import _grads_placement as _GP

_L.load()  # fail loudly at import if the HIP library is missing


# acts element types the kernels read (the arithmetic is fp32/fp64 in registers whatever the type)
_ELEM = {torch.float32: _L.MRNNT_F32, torch.bfloat16: _L.MRNNT_BF16, torch.float16: _L.MRNNT_F16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Lengths:
    """int32 host copies of one (T, S) pair (the plan needs them on the host), their device copies per device,
    and the workspace sizes of that shape. Cached by content: training loops repeat shapes, so the conversions,
    the pinned staging copy and its H2D transfer are paid once per distinct shape, not per call. Entries are
    never written after creation (the kernels only read them)."""

    __slots__ = ("T", "S", "T_ptr", "S_ptr", "dev", "ws")

    def __init__(self, T: np.ndarray, S: np.ndarray):
        self.T, self.S = T, S
        self.T_ptr, self.S_ptr = T.ctypes.data, S.ctypes.data
        self.dev = {}
        self.ws = {}

    def on(self, dev: torch.device):
        """Device copies of T, S and the lattice offsets (mrnnt_lattice_host: with them the forward launches no
        setup kernel), uploaded once as one pinned non-blocking copy on the current stream (no host wait); a call
        on another stream waits for that upload through an event. Returns (T_dev, S_dev, lattice_dev)."""
        hit = self.dev.get(dev)
        stream = torch.cuda.current_stream(dev)
        if hit is None and torch.cuda.is_current_stream_capturing():
            # the upload would only be captured, not run: an eager call with these lengths before the first replay
            # would read unwritten offsets
            raise RuntimeError("monotonic_rnnt: these host lengths are first seen inside HIP-graph capture; run one "
                               "warm-up call with them before capturing, or pass the lengths as GPU tensors")
        if hit is None:
            B = self.T.size
            p = _L.MrnntProblem()
            p.B, p.T_host, p.S_host = B, self.T_ptr, self.S_ptr
            n = ctypes.c_size_t(0)
            _L.check(_L.load().mrnnt_lattice_bytes(ctypes.byref(p), ctypes.byref(n)), "lattice_bytes")
            lat_off = 8 * ((2 * B * 4 + 7) // 8)
            host = torch.empty(lat_off + n.value, dtype=torch.uint8).pin_memory()
            hv = host.numpy()
            hv[:B * 4] = self.T.view(np.uint8)
            hv[B * 4:2 * B * 4] = self.S.view(np.uint8)
            _L.check(_L.load().mrnnt_lattice_host(ctypes.byref(p), ctypes.c_void_p(host.data_ptr() + lat_off), n.value),
                     "lattice_host")
            d = host.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            hit = self.dev[dev] = (d[:B * 4].view(torch.int32), d[B * 4:2 * B * 4].view(torch.int32), d[lat_off:],
                                   ev, stream)
        elif hit[4] != stream and not torch.cuda.is_current_stream_capturing():
            # (under HIP-graph capture the wait is skipped: torch.cuda.graph synchronises the device before
            # capture begins, so an upload issued before it has landed)
            stream.wait_event(hit[3])
        return hit[0], hit[1], hit[2]


_LEN_CACHE: "dict" = {}
_LEN_CACHE_MAX = 64


def _host_int32(t: torch.Tensor) -> np.ndarray:
    t = t.detach()
    if t.is_cuda:
        t = t.cpu()  # a sync, as the reference's cudaMemcpy of the lengths (gpu_workspace_manager.h:87-96)
    return np.ascontiguousarray(t.numpy() if t.dtype == torch.int32 else t.to(torch.int32).numpy()).reshape(-1)


def _content(t: torch.Tensor) -> bytes:
    if not t.is_cuda and t.dtype == torch.int32 and t.is_contiguous():
        return ctypes.string_at(t.data_ptr(), t.numel() * 4)  # no numpy round trip for the common case
    return _host_int32(t).tobytes()


def _lengths(input_lengths: torch.Tensor, label_lengths: torch.Tensor) -> _Lengths:
    key = (_content(input_lengths), _content(label_lengths))
    hit = _LEN_CACHE.get(key)
    if hit is None:
        hit = _Lengths(np.frombuffer(key[0], np.int32).copy(), np.frombuffer(key[1], np.int32).copy())
        if len(_LEN_CACHE) >= _LEN_CACHE_MAX:
            _LEN_CACHE.pop(next(iter(_LEN_CACHE)))
        _LEN_CACHE[key] = hit
    return hit


import os as _os

_SYNC_LENGTH_CHECK = _os.environ.get("MRNNT_SYNC_LENGTH_CHECK", "0") not in ("", "0")
_STATUS = None
_DYN_WS: "dict" = {}


def _status_word():
    """The library's host-mapped status word (mrnnt_status_word): the device stores into it when device-resident
    lengths fail validation, with no copy on the stream."""
    global _STATUS
    if _STATUS is None:
        ptr = _L.load().mrnnt_status_word()
        if not ptr:
            raise RuntimeError("monotonic_rnnt: could not allocate the host-mapped status word")
        _STATUS = ptr
    return _STATUS


def check_lengths(sync: bool = True) -> None:
    """Raise if an earlier call's GPU-resident lengths failed validation on the device (their costs and gradients
    are NaN). sync=True waits for the current device's queued work first."""
    if _STATUS is None:
        return
    if sync and torch.cuda.is_available():
        torch.cuda.synchronize()
    if _STATUS[0] != 0:
        _STATUS[0] = 0
        raise _L.MrnntError(_L.RNNT_STATUS_INVALID_VALUE, "monotonic_rnnt",
                            "GPU-resident lengths of an earlier call failed validation on the device: need "
                            "T_b > 0, 0 <= S_b <= T_b, S_b <= labels.size(1), sum_b T_b (S_b+1) == acts.size(0) "
                            "(padded acts: T_b <= size(1), S_b < size(2)), T_b <= alignment.size(1); that call's "
                            "costs and gradients are NaN")


def _device_lengths(t: torch.Tensor, dev: torch.device, B: int, what: str) -> torch.Tensor:
    t = t.detach()
    if t.device != dev or t.dtype != torch.int32:
        t = t.to(dev, torch.int32, non_blocking=True)
    t = t.reshape(-1).contiguous()
    if t.numel() != B:
        raise RuntimeError(f"monotonic_rnnt: expected {B} {what}, got {t.numel()}")
    return t


class _Prepared:
    """Views of one call's inputs on the device they live on, plus the filled mrnnt_problem.

    GPU acts: device lengths / labels / alignment (host lengths plan the launch). CPU acts: every pointer on
    the host (the mrnnt_cpu_* entry points)."""

    def __init__(self, acts, labels, input_lengths, label_lengths, alignment, max_shift, blank_label,
                 num_threads=0):
        if acts.dtype not in _ELEM:
            raise RuntimeError("monotonic_rnnt: acts must be float32 (reference monotonic_rnnt.cu:19,84), "
                               f"or bfloat16 / float16 (extension, GPU only); got {acts.dtype}")
        if acts.dim() not in (2, 4):
            raise RuntimeError("monotonic_rnnt: acts must be packed 2-D [sum_b T_b (S_b+1), V] "
                               "or padded 4-D [B, max_T, max_S+1, V]")
        self.on_gpu = acts.is_cuda
        if not self.on_gpu and acts.dtype != torch.float32:
            raise RuntimeError(f"monotonic_rnnt: the CPU implementation takes float32 acts, got {acts.dtype}")
        dev = acts.device
        self.acts = acts.contiguous()
        self.num_threads = int(num_threads)
        B = labels.size(0)
        # GPU acts with GPU lengths: planned without reading the lengths back (ABI v7 lengths_on_device)
        self.dyn = self.on_gpu and (input_lengths.is_cuda or label_lengths.is_cuda)
        if self.dyn:
            self.lengths = ln = None
            self.T_host = self.S_host = None
            self.T_dev = _device_lengths(input_lengths, dev, B, "input lengths")
            self.S_dev = _device_lengths(label_lengths, dev, B, "label lengths")
        else:
            self.lengths = ln = _lengths(input_lengths, label_lengths)
            self.T_host, self.S_host = ln.T, ln.S
            if self.T_host.size != B or self.S_host.size != B:
                raise RuntimeError(f"monotonic_rnnt: expected {B} input/label lengths, "
                                   f"got {self.T_host.size}/{self.S_host.size}")
        lab = labels.detach()
        if lab.device != dev or lab.dtype != torch.int32:
            lab = lab.to(dev, torch.int32)
        if lab.dim() == 1:
            lab = lab.view(B, -1)
        self.labels = lab.contiguous() if lab.numel() else torch.zeros(B, 1, dtype=torch.int32, device=dev)
        self.lattice = None
        if self.on_gpu and not self.dyn:
            self.T_dev, self.S_dev, self.lattice = ln.on(dev)
        if self.on_gpu and not labels.is_cuda and not self.dyn:
            _check_labels(labels, self.S_host, acts.size(-1))
        self.alignment = None
        if alignment is not None:
            al = alignment.detach().to(dev, torch.int32)
            self.alignment = (al.view(B, -1) if al.dim() == 1 else al).contiguous()
        p = _L.MrnntProblem()
        p.B = B
        p.V = self.acts.size(-1)
        p.blank = int(blank_label)
        p.max_shift = int(max_shift)
        if self.dyn:
            p.lengths_on_device = 1
            # (first allocated outside graph capture; a capture that comes first fails closed without the report)
            if _STATUS is not None or not torch.cuda.is_current_stream_capturing():
                p.status_host = ctypes.cast(_status_word(), ctypes.c_void_p).value
        else:
            p.T_host = ln.T_ptr
            p.S_host = ln.S_ptr
        if self.on_gpu:
            p.T_dev = self.T_dev.data_ptr()
            p.S_dev = self.S_dev.data_ptr()
            p.lattice = self.lattice.data_ptr() if self.lattice is not None else None
        p.acts = self.acts.data_ptr()
        p.labels = self.labels.data_ptr()
        p.label_stride = self.labels.size(1)
        p.alignment = self.alignment.data_ptr() if self.alignment is not None else None
        p.align_stride = self.alignment.size(1) if self.alignment is not None else 0
        p.align_blank = int(blank_label)  # the reference parses the alignment with the same blank (monotonic_rnnt.cu:144)
        p.acts_dtype = _ELEM[self.acts.dtype]
        if self.acts.dim() == 4:
            if self.acts.size(0) != B:
                raise RuntimeError(f"monotonic_rnnt: padded acts has {self.acts.size(0)} utterances, labels {B}")
            p.pad_T, p.pad_S1 = self.acts.size(1), self.acts.size(2)
            p.num_rows = B * p.pad_T * p.pad_S1
        else:
            p.num_rows = self.acts.size(0)
        self.problem = p
        self.device = dev

    def workspace(self, num_paths: int = 0, expect: bool = False) -> torch.Tensor:
        """The call's workspace; num_paths > 0: the one of monotonic_rnnt_path_loss for that many paths; expect: the
        one of monotonic_rnnt_expected_cost."""
        p = self.problem
        # the plan also depends on V and the acts element type (whether the chase launch applies, and so whether the
        # workspace holds its ready flags) and on the device (its CU count bounds the chase)
        key = (self.on_gpu, self.alignment is not None, _L.load(), p.V, p.acts_dtype, str(self.device), p.pad_T,
               p.pad_S1, -1 if expect else num_paths)
        if self.dyn:  # sized from bounds: the shapes of acts and labels
            key = key + (p.B, p.num_rows, p.label_stride)
            cache = _DYN_WS
        else:
            cache = self.lengths.ws  # with the key above, a function of the lengths
        n = cache.get(key)
        if n is None:
            c = ctypes.c_size_t(0)
            name, args = (("expect_workspace_size", ()) if expect else
                          ("path_workspace_size", (num_paths,)) if num_paths > 0 else ("workspace_size", ()))
            size = getattr(_L.load(), ("mrnnt_" if self.on_gpu else "mrnnt_cpu_") + name)
            # the plan reads the CU count of the CURRENT device: make it this call's
            with (_on_device(self.device) if self.on_gpu else _NULL_CTX):
                _L.check(size(ctypes.byref(self.problem), *args, ctypes.byref(c)), name)
            n = cache[key] = max(1, c.value)
            if self.dyn and len(_DYN_WS) > 256:
                _DYN_WS.clear()
        return torch.empty(n, dtype=torch.uint8, device=self.device)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


def _check_labels(labels: torch.Tensor, S_host: np.ndarray, V: int) -> None:
    """Host labels: every label inside the lattice (s < S_b) must be in [0, V). (Device labels are not read back;
    the kernels never index past a row with them, and an out-of-range label yields a non-finite cost.)"""
    lab = labels.detach().to(torch.int32).numpy()
    lab = lab.reshape(len(S_host), -1) if lab.size else lab.reshape(len(S_host), 0)
    if lab.shape[1] < int(S_host.max(initial=0)):
        return  # the stride check in the library reports this
    mask = np.arange(lab.shape[1])[None, :] < S_host[:, None]
    bad = mask & ((lab < 0) | (lab >= V))
    if bad.any():
        b, s = map(int, np.argwhere(bad)[0])
        raise _L.MrnntError(_L.RNNT_STATUS_INVALID_VALUE, "monotonic_rnnt",
                            f"label {int(lab[b, s])} at ({b}, {s}) outside [0, V = {V})")


_NULL_CTX = contextlib.nullcontext()


def _on_device(dev: torch.device):
    """torch.cuda.device(dev) only when dev is not already current (the context manager costs microseconds)."""
    return _NULL_CTX if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _call(prep: _Prepared, name: str, *args, pending: bool = False, lengths: bool = True):
    """Runs entry point `name` where the inputs live: mrnnt_cpu_<name>(problem, *args, num_threads) on the host, else
    mrnnt_<name>(problem, *args, stream) on the device's current stream. GPU-resident lengths: `pending` first surfaces
    an earlier call's failed validation (no wait); `lengths` is the MRNNT_SYNC_LENGTH_CHECK tail."""
    lib = _L.load()
    if not prep.on_gpu:
        _L.check(getattr(lib, "mrnnt_cpu_" + name)(ctypes.byref(prep.problem), *args, prep.num_threads),
                 "mrnnt_cpu_" + name)
        return
    if pending and prep.dyn:
        check_lengths(sync=False)
    with _on_device(prep.device):  # kernels go to this device's current stream
        _L.check(getattr(lib, "mrnnt_" + name)(ctypes.byref(prep.problem), *args, prep.stream()), "mrnnt_" + name)
        if lengths and prep.dyn and _SYNC_LENGTH_CHECK and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(prep.device).synchronize()
            check_lengths(sync=False)


def _forward(prep: _Prepared, with_beta: bool, hat: bool = False):
    """The forward on a fresh workspace; hat: the factorised-blank entry points (mrnnt_hat_* / mrnnt_cpu_hat_*)."""
    ws = prep.workspace()
    costs = torch.empty(prep.problem.B, dtype=torch.float32, device=prep.device)
    _call(prep, "hat_forward" if hat else "forward", _ptr(ws), ws.numel(), _ptr(costs), 1 if with_beta else 0,
          pending=True)
    return costs, ws


def _tracked_backward(prep: _Prepared, stem: str, lead: tuple, grads: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The dense gradient of entry point `stem` (mrnnt_<stem> / mrnnt_cpu_<stem>; lead: its arguments before grads)
    into grads, or into a buffer of this call's."""
    ticket = None
    if grads is None:  # large GPU gradients: a fast-writing buffer, kept across calls (_grads_placement), with the
        # state of its rows: the tracked entry does not store again the zero rows the buffer already holds
        grads, ticket = _GP.grads_tracked(prep.acts) if prep.on_gpu else (torch.empty_like(prep.acts), None)
    if ticket is not None:
        _call(prep, stem + "_tracked", *lead, _ptr(grads), _ptr(ticket.state), ticket.state.numel(), lengths=False)
        ticket.commit()  # enqueued: the state describes the buffer from here on (in stream order)
    else:
        _call(prep, stem, *lead, _ptr(grads), lengths=False)
    return grads


def _backward(prep: _Prepared, ws: torch.Tensor, grad_scale: Optional[torch.Tensor],
              grads: Optional[torch.Tensor] = None, hat: bool = False) -> torch.Tensor:
    prep.problem.grad_scale_broadcast = 0
    if grad_scale is not None:
        grad_scale = grad_scale.detach()
        if (grad_scale.dim() == 1 and grad_scale.numel() > 1 and grad_scale.stride(0) == 0
                and grad_scale.dtype == torch.float32 and grad_scale.device == prep.device):
            # the backward of costs.sum() / .mean(): one value expanded over B -- read it in place (ABI v6)
            # instead of materialising the [B] vector (a copy kernel per step)
            prep.problem.grad_scale_broadcast = 1
        else:
            grad_scale = grad_scale.to(prep.device, torch.float32).contiguous()
    return _tracked_backward(prep, "hat_backward" if hat else "backward", (_ptr(ws), _ptr(grad_scale)), grads)


def _loss_forward(ctx, hat, acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment,
                  blank_label):
    """The forward of MonotonicRNNTFunction (hat = False) and MonotonicRNNTHatFunction (hat = True)."""
    prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment, blank_label)
    need_grad = bool(ctx.needs_input_grad[0])
    costs, ws = _forward(prep, with_beta=need_grad, hat=hat)
    if need_grad:
        # acts is re-read by the gradient kernel (saving it lets autograd catch in-place edits); the workspace
        # (den / lp / alpha / beta) is a saved tensor too, so autograd frees it after the last backward and
        # keeps it for another one under retain_graph=True (the reference saves its grads, :92)
        ctx.save_for_backward(acts, ws)
        ctx.prep, ctx.hat = prep, hat
    return costs


class MonotonicRNNTFunction(torch.autograd.Function):
    """reference pytorch_binding/monotonic_rnnt_op.py:18-118"""

    @staticmethod
    def forward(ctx, acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                max_distance_from_alignment: int = 0, blank_label: int = 0) -> torch.Tensor:
        return _loss_forward(ctx, False, acts, labels, input_lengths, label_lengths, alignment,
                             max_distance_from_alignment, blank_label)

    @staticmethod
    def backward(ctx, grad_outputs):
        _, ws = ctx.saved_tensors
        grads = _backward(ctx.prep, ws, grad_outputs, hat=ctx.hat)
        return grads, None, None, None, None, None, None


def monotonic_rnnt_loss(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                        label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                        max_distance_from_alignment: int = 0, blank_label: int = 0) -> torch.Tensor:
    """Computes the monotonic RNN-T loss between a sequence of activations and a ground truth labeling.

    Args (reference monotonic_rnnt_op.py:130-160):
        acts:           packed 2-D float32 tensor of logits (GPU: HIP kernels; CPU: host implementation), (sum_b T_b*(S_b+1), V), utterance b
                        contiguous, then t-major, then s. Softmax is applied internally.
                        Extensions (GPU): bfloat16 / float16 elements (fp32 math; grads in the same type), and
                        the padded 4-D joint-network layout [B, pad_T >= max T, pad_S1 >= max S + 1, V]
                        read in place (no packing copy; grads of padding rows are 0).
        labels:         2-D int tensor [B, max_b S_b] of padded label sequences.
        input_lengths:  1-D int tensor [B] of T_b.
        label_lengths:  1-D int tensor [B] of S_b.
        alignment:      optional [B, max_b T_b] int tensor; restricts paths to within
                        max_distance_from_alignment frames of it.
        blank_label:    index of the blank symbol.
    Returns:
        1-D float tensor [B] of costs (negative log probabilities) on acts.device.
    """
    result = MonotonicRNNTFunction.apply(acts, labels, input_lengths, label_lengths, alignment,
                                         max_distance_from_alignment, blank_label)
    assert result is not None
    return result


class MonotonicRNNTHatFunction(MonotonicRNNTFunction):
    """The loss with the factorised blank of the hybrid autoregressive transducer (mrnnt_hat_forward /
    mrnnt_hat_backward and the mrnnt_cpu_hat_* twins, include/mrnnt.h): apply(acts, labels, input_lengths,
    label_lengths, alignment=None, max_distance_from_alignment=0, blank_label=0) -> costs [B]. The backward is
    MonotonicRNNTFunction's (the context remembers the flavour)."""

    @staticmethod
    def forward(ctx, acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                max_distance_from_alignment: int = 0, blank_label: int = 0) -> torch.Tensor:
        return _loss_forward(ctx, True, acts, labels, input_lengths, label_lengths, alignment,
                             max_distance_from_alignment, blank_label)


def monotonic_rnnt_hat_loss(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                            label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                            max_distance_from_alignment: int = 0, blank_label: int = 0) -> torch.Tensor:
    """The monotonic RNN-T loss with the factorised blank of the hybrid autoregressive transducer (HAT): for a row z
    of logits, blank is a Bernoulli on its own logit and the labels a softmax over the other V - 1 logits,

        log p(blank) = log sigmoid(z[blank])
        log p(label) = log sigmoid(-z[blank]) + z[label] - logsumexp(z[v] for v != blank)

    -- the form that makes internal-LM subtraction well defined and separates the emission decision from the label
    identity. Lattice, band, alignment restriction, recursion and cost are monotonic_rnnt_loss's, and so are the
    arguments and everything they support: CPU and GPU tensors, bfloat16 / float16 acts, the padded 4-D layout,
    GPU-resident lengths without a host read, HIP-graph capture. blank_label may be any index in [0, V).

    The transform runs inside the log-softmax and gradient kernels (no second N x V tensor; the step moves the bytes
    of monotonic_rnnt_loss) with the blank logit kept out of the denominator's max and sum, so a dominant or
    suppressed blank logit loses no digits. A -inf label logit or blank logit means "no such arc"; a NaN or +inf
    logit in an utterance's band (the blank logit included) gives that utterance a NaN cost and leaves the others
    bit-identical. Returns float32 costs [B] on acts.device. The read-outs take blank_factorized=True
    (monotonic_rnnt_align / _posteriors / _sample), and so do monotonic_rnnt_path_loss and monotonic_rnnt_expected_cost;
    the fused joint's path scores and expected costs are softmax-only for now."""
    result = MonotonicRNNTHatFunction.apply(acts, labels, input_lengths, label_lengths, alignment,
                                            max_distance_from_alignment, blank_label)
    assert result is not None
    return result


def _readout_length(prep, max_input_length, who):
    """Row length of a per-frame read-out: max_input_length, else the padded acts' frames, else the longest host length,
    else the alignment's row length."""
    if max_input_length is not None:
        L = int(max_input_length)
    elif prep.acts.dim() == 4:
        L = prep.acts.size(1)
    elif not prep.dyn:
        L = int(prep.T_host.max())
    elif prep.alignment is not None:
        L = prep.alignment.size(1)
    else:
        raise RuntimeError(f"{who}: with GPU-resident lengths and packed acts the longest input length "
                           "is not known on the host; pass max_input_length (>= every input length)")
    if L < 1:
        raise RuntimeError(f"{who}: max_input_length must be >= 1, got {L}")
    return L


def monotonic_rnnt_align(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                         label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                         max_distance_from_alignment: int = 0, blank_label: int = 0,
                         max_input_length: Optional[int] = None, blank_factorized: bool = False):
    """Best-path (Viterbi) alignment of every utterance: the single most probable monotonic path through the lattice
    the loss sums over (mrnnt_align / mrnnt_cpu_align, include/mrnnt.h). Arguments as monotonic_rnnt_loss; an
    `alignment` with `max_distance_from_alignment` restricts the search to the same band as the loss.

    Returns (alignment, costs):
        alignment: int32 [B, L] on acts.device. Row b holds, for t < T_b, the label frame t emits or blank_label --
                   the format `alignment=` of the loss consumes -- and blank_label for t >= T_b.
        costs:     float32 [B], the negative log-probability of that path (>= the loss of the same inputs).
    L is max T_b for host lengths, acts.size(1) for padded 4-D acts; for GPU-resident lengths with packed acts pass
    max_input_length (>= every T_b), or else alignment.size(1) is used when a restricting alignment is given.
    On a tie the frame emits blank (the label arc is taken only when strictly more probable). An utterance without a
    finite path (masked -inf logits, a band no path fits) has cost +inf and its row -1; a NaN / +inf logit in its band
    gives cost NaN and the row -1. Not differentiable: requires_grad is ignored and plain tensors are returned.
    GPU-resident lengths that fail validation surface through check_lengths() exactly as for the loss.
    blank_factorized=True: the best path under monotonic_rnnt_hat_loss's distribution (mrnnt_hat_align)."""
    acts = acts.detach()
    prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment, blank_label)
    L = _readout_length(prep, max_input_length, "monotonic_rnnt_align")
    ws = prep.workspace()
    B = prep.problem.B
    out = torch.empty((B, L), dtype=torch.int32, device=prep.device)
    costs = torch.empty(B, dtype=torch.float32, device=prep.device)
    _call(prep, "hat_align" if blank_factorized else "align", _ptr(ws), ws.numel(), _ptr(out), L, _ptr(costs),
          pending=True)
    return out, costs


Posteriors = collections.namedtuple("Posteriors", ["blank", "label", "emit", "label_time", "costs"])


def monotonic_rnnt_posteriors(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                              label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                              max_distance_from_alignment: int = 0, blank_label: int = 0,
                              max_input_length: Optional[int] = None, blank_factorized: bool = False) -> Posteriors:
    """Arc posteriors of the lattice the loss sums over -- the soft alignment (mrnnt_posteriors /
    mrnnt_cpu_posteriors, include/mrnnt.h): the forward pass with beta, then a read-out of its workspace on the same
    stream. Arguments as monotonic_rnnt_loss; with `alignment` and `max_distance_from_alignment` the posteriors are
    those of the restricted distribution.

    Returns the namedtuple (blank, label, emit, label_time, costs), all float32 on acts.device:
        blank, label: shape acts.shape[:-1]. For lattice row (b, t, s) the probability, under the model and given the
                      labels, that frame t takes the blank arc / the label arc out of state (t, s) (label: 0 at
                      s = S_b). Per frame, sum_s (blank + label) = 1. Padding rows of 4-D acts are 0.
        emit:         [B, L], sum_s label(t, s): the probability that frame t emits a label; 0 for t >= T_b.
                      sum_t emit = S_b. L is chosen as monotonic_rnnt_align chooses it: max T_b for host lengths,
                      acts.size(1) for padded 4-D acts, else max_input_length (>= every T_b) or alignment.size(1).
        label_time:   [B, labels.size(1)], sum_t t * label(t, s): the expected frame at which label s is emitted
                      (increasing in s); -1 for s >= S_b.
        costs:        [B], the loss of the same inputs.
    Rows no path can reach (outside the band, masked logits) are exactly 0. An utterance without a finite cost (no
    path: +inf; a NaN / +inf logit in its band) has NaN in all of its values; the other utterances are unaffected.
    Not differentiable: requires_grad is ignored and plain tensors are returned. GPU-resident lengths that fail
    validation make every value NaN and surface through check_lengths() exactly as for the loss.
    blank_factorized=True: the posteriors (and costs) under monotonic_rnnt_hat_loss's distribution -- the same read-out
    over the state of the factorised forward."""
    acts = acts.detach()
    prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment, blank_label)
    L = _readout_length(prep, max_input_length, "monotonic_rnnt_posteriors")
    costs, ws = _forward(prep, with_beta=True, hat=blank_factorized)
    B, dev = prep.problem.B, prep.device
    Sw = labels.size(1) if labels.dim() == 2 else prep.labels.size(1)
    blank = torch.empty(prep.acts.shape[:-1], dtype=torch.float32, device=dev)
    label = torch.empty_like(blank)
    emit = torch.empty((B, L), dtype=torch.float32, device=dev)
    label_time = torch.empty((B, Sw), dtype=torch.float32, device=dev)
    _call(prep, "posteriors", _ptr(ws), _ptr(blank), _ptr(label), _ptr(emit), L, _ptr(label_time), Sw)
    return Posteriors(blank, label, emit, label_time, costs)


Samples = collections.namedtuple("Samples", ["alignments", "path_costs", "costs"])


def _sample_args(num_samples, seed, first_sample, where):
    """(num_samples, seed as uint64, first_sample) as the library takes them; the library checks the ranges."""
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise RuntimeError(f"{where}: seed must fit in 64 bits, got {seed}")
    return int(num_samples), seed & ((1 << 64) - 1), int(first_sample)


def monotonic_rnnt_sample(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                          label_lengths: torch.Tensor, num_samples: int, seed: int, first_sample: int = 0,
                          alignment: Optional[torch.Tensor] = None, max_distance_from_alignment: int = 0,
                          blank_label: int = 0, max_input_length: Optional[int] = None,
                          blank_factorized: bool = False) -> Samples:
    """Whole alignments drawn from the path posterior p(path | labels, acts) of the lattice the loss sums over
    (mrnnt_sample / mrnnt_cpu_sample, include/mrnnt.h): the forward pass with beta, then a read-out of its workspace
    on the same stream. Arguments as monotonic_rnnt_loss; with `alignment` and `max_distance_from_alignment` the
    draws come from the restricted distribution (k = 0 returns the given alignment).

    Returns the namedtuple (alignments, path_costs, costs) on acts.device:
        alignments: int32 [B, num_samples, L]. Row (b, k) holds, for t < T_b, the label frame t emits or blank_label
                    -- the format `alignment=` of the loss consumes -- and blank_label for t >= T_b. L is chosen as
                    monotonic_rnnt_posteriors chooses it: max T_b for host lengths, acts.size(1) for padded 4-D acts,
                    else max_input_length (>= every T_b) or alignment.size(1).
        path_costs: float32 [B, num_samples], the negative log-probability of each drawn path under the model
                    (>= costs; exp(costs - path_costs) is the probability of drawing it).
        costs:      float32 [B], the loss of the same inputs.
    Random numbers are counter-based (Philox4x32-10 keyed by `seed`, counted by frame, sample index first_sample + k
    and utterance index): the same call gives the same bits, num_samples = 8 gives the first 8 rows of num_samples =
    64, and first_sample = 8 continues where 8 samples stopped. An utterance without a finite cost has all its rows
    -1 and path costs +inf (no path) or NaN; the others are unaffected. Not differentiable: requires_grad is ignored
    and plain tensors are returned. GPU-resident lengths that fail validation give -1 / NaN everywhere and surface
    through check_lengths() exactly as for the loss.
    blank_factorized=True: draws, path costs and costs under monotonic_rnnt_hat_loss's distribution -- the same read-out
    over the state of the factorised forward."""
    K, seed, first = _sample_args(num_samples, seed, first_sample, "monotonic_rnnt_sample")
    acts = acts.detach()
    prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment, blank_label)
    L = _readout_length(prep, max_input_length, "monotonic_rnnt_sample")
    if K < 1:
        raise RuntimeError(f"monotonic_rnnt_sample: num_samples must be >= 1, got {K}")
    costs, ws = _forward(prep, with_beta=True, hat=blank_factorized)
    B, dev = prep.problem.B, prep.device
    out = torch.empty((B, K, L), dtype=torch.int32, device=dev)
    path_costs = torch.empty((B, K), dtype=torch.float32, device=dev)
    _call(prep, "sample", _ptr(ws), K, seed, first, _ptr(out), L, _ptr(path_costs))
    return Samples(out, path_costs, costs)


def _path_alignments(alignments: torch.Tensor, dev: torch.device, B: int, who: str) -> torch.Tensor:
    """The alignment rows as the path entry points take them: int32 [B, K >= 1, L >= 1], contiguous, on dev."""
    al = alignments.detach()
    if al.device != dev or al.dtype != torch.int32:
        al = al.to(dev, torch.int32)
    if al.dim() != 3 or al.size(0) != B:
        raise RuntimeError(f"{who}: alignments must be [B = {B}, K, L], got {tuple(al.shape)}")
    al = al.contiguous()
    if al.size(1) < 1 or al.size(2) < 1:
        raise RuntimeError(f"{who}: alignments needs K >= 1 paths of L >= 1 frames, got {al.size(1)}, {al.size(2)}")
    return al


def _upstream(g: Optional[torch.Tensor], prep) -> Optional[torch.Tensor]:
    """An upstream gradient as the backward entry points take it: float32, contiguous, on the call's device."""
    return None if g is None else g.detach().to(prep.device, torch.float32).contiguous()


class MonotonicRNNTPathFunction(torch.autograd.Function):
    """Scores of given alignments with their logit gradient (mrnnt_path_forward / mrnnt_path_backward and the
    mrnnt_cpu_path_* twins, include/mrnnt.h): apply(acts, labels, input_lengths, label_lengths, alignments,
    blank_label=0, blank_factorized=False) -> path_costs [B, K]. The upstream gradient of path_costs is the kernels'
    weights w[b, k]. blank_factorized: the mrnnt_hat_path_* / mrnnt_cpu_hat_path_* entry points."""

    @staticmethod
    def forward(ctx, acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                label_lengths: torch.Tensor, alignments: torch.Tensor, blank_label: int = 0,
                blank_factorized: bool = False) -> torch.Tensor:
        prep = _Prepared(acts, labels, input_lengths, label_lengths, None, 0, blank_label)
        hat = "hat_" if blank_factorized else ""
        B, dev = prep.problem.B, prep.device
        al = _path_alignments(alignments, dev, B, "monotonic_rnnt_path_loss")
        K, L = al.size(1), al.size(2)
        ws = prep.workspace(num_paths=K)
        costs = torch.empty((B, K), dtype=torch.float32, device=dev)
        _call(prep, hat + "path_forward", _ptr(ws), ws.numel(), _ptr(al), K, L, _ptr(costs), pending=True)
        if ctx.needs_input_grad[0]:
            # acts is re-read by the gradient kernel on the rows the paths visit; the workspace holds den, the hull
            # and the paths' validity
            ctx.save_for_backward(acts, ws, al)
            ctx.prep, ctx.hat = prep, hat
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        _, ws, al = ctx.saved_tensors
        prep, hat = ctx.prep, ctx.hat
        K, L = al.size(1), al.size(2)
        w = _upstream(grad_costs, prep)
        grads = _tracked_backward(prep, hat + "path_backward", (_ptr(ws), ws.numel(), _ptr(al), K, L, _ptr(w)))
        return grads, None, None, None, None, None, None


def monotonic_rnnt_path_loss(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                             label_lengths: torch.Tensor, alignments: torch.Tensor,
                             blank_label: int = 0, blank_factorized: bool = False) -> torch.Tensor:
    """Differentiable scores of given alignments: path_costs[b, k] = -log p(alignment (b, k) | acts), the negative
    log-probability of that one path through the lattice the loss sums over, with a gradient with respect to acts.
    The missing piece between the read-outs (monotonic_rnnt_align, monotonic_rnnt_sample: not differentiable) and
    training on their paths: Viterbi training (K = 1), risk-weighted / MWER / REINFORCE objectives over sampled paths
    (the upstream gradient of each path cost may have either sign), latency penalties. One forward and one dense
    gradient pass whatever K is:

        s = monotonic_rnnt_sample(acts, labels, T, S, num_samples=8, seed=step)
        pc = monotonic_rnnt_path_loss(acts, labels, T, S, s.alignments)          # [B, 8], differentiable
        (risk(s.alignments).detach() * torch.softmax(-pc, 1)).sum().backward()

    Args: acts, labels, input_lengths, label_lengths, blank_label as monotonic_rnnt_loss (CPU or GPU tensors; GPU: also
    bfloat16 / float16 acts, the padded 4-D layout, GPU-resident lengths without a host read).
        alignments: int [B, K, L] (returns [B, K]) or [B, L] (returns [B]), L >= every T_b, in the format
                    monotonic_rnnt_align / monotonic_rnnt_sample return: entry t < T_b is blank_label or the label
                    frame t emits; entries at t >= T_b are ignored.
    A row that is no path of its utterance (a wrong or negative label, a -1 sentinel row, too few or too many labels)
    costs +inf and gets no gradient whatever its upstream gradient is. A path through a -inf logit costs +inf; a NaN
    logit on a visited row makes the visiting paths' costs and that row's gradient NaN and nothing else. Rows no valid
    path with a non-zero upstream gradient visits have an exactly zero gradient and are not read. Costs and gradients
    are bitwise reproducible. GPU-resident lengths that fail validation (T_b <= L included) make every value NaN and
    surface through check_lengths() exactly as for the loss.
    blank_factorized=True: the scores and their gradient under monotonic_rnnt_hat_loss's distribution (blank a Bernoulli
    on its own logit, the labels a softmax over the others) -- the distribution that monotonic_rnnt_sample / _align
    (blank_factorized=True) draw and search under -- with the same kernels around a factorised log-softmax and gradient
    pass; a row whose non-blank logits are all -inf has no label arc and only its blank element gets a gradient."""
    if alignments.dim() == 2:
        out = MonotonicRNNTPathFunction.apply(acts, labels, input_lengths, label_lengths, alignments.unsqueeze(1),
                                              blank_label, blank_factorized)
        return out.squeeze(1)
    return MonotonicRNNTPathFunction.apply(acts, labels, input_lengths, label_lengths, alignments, blank_label,
                                           blank_factorized)


def _cost_array(x: Optional[torch.Tensor], prep: _Prepared, what: str) -> Optional[torch.Tensor]:
    """A per-arc cost array as the library takes it: float32, one value per row of acts, on acts' device."""
    if x is None:
        return None
    rows = tuple(prep.acts.shape[:-1])
    if tuple(x.shape) != rows:
        raise RuntimeError(f"monotonic_rnnt_expected_cost: {what} must have one value per row of acts, shape "
                           f"{rows}, got {tuple(x.shape)}")
    return x.detach().to(prep.device, torch.float32).contiguous()


class MonotonicRNNTExpectedCostFunction(torch.autograd.Function):
    """Expected path costs and the loss with their logit gradient (mrnnt_expect_forward / mrnnt_expect_backward and the
    mrnnt_cpu_expect_* twins, include/mrnnt.h): apply(acts, labels, input_lengths, label_lengths, blank_costs,
    label_costs, alignment=None, max_distance_from_alignment=0, blank_label=0, blank_factorized=False) ->
    (expected [B], costs [B]). The two upstream gradients go into one backward call that writes one gradient buffer.
    blank_factorized: the mrnnt_hat_expect_* / mrnnt_cpu_hat_expect_* entry points."""

    @staticmethod
    def forward(ctx, acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                label_lengths: torch.Tensor, blank_costs: Optional[torch.Tensor] = None,
                label_costs: Optional[torch.Tensor] = None, alignment: Optional[torch.Tensor] = None,
                max_distance_from_alignment: int = 0, blank_label: int = 0, blank_factorized: bool = False):
        prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment,
                         blank_label)
        hat = "hat_" if blank_factorized else ""
        wb = _cost_array(blank_costs, prep, "blank_costs")
        we = _cost_array(label_costs, prep, "label_costs")
        need_grad = bool(ctx.needs_input_grad[0])
        ws = prep.workspace(expect=True)
        B, dev = prep.problem.B, prep.device
        expected = torch.empty(B, dtype=torch.float32, device=dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        _call(prep, hat + "expect_forward", _ptr(ws), ws.numel(), _ptr(wb), _ptr(we), _ptr(expected), _ptr(costs),
              1 if need_grad else 0, pending=True)
        if need_grad:
            # acts is re-read by the gradient kernel; the workspace holds the loss's state and A / Bk / R
            ctx.save_for_backward(acts, ws)
            ctx.prep, ctx.wb, ctx.we, ctx.hat = prep, wb, we, hat
        return expected, costs

    @staticmethod
    def backward(ctx, grad_expected, grad_costs):
        _, ws = ctx.saved_tensors
        prep, hat = ctx.prep, ctx.hat
        ge, gc = _upstream(grad_expected, prep), _upstream(grad_costs, prep)
        grads = _tracked_backward(prep, hat + "expect_backward",
                                  (_ptr(ws), ws.numel(), _ptr(ctx.wb), _ptr(ctx.we), _ptr(ge), _ptr(gc)))
        return grads, None, None, None, None, None, None, None, None, None


def monotonic_rnnt_expected_cost(acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                                 label_lengths: torch.Tensor, blank_costs: Optional[torch.Tensor] = None,
                                 label_costs: Optional[torch.Tensor] = None,
                                 alignment: Optional[torch.Tensor] = None, max_distance_from_alignment: int = 0,
                                 blank_label: int = 0, blank_factorized: bool = False):
    """The exact expectation, under the path posterior p(path | labels, acts) of the lattice the loss sums over, of a
    cost that adds up over the arcs of a path -- and the loss of the same inputs -- both differentiable with respect to
    acts (the first-order expectation semiring: one more recursion over the forward's state, no sampling):

        expected[b] = sum_path p(path) sum_t cost(arc_t)      (= sum_rows blank_post * blank_costs + label_post * label_costs
                                                                 with monotonic_rnnt_posteriors of the same inputs)

    Emission time gives the expected latency streaming models are regularised with, blank_costs = 1 the expected blank
    count, a per-arc risk a minimum-risk objective:

        t = torch.arange(T_max).view(1, -1, 1).expand(B, T_max, S_max + 1)           # padded 4-D acts
        latency, costs = monotonic_rnnt_expected_cost(acts, labels, T, S, label_costs=t.float())
        (costs + 0.01 * latency).sum().backward()                                     # one gradient pass, one buffer

    Args: acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment, blank_label as
    monotonic_rnnt_loss (CPU or GPU tensors; GPU: also bfloat16 / float16 acts, the padded 4-D layout, GPU-resident
    lengths without a host read). With `alignment` the expectation is under the restricted distribution.
        blank_costs, label_costs: float tensors of shape acts.shape[:-1] -- one value per lattice row (b, t, s), the
                    layout of monotonic_rnnt_posteriors' blank / label -- the cost of the blank arc / the label arc out
                    of that row; either may be None (all zeros). Signed costs are fine. label_costs at s = S_b and
                    anything at padding rows is ignored.
    Returns (expected, costs), both float32 [B] on acts.device; costs is monotonic_rnnt_loss's (bit-identical).
    The backward of any function of the two is ONE call that writes ONE gradient buffer (the loss's own gradient folded
    into the same dense pass). The cost arrays are not differentiated: their gradient is the arc posteriors
    (monotonic_rnnt_posteriors). Rows outside the band, unreachable rows and rows whose coefficients underflow have an
    exactly zero gradient and are not read. An utterance without a finite cost has a NaN expected value and NaN gradient
    rows; the others are unaffected. Results are bitwise reproducible and do not depend on the other utterances.
    GPU-resident lengths that fail validation make every value NaN and surface through check_lengths() as for the
    loss.
    blank_factorized=True: the expectation, the costs (monotonic_rnnt_hat_loss's, bit-identical) and the gradient under
    the factorised-blank distribution of monotonic_rnnt_hat_loss -- the expected-latency regulariser of a HAT model."""
    return MonotonicRNNTExpectedCostFunction.apply(acts, labels, input_lengths, label_lengths, blank_costs, label_costs,
                                                   alignment, max_distance_from_alignment, blank_label,
                                                   blank_factorized)


class MonotonicRNNTLoss(torch.nn.Module):
    """reference monotonic_rnnt_op.py:166-217 (with the self.blank -> self.blank_label fix)."""

    function = MonotonicRNNTFunction

    def __init__(self, blank_label: int = 0) -> None:
        super().__init__()
        self.blank_label = blank_label
        self.loss = self.function.apply

    def forward(self, acts: torch.Tensor, labels: torch.Tensor, input_lengths: torch.Tensor,
                label_lengths: torch.Tensor, alignment: Optional[torch.Tensor] = None,
                max_distance_from_alignment: int = 0) -> torch.Tensor:
        loss = self.loss(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment,
                         self.blank_label)
        assert loss is not None
        return loss


class MonotonicRNNTHatLoss(MonotonicRNNTLoss):
    """monotonic_rnnt_hat_loss as a module, in the shape of MonotonicRNNTLoss."""

    function = MonotonicRNNTHatFunction


class _Ext:
    """The reference's pybind extension functions (monotonic_rnnt.cu:155-164), same argument order.

    gpu_*: acts on the GPU (the reference's TORCH_CHECK, :85; labels / lengths may be host or device tensors,
    the reference requires device ones); costs may live on any device (the reference takes a host tensor);
    grads [N, V] on the GPU, an empty tensor = cost only.
    cpu_*: every tensor on the host (the reference's cpu_monotonic_rnnt, :16-77); num_threads > 0 sets the
    thread count of the call. grads may also be acts itself (gradient written in place over the logits).
    Return 0 (RNNT_STATUS_SUCCESS) or raise RuntimeError.
    """

    @staticmethod
    def _run(acts, labels, input_lengths, label_lengths, alignment, k, costs, grads, blank_label, num_threads,
             want_gpu):
        if acts.is_cuda != want_gpu:  # labels / lengths may live on either device (copied as needed)
            raise RuntimeError(f"{'gpu' if want_gpu else 'cpu'}_monotonic_rnnt: acts must be a "
                               f"{'GPU' if want_gpu else 'CPU'} tensor")
        prep = _Prepared(acts, labels, input_lengths, label_lengths, alignment, k, blank_label, num_threads)
        want = grads is not None and grads.numel() > 0
        if want:
            if grads.device != prep.device or grads.dtype != prep.acts.dtype or not grads.is_contiguous():
                raise RuntimeError(f"grads must be a contiguous {prep.acts.dtype} tensor on {prep.device}")
            if grads.shape != prep.acts.shape:
                raise RuntimeError(f"grads must have the shape of acts {tuple(prep.acts.shape)}")
        c, ws = _forward(prep, with_beta=want)
        if want:
            _backward(prep, ws, None, grads)
        costs.copy_(c)
        return _L.RNNT_STATUS_SUCCESS

    def gpu_monotonic_rnnt(self, acts, labels, input_lengths, label_lengths, costs, grads, blank_label,
                           num_threads=0):
        return self._run(acts, labels, input_lengths, label_lengths, None, 0, costs, grads, blank_label, 0, True)

    def gpu_monotonic_rnnt_align_restrict(self, acts, labels, input_lengths, label_lengths, alignment,
                                          max_distance_from_alignment, costs, grads, blank_label, num_threads=0):
        return self._run(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment,
                         costs, grads, blank_label, 0, True)

    def cpu_monotonic_rnnt(self, acts, labels, input_lengths, label_lengths, costs, grads, blank_label,
                           num_threads=0):
        return self._run(acts, labels, input_lengths, label_lengths, None, 0, costs, grads, blank_label,
                         num_threads, False)

    def cpu_monotonic_rnnt_align_restrict(self, acts, labels, input_lengths, label_lengths, alignment,
                                          max_distance_from_alignment, costs, grads, blank_label, num_threads=0):
        return self._run(acts, labels, input_lengths, label_lengths, alignment, max_distance_from_alignment,
                         costs, grads, blank_label, num_threads, False)


monotonic_rnnt_cpp = _Ext()

__all__ = ["MonotonicRNNTFunction", "monotonic_rnnt_loss", "MonotonicRNNTLoss", "monotonic_rnnt_cpp", "check_lengths",
           "monotonic_rnnt_align", "monotonic_rnnt_posteriors", "monotonic_rnnt_sample",
           "MonotonicRNNTPathFunction", "monotonic_rnnt_path_loss", "MonotonicRNNTExpectedCostFunction",
           "monotonic_rnnt_expected_cost", "MonotonicRNNTHatFunction", "monotonic_rnnt_hat_loss",
           "MonotonicRNNTHatLoss"]
