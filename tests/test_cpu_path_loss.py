"""monotonic_rnnt_path_loss on the host implementation (mrnnt_cpu_path_forward / mrnnt_cpu_path_backward): the shared
checks of tests/_path_checks.py on CPU tensors. No GPU needed."""
import numpy as np
import pytest
import torch

import _align_checks as A
import _path_checks as C
import _sample_checks as SC


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


@pytest.mark.parametrize("name", [c[0] for c in C.EDGE_CASES])
def test_edge_shapes_against_the_yardstick(op, name):
    C.check_edge_case(C.run_cpu, name)


def test_signed_weights_and_cancellation(op):
    C.check_signed_weights(C.run_cpu)


def test_invalid_rows(op):
    C.check_invalid_rows(C.run_cpu)


def test_padded_layout_bit_identical_to_packed(op):
    C.check_padded(C.run_cpu)


def _loss_grad(acts, labels, T, S, al):
    import monotonic_rnnt_op as op
    a = torch.from_numpy(acts).requires_grad_(True)
    op.monotonic_rnnt_loss(a, torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S),
                           torch.from_numpy(al), 0).sum().backward()
    return a.grad.numpy().astype(np.float64)


def test_consistency_with_align_sample_and_the_restricted_loss(op):
    C.check_consistency(C.run_cpu, A.run_cpu, SC.run_cpu, _loss_grad)


def test_non_finite_logits(op):
    C.check_non_finite(C.run_cpu)


def test_reproducible(op):
    C.check_reproducible(C.run_cpu)


def test_surface(op):
    """[B, L] alignments give [B]; acts without requires_grad give plain costs; int64 alignments are converted; the
    gradient may be written over the logits (the C entry point, grads = acts)."""
    import ctypes

    import _mrnnt_lib as L
    acts, labels, T, S, al, w = C.small_problem(seed=27, K=4)
    args = (torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S))
    pc = op.monotonic_rnnt_path_loss(torch.from_numpy(acts), *args, torch.from_numpy(al))
    assert not pc.requires_grad and tuple(pc.shape) == (4, 4)
    one = op.monotonic_rnnt_path_loss(torch.from_numpy(acts), *args, torch.from_numpy(al[:, 1]).to(torch.int64))
    assert tuple(one.shape) == (4,) and one.numpy().tobytes() == pc[:, 1].contiguous().numpy().tobytes()
    with pytest.raises(RuntimeError, match="alignments"):
        op.monotonic_rnnt_path_loss(torch.from_numpy(acts), *args, torch.from_numpy(al[:3]))
    with pytest.raises(RuntimeError, match="alignments row stride"):
        op.monotonic_rnnt_path_loss(torch.from_numpy(acts), *args, torch.from_numpy(np.ascontiguousarray(al[:, :, :29])))
    # in place: grads = acts
    c, g = C.run_cpu(acts, labels, T, S, al, w)
    buf = torch.from_numpy(acts.copy())
    prep = op._Prepared(buf, *args, None, 0, C.BLANK)
    ws = prep.workspace(num_paths=4)
    alt, wt, out = torch.from_numpy(al), torch.from_numpy(w), torch.empty(4, 4)
    vp = ctypes.c_void_p
    lib = L.load()
    L.check(lib.mrnnt_cpu_path_forward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(alt.data_ptr()), 4,
                                       al.shape[2], vp(out.data_ptr()), 0), "forward")
    L.check(lib.mrnnt_cpu_path_backward(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(alt.data_ptr()), 4,
                                        al.shape[2], vp(wt.data_ptr()), vp(buf.data_ptr()), 0), "backward")
    assert out.numpy().tobytes() == c.tobytes() and buf.numpy().tobytes() == g.tobytes()
