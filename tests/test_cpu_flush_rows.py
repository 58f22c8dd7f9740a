"""The host path's flush-dead rows (mrnnt_cpu.cpp LossRows, mrnnt_host.h kFlushLnCpu): a row whose largest possible
exponent c - den is below -87 - 2^-6 and whose blank / label corrections are 0 in fp32 is stored as 0 * grad_scale
without reading acts, because vexp returns exactly 0 below -87. The gradient's bits do not depend on the rule: the
development build switches it off (mrnnt_cpu_flush_rows) and the result is compared bit for bit, signed zeros included.

Shapes: seeded normal logits x scale with many rows of log-occupancy in [-110, -87.6) (counted from the oracle's fp64
alpha / beta, so the comparison cannot pass without rows the rule decides), plus an S = 0 utterance, which has none."""
import numpy as np
import pytest
import torch

import oracle as O
from _flush_rows import window_rows
from _parity import assert_costs, assert_grads

# (T, S, V, scale): the window counts of the first utterance are 1,487 and 296
SHAPES = {"t400_s80_v64_x3": (400, 80, 64, 3.0), "t200_s60_v1024_x1": (200, 60, 1024, 1.0)}


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


def _run(op, acts, labels, T, S, scale):
    a = torch.from_numpy(acts).requires_grad_(True)
    c = op.monotonic_rnnt_loss(a, torch.from_numpy(labels), torch.from_numpy(T), torch.from_numpy(S))
    (c * torch.from_numpy(scale)).sum().backward()
    return c.detach().numpy().copy(), a.grad.numpy().copy()


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_gradient_is_bit_identical_with_the_rule_on_and_off(op, name):
    import _mrnnt_lib as L
    Tb, Sb, V, mul = SHAPES[name]
    rng = np.random.default_rng(606)
    T, S = np.array([Tb, Tb, 23], np.int32), np.array([Sb, Sb, 0], np.int32)
    rows = int(np.sum(T * (S + 1)))
    acts = (mul * rng.standard_normal((rows, V))).astype(np.float32)
    labels = rng.integers(1, V, (3, int(S.max()))).astype(np.int32)
    scale = np.array([1.0, -0.5, 2.0], np.float32)
    cr, gr, _, al, be = O.oracle_rnnt(acts, labels, T, S, num_threads=4, debug=True)
    win = window_rows(al, be, cr, T, S)
    print(f"{name}: rows with -110 <= log-occupancy < -87.6 per utterance: {win}")
    assert win[0] >= 100 and win[1] >= 100 and win[2] == 0, win
    # the rows on which the host rule provably fires: its two corrections are IEEE, e^x <= occupancy, and round to 0
    # in fp32 only below e^-103.97 (half the smallest denormal), so the rule needs log-occupancy below about -104;
    # at [-110, -104.5) c - den = log-occupancy < -87.02 and cb = ce = 0 hold with half a nat to spare
    deep = window_rows(al, be, cr, T, S, hi=-104.5)
    print(f"{name}: rows with -110 <= log-occupancy < -104.5 per utterance: {deep}")
    assert deep[0] >= 30 and deep[1] >= 30, deep
    with L.use(L.load_dev()):
        lib = L.load()
        assert lib.mrnnt_cpu_flush_rows(-1) == 1  # on by default
        on = _run(op, acts, labels, T, S, scale)
        assert lib.mrnnt_cpu_flush_rows(0) == 1
        try:
            off = _run(op, acts, labels, T, S, scale)
        finally:
            lib.mrnnt_cpu_flush_rows(1)
    product = _run(op, acts, labels, T, S, scale)
    for got in (on, product):
        assert np.array_equal(got[0].view(np.uint32), off[0].view(np.uint32))
        assert np.array_equal(got[1].view(np.uint32), off[1].view(np.uint32))  # signed zeros included
    assert_costs(on[0], cr)
    assert_grads(on[1], gr * np.repeat(scale.astype(np.float64), T * (S + 1))[:, None])


def test_product_library_has_no_switch():
    import _mrnnt_lib as L
    assert not hasattr(L.load(), "mrnnt_cpu_flush_rows")
    assert L.load_dev().mrnnt_cpu_flush_rows(-1) == 1
