"""monotonic_rnnt_expected_cost on CPU tensors (mrnnt_cpu_expect_forward / mrnnt_cpu_expect_backward, csrc/mrnnt_cpu.cpp):
the shared checks of tests/_expect_checks.py on the host implementation. No GPU needed."""
import numpy as np
import pytest
import torch

import _expect_checks as C
import _parity as P


@pytest.fixture(scope="module")
def op():
    import monotonic_rnnt_op
    return monotonic_rnnt_op


@pytest.mark.parametrize("V", [5, 8])
def test_brute_force(op, V):
    C.check_brute(C.run_cpu, V)


@pytest.mark.parametrize("name", [c[0] for c in C.EDGE_CASES])
def test_edge_shapes_against_the_yardstick(op, name):
    C.check_edge_case(C.run_cpu, name)


def test_expected_is_the_posteriors_weighted_cost(op):
    C.check_posteriors_identity(C.run_cpu, C.posteriors_cpu)


def test_costs_output_is_the_loss(op):
    C.check_costs_identity(C.run_cpu, C.loss_cpu)


def test_constant_costs(op):
    C.check_constant_costs(C.run_cpu)


def test_negated_costs(op):
    C.check_negation(C.run_cpu)


def test_two_upstreams_in_one_pass(op):
    C.check_two_upstreams(C.run_cpu)


def test_restricting_alignment(op):
    C.check_restriction(C.run_cpu, C.posteriors_cpu)


def test_non_finite_logits(op):
    C.check_non_finite(C.run_cpu)


def test_reproducible_and_independent_of_the_batch(op):
    C.check_reproducible(C.run_cpu)


@pytest.mark.parametrize("V", [12, 7])
def test_padded_layout_bit_identical_to_packed(op, V):
    C.check_padded(C.run_cpu, V)


def test_absent_cost_arrays_and_no_grad(op):
    """Either cost array may be None (zeros); both None: expected = 0. Without requires_grad the outputs are plain.
    The gradient may be written over the logits (the C entry point, grads = acts)."""
    P.check_gradient_in_place(op, "expect_")
    acts, labels, T, S, wb, we = C.small_problem(seed=70)
    zero = np.zeros_like(wb)
    for x, y, xz, yz in ((None, we, zero, we), (wb, None, wb, zero), (None, None, zero, zero)):
        r1, r2 = C.run_cpu(acts, labels, T, S, x, y), C.run_cpu(acts, labels, T, S, xz, yz)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))
    assert np.all(r1[0] == 0.0)
    e, c = op.monotonic_rnnt_expected_cost(torch.from_numpy(acts), torch.from_numpy(labels), torch.from_numpy(T),
                                           torch.from_numpy(S), torch.from_numpy(wb), torch.from_numpy(we))
    assert not e.requires_grad and not c.requires_grad
    ref = C.run_cpu(acts, labels, T, S, wb, we)
    assert e.numpy().tobytes() == ref[0].tobytes() and c.numpy().tobytes() == ref[1].tobytes()
    with pytest.raises(RuntimeError, match="one value per row"):
        op.monotonic_rnnt_expected_cost(torch.from_numpy(acts), torch.from_numpy(labels), torch.from_numpy(T),
                                        torch.from_numpy(S), torch.from_numpy(wb[:-1]), None)
