"""monotonic_rnnt_expected_cost(blank_factorized=True) on the host implementation (mrnnt_cpu_hat_expect_forward /
mrnnt_cpu_hat_expect_backward): the shared checks of tests/_hat_weight_checks.py on CPU tensors. No GPU needed."""
import pytest

import _hat_checks as H
import _hat_weight_checks as C
import _parity as P

DEV = C.Dev("cpu")
VS = [5, 64, 512, 1024]


@pytest.mark.parametrize("V,blank", [(V, b) for V in VS for b in H.blank_positions(V)])
def test_parity_with_the_dp_yardstick(V, blank):
    C.check_expect_parity(DEV, V, blank)


@pytest.mark.parametrize("V,blank", [(5, b) for b in H.blank_positions(5)])
def test_parity_with_path_enumeration(V, blank):
    C.check_expect_brute(DEV, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 47)])
def test_non_finite_logits(V, blank):
    C.check_expect_non_finite(DEV, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63), (100, 98), (1028, 1024)])
def test_consistency_with_posteriors_and_the_hat_loss(V, blank):
    C.check_expect_consistency(DEV, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 0)])
def test_restricting_alignment(V, blank):
    C.check_restriction(DEV, V, blank)


def test_reproducible_and_independent_of_the_batch():
    """... and of where the gradient goes: it may be written over the logits (the C entry point, grads = acts)."""
    import monotonic_rnnt_op
    C.check_expect_reproducible(DEV, 64, 47)
    P.check_gradient_in_place(monotonic_rnnt_op, "hat_expect_")
