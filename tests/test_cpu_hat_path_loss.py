"""monotonic_rnnt_path_loss(blank_factorized=True) on the host implementation (mrnnt_cpu_hat_path_forward /
mrnnt_cpu_hat_path_backward): the shared checks of tests/_hat_weight_checks.py on CPU tensors. No GPU needed."""
import pytest

import _hat_checks as H
import _hat_weight_checks as C
import _parity as P

DEV = C.Dev("cpu")
VS = [5, 64, 512, 1024]


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("V,blank", [(V, b) for V in VS for b in H.blank_positions(V)])
def test_parity_with_the_yardstick(V, blank, K):
    C.check_path_parity(DEV, V, blank, K)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 0)])
def test_transform_identity(V, blank):
    C.check_transform_identity(DEV, V, blank)


def test_signed_weights():
    C.check_signed_weights(DEV)


@pytest.mark.parametrize("zb", [60.0, 100.0, -60.0, -100.0])
@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63)])
def test_dominant_and_suppressed_blank(V, blank, zb):
    C.check_blank_logit(DEV, V, blank, zb)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 47)])
def test_non_finite_logits(V, blank):
    C.check_path_non_finite(DEV, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 4), (64, 0), (100, 98), (1028, 1024)])
def test_consistency_with_sample_and_align(V, blank):
    C.check_path_consistency(DEV, V, blank)


def test_reproducible_and_independent_of_the_batch():
    """... and of where the gradient goes: it may be written over the logits (the C entry point, grads = acts)."""
    import monotonic_rnnt_op
    C.check_path_reproducible(DEV, 64, 47)
    P.check_gradient_in_place(monotonic_rnnt_op, "hat_path_")
