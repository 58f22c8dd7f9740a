"""The factorised-blank (HAT) loss and its read-outs on CPU tensors (mrnnt_cpu_hat_*), against the fp64 oracle on
transformed logits (tests/_hat_checks.py). GPU-vs-CPU agreement follows through the common reference."""
import numpy as np
import pytest
import torch

import _hat_checks as H
import _parity as P


@pytest.fixture(scope="module")
def run():
    import monotonic_rnnt_op
    return H.Runner(monotonic_rnnt_op, torch.device("cpu"))


VS = [5, 64, 256, 512, 1024, 2048]
CASES = [(V, b) for V in VS for b in H.blank_positions(V)]


@pytest.mark.parametrize("V,blank", CASES)
def test_parity(run, V, blank):
    H.check_parity(run, V, blank)


@pytest.mark.parametrize("zb", [60.0, 100.0, -60.0, -100.0])
@pytest.mark.parametrize("V,blank", [(5, 2), (1024, 0)])
def test_dominant_and_suppressed_blank(run, V, blank, zb):
    H.check_blank_logit(run, V, blank, zb)


@pytest.mark.parametrize("V,blank", [(5, 4), (1024, 767)])
def test_label_shift(run, V, blank):
    H.check_label_shift(run, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 0), (64, 63), (2048, 1535)])
def test_closed_form(run, V, blank):
    H.check_closed_form(run, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 0), (256, 191)])
def test_non_finite(run, V, blank):
    H.check_non_finite(run, V, blank)


@pytest.mark.parametrize("V,blank,masked", H.MASKED_CASES, ids=[f"{v}-{b}" for v, b, _ in H.MASKED_CASES])
def test_masked_non_label_entries(run, V, blank, masked):
    H.check_masked_entries(run, V, blank, masked)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 0)])
def test_align_is_best_path(run, V, blank):
    H.check_align(run, V, blank)


def _tensors(run, acts, labels):
    lab, T, S = run.tensors(labels, False)
    return run.acts(acts), lab, T, S


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63)])
def test_posteriors(run, V, blank):
    def post(acts, labels, blank):
        r = run.op.monotonic_rnnt_posteriors(*_tensors(run, acts, labels), blank_label=blank, blank_factorized=True)
        return type(r)(*[x.numpy() for x in r])
    H.check_posteriors(post, V, blank)


@pytest.mark.parametrize("V,blank", [(5, 2), (64, 63)])
def test_sample_path_costs(run, V, blank):
    def sample(acts, labels, blank, K):
        r = run.op.monotonic_rnnt_sample(*_tensors(run, acts, labels), num_samples=K, seed=11, blank_label=blank,
                                         blank_factorized=True)
        return type(r)(*[x.numpy() for x in r])
    H.check_sample(sample, V, blank)


def test_standard_loss_differs(run):
    """The factorised distribution is another one: on the same logits the two losses disagree. Its gradient, like
    the standard one, may be written over the logits (the C entry point, grads = acts)."""
    P.check_gradient_in_place(run.op, "hat_")
    acts, labels = H.problem(64, 0)
    c, _, _ = run.loss(acts, labels, 0, grads=False)
    lab, T, S = run.tensors(labels, False)
    std = run.op.monotonic_rnnt_loss(run.acts(acts), lab, T, S).numpy()
    assert np.abs(c - std).min() > 1e-2
