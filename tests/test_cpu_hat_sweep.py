"""The sweep of tests/_hat_sweep.py on the host implementation (mrnnt_cpu_hat_*): the directed table and random seeds of
tests/test_gpu_hat_sweep.py through Dev("cpu"). No GPU needed. It shows that the generator, the yardstick and the
tolerances are sound before a kernel is asked to meet them. The host implementation takes float32 acts only: a bf16 /
fp16 case runs on its upcast values (the same yardstick, no rounding allowance), so of the directed table the float32
rows and the (V, blank) pairs only the reduced-precision rows have are run. Every random seed of the GPU file is run."""
import pytest

import _hat_sweep as W
import _hat_weight_checks as C

DEV = C.Dev("cpu")

_F32 = {(V, b) for d, V, b in W.DIRECTED if d == "f32"}
DIRECTED = [(d, V, b) for d, V, b in W.DIRECTED if d == "f32" or (d == "bf16" and (V, b) not in _F32)]
SEEDS = range(W.FIRST, W.FIRST + W.N_CASES)


@pytest.mark.parametrize("dtype,V,blank", DIRECTED)
def test_directed(dtype, V, blank):
    W.check_directed(DEV, dtype, V, blank)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_case(seed):
    W.check_random(DEV, seed)


def test_many_utterances():
    c = W.many_utterances_case()
    W.check_loss(DEV, c, cost_only_too=True)
    W.check_expect(DEV, c)


@pytest.mark.parametrize("V,blank", [(5, 2), (100, 98), (1028, 1024)])
def test_label_equal_to_blank_is_no_arc(V, blank):
    W.check_label_equal_to_blank(DEV, V, blank)
