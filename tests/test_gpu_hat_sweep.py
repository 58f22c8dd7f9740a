"""The factorised-blank (HAT) loss, path scores and expected costs on the GPU over ragged V and long S: the directed
table and the seeded random sweep of tests/_hat_sweep.py (the table of (type, V) -> kernel branch, the yardstick and the
tolerances are in its docstring), and what the earlier HAT tests left out: misaligned acts, B = 300, a label equal to
the blank, the tracked backward on ragged rows.
Long sweeps: MRNNT_HAT_FUZZ_CASES / MRNNT_HAT_FUZZ_FIRST, as MRNNT_FUZZ_CASES / MRNNT_FUZZ_FIRST of test_gpu_fuzz.py."""
import pytest
import torch

import _hat_checks as H
import _hat_sweep as W
import _hat_weight_checks as C

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return C.Dev("cuda:0")


@pytest.mark.parametrize("dtype,V,blank", W.DIRECTED)
def test_directed(dev, dtype, V, blank):
    W.check_directed(dev, dtype, V, blank)


@pytest.mark.parametrize("seed", range(W.FIRST, W.FIRST + W.N_CASES))
def test_random_case(dev, seed):
    W.check_random(dev, seed)


@pytest.mark.parametrize("dtype,V", [("f32", 1024), ("bf16", 2048)])
def test_misaligned_acts(dev, dtype, V):
    """acts viewed 4 bytes past a 16-byte boundary take the scalar kernels at a V the vector kernels would: four and
    eight 256-strides, the blank (3V/4 - 1 = 767 / 1535) in a later one."""
    c = W.directed_case(dtype, V, (3 * V) // 4 - 1)
    c["unaligned"] = True
    W.check_loss(dev, c, cost_only_too=True)
    W.check_path(dev, c, 3)
    W.check_expect(dev, c)


def test_many_utterances(dev):
    c = W.many_utterances_case()
    W.check_loss(dev, c, cost_only_too=True)
    W.check_expect(dev, c)


@pytest.mark.parametrize("V,blank", [(5, 2), (100, 98), (1028, 1024)])
def test_label_equal_to_blank_is_no_arc(dev, V, blank):
    W.check_label_equal_to_blank(dev, V, blank)


@pytest.mark.parametrize("V,blank,padded", [(1000, 749, False), (1000, 999, True), (257, 256, False)])
def test_tracked_backward_on_ragged_rows(V, blank, padded):
    """test_gpu_hat.py::test_tracked_backward_equals_untracked on rows that are no whole number of chunks: at V = 1000
    the staged kernel runs with a ragged tail and keeps the row state; at V = 257 the scalar kernel runs and every state
    byte stays 0 ("unknown"). The buffers are byte-equal over two calls."""
    import monotonic_rnnt_op as op
    run = H.Runner(op, torch.device("cuda:0"))
    acts, labels = H.problem(V, blank, seed=9)
    a = run.acts(acts, padded=padded)
    lab, T, S = run.tensors(labels, False)
    prep = op._Prepared(a, lab, T, S, None, 0, blank)
    _, ws = op._forward(prep, with_beta=True, hat=True)
    plain = op._backward(prep, ws, None, torch.full_like(a, 7.0), hat=True)
    g = plain.cpu().numpy()
    H.assert_grads(H.padded_to_packed(g) if padded else g, H.reference(acts, labels, blank)[1])
    rows = a.numel() // V
    state =torch.zeros(rows, dtype=torch.uint8, device=a.device)
    buf = torch.full_like(a, 5.0)
    for _ in range(2):
        op._call(prep, "hat_backward_tracked", op._ptr(ws), None, op._ptr(buf), op._ptr(state), rows, lengths=False)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert int(state.max()) == (1 if V % 4 == 0 else 0)
