"""The yardstick of the joint expected-cost tests (tests/_joint_expect_checks.py) against torch.autograd: the logit
gradient of _expect_checks.yardstick pushed through _joint_path_checks.chain agrees with autograd through the whole fp64
composition, the roundings passing gradients straight through, within 1e-9 (test_joint_path_yardstick.py's construction
and tolerance) -- with path enumeration on the T <= 7 utterances -- so the yardstick is checked without a GPU before
anything is measured against it. The banded recursion used under a restricting alignment is held to the unrestricted
yardstick (full bands) and to path enumeration (narrow bands)."""
import numpy as np
import pytest

import _align_checks as A
import _expect_checks as EC
import _joint_expect_checks as JE
import _joint_path_checks as JC

TOL = 1e-9
NAMES = ("d_enc", "d_pred", "d_weight", "d_bias")


def _compare(got, ref):
    for x, r, name in zip(got[:2], ref[:2], ("expected", "costs")):
        assert np.abs(x - r).max() <= TOL * np.maximum(1.0, np.abs(r)).max(), name
    for x, r, name in zip(got[2:], ref[2:], NAMES):
        err = (x - r).abs().max().item()
        print(name, err, r.abs().max().item())
        assert r.abs().max().item() > 1e-3, name      # a gradient is there to compare
        assert err <= TOL * max(1.0, r.abs().max().item()), (name, err)


@pytest.mark.parametrize("seed,shapes,H,V,blank", [(1, [(7, 3), (1, 0), (4, 4)], 16, 11, 0),
                                                   (2, [(9, 2), (5, 5), (3, 0), (6, 1)], 24, 7, 6)])
def test_chain_agrees_with_autograd(seed, shapes, H, V, blank):
    enc, pred, w, bias, labels, T, S = JC.make_case(seed, shapes, H, V, blank)
    rng = np.random.default_rng(seed)
    wb, we = JE.random_costs(rng, T, S)
    ge, gc = EC.upstreams(rng, len(T))
    got = JE.yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank)
    ref = JE.autograd_reference(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank)
    _compare(got, ref)
    for b in range(len(T)):  # padding frames / label slots get nothing
        assert (got[2][b, T[b]:] == 0).all() and (got[3][b, S[b] + 1:] == 0).all()
    # path enumeration on the utterances with T <= 7
    small = [b for b in range(len(T)) if T[b] <= 7]
    assert len(small) >= 2
    off = EC.offsets(T, S)
    rows = np.concatenate([np.arange(off[b], off[b + 1]) for b in small])
    sub = (enc[small], pred[small], w, bias, labels[small], T[small], S[small])
    args = (wb[rows], we[rows], ge[small], gc[small], blank)
    brute = JE.yardstick(*sub, *args, brute=True)
    _compare(JE.yardstick(*sub, *args), brute)
    _compare(brute, JE.autograd_reference(*sub, *args, brute=True))


def test_banded_recursion():
    blank, V = 6, 7
    enc, pred, w, bias, labels, T, S = JC.make_case(4, [(7, 3), (6, 2), (5, 5), (4, 0)], 16, V, blank)
    rng = np.random.default_rng(4)
    wb, we = JE.random_costs(rng, T, S)
    ge, gc = EC.upstreams(rng, len(T))
    logits = JC.joint_logits(enc, pred, w, bias, T, S)
    free = JE.yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank, logits=logits)
    full = [(np.zeros(t, int), np.full(t, s)) for t, s in zip(T, S)]
    _compare(JE.yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank, logits=logits, bands=full), free)
    # a band of width 1 around the all-labels-first path: fewer paths than the lattice has
    al = JC.extreme_paths(labels, T, S, int(T.max()), blank)[:, 0]
    bands = [A.band_of(al[b], int(T[b]), 1, blank) for b in range(len(T))]
    dp = JE.yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank, logits=logits, bands=bands)
    _compare(dp, JE.yardstick(enc, pred, w, bias, labels, T, S, wb, we, ge, gc, blank, logits=logits, bands=bands,
                              brute=True))
    assert dp[1][0] > free[1][0] + 1e-6  # (the restriction removed paths of utterance 0)


def test_grid_puts_garbage_where_nothing_is_read():
    T, S = np.array([3, 2], np.int32), np.array([1, 2], np.int32)
    n = int(EC.offsets(T, S)[-1])
    wb, we = np.arange(n, dtype=np.float32), -np.arange(n, dtype=np.float32)
    gb, ge = JE.grid(wb, we, T, S, 4, 4)
    assert gb.shape == ge.shape == (2, 4, 4)
    assert np.array_equal(gb[0, :3, :2].reshape(-1), wb[:6]) and np.array_equal(ge[1, :2, :2], we[6:].reshape(2, 3)[:, :2])
    assert np.all(gb[0, 3:] == JE.GARBAGE) and np.all(gb[0, :, 2:] == JE.GARBAGE) and np.all(gb[1, 2:] == JE.GARBAGE)
    assert np.all(ge[0, :, 1:] == JE.GARBAGE) and np.all(ge[1, :, 2:] == JE.GARBAGE)
    assert JE.grid(None, we, T, S, 4, 4)[0] is None and JE.grid(wb, None, T, S, 4, 4)[1] is None
