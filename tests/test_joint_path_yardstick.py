"""The yardstick of the joint path-loss tests (tests/_joint_path_checks.py) against torch.autograd: its hand-written
chain (dweight = dz^T h, dbias = sum dz, dpre = (dz weight)(1 - h^2), d_enc / d_pred sums) agrees with autograd through
the fp64 composition, the roundings passing gradients straight through, within 1e-9 -- so the yardstick is checked
without a GPU before anything is measured against it."""
import numpy as np
import pytest

import _joint_path_checks as JC
import _path_checks as PC

TOL = 1e-9


def _paths(labels, T, S, blank, rng, K):
    """The two extreme paths, then random valid paths (a random choice of the frames that emit); one row spoiled."""
    L = int(T.max())
    al = np.full((len(T), K, L), blank, np.int32)
    al[:, :2] = JC.extreme_paths(labels, T, S, L, blank)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        for k in range(2, K):
            frames = np.sort(rng.choice(int(Tb), int(Sb), replace=False))
            al[b, k, frames] = labels[b, :Sb]
    al[0, K - 1] = -1  # an invalid row: +inf, no gradient whatever its weight
    return al


@pytest.mark.parametrize("seed,shapes,H,V,blank", [(1, [(7, 3), (1, 0), (4, 4)], 16, 11, 0),
                                                   (2, [(9, 2), (5, 5), (3, 0), (6, 1)], 24, 7, 6)])
def test_chain_agrees_with_autograd(seed, shapes, H, V, blank):
    enc, pred, w, bias, labels, T, S = JC.make_case(seed, shapes, H, V, blank)
    rng = np.random.default_rng(seed)
    K = 5
    al = _paths(labels, T, S, blank, rng, K)
    wts = rng.standard_normal((len(T), K))
    c, de, dp, dw, db = JC.yardstick(enc, pred, w, bias, labels, T, S, al, wts, blank)
    cr, de_r, dp_r, dw_r, db_r = JC.autograd_reference(enc, pred, w, bias, labels, T, S, al, wts, blank)
    assert np.isinf(c[0, K - 1]) and np.isinf(cr[0, K - 1])
    fin = np.isfinite(cr)
    assert np.array_equal(np.isfinite(c), fin) and fin.sum() == fin.size - 1
    assert np.abs(c[fin] - cr[fin]).max() <= TOL * np.maximum(1.0, np.abs(cr[fin])).max()
    for x, r, name in ((de, de_r, "d_enc"), (dp, dp_r, "d_pred"), (dw, dw_r, "d_weight"), (db, db_r, "d_bias")):
        err = (x - r).abs().max().item()
        print(name, err, r.abs().max().item())
        assert r.abs().max().item() > 1e-3, name      # a gradient is there to compare
        assert err <= TOL * max(1.0, r.abs().max().item()), (name, err)
    # padding frames / label slots get nothing
    for b in range(len(T)):
        assert (de[b, T[b]:] == 0).all() and (dp[b, S[b] + 1:] == 0).all()


def test_blank_exchange_matches_default_blank():
    """path_yardstick's vocabulary exchange: a problem with blank = V - 1 is the default-blank problem with the two
    entries exchanged -- checked against the direct walk (walk takes the blank) on the costs."""
    blank, V = 6, 7
    enc, pred, w, bias, labels, T, S = JC.make_case(3, [(8, 3), (4, 4), (2, 0)], 16, V, blank)
    al = JC.extreme_paths(labels, T, S, int(T.max()), blank)
    _, acts = JC.joint_logits(enc, pred, w, bias, T, S)
    costs, dz = JC.path_yardstick(acts, labels, T, S, al, None, blank)
    lsm = acts.astype(np.float64) - np.log(np.exp(acts.astype(np.float64)).sum(1, keepdims=True))
    off = PC.offsets(T, S)
    for b in range(len(T)):
        for k in range(2):
            rows, cols = PC.walk(al[b, k], labels[b], int(T[b]), int(S[b]), blank)
            assert abs(costs[b, k] + lsm[np.asarray(rows) + off[b], cols].sum()) <= 1e-9
    assert abs(dz.sum()) <= 1e-9  # every row's gradient sums to Wocc - Wb - We = 0
