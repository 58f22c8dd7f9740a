"""The host implementation (RNNT_CPU) on logits outside N(0,1): large offsets, peaked and constant rows, denormals,
-inf masks, NaN / +inf poison -- against the fp64 oracle, with the case builders and bounds of _value_domain.py.
Runs without a GPU.

The rule the poison tests pin: a non-finite cost has a class. +inf means "no alignment path" (a masked label, an
infeasible alignment); NaN means "bad input". A NaN or +inf logit in a row the recursion uses makes the oracle's cost
NaN, and the library must say NaN too -- never +inf, never a finite number -- and must leave the other utterances of
the batch bit for bit alone.
"""
import numpy as np
import pytest

import oracle as O
import _value_domain as D
from _parity import assert_grads
from test_cpu_parity import run_cpu

# B = 3, T in [6, 20], S <= 6; one utterance with S = 0, one with T = S
FORCE = {0: (17, 5), 1: (13, 0), 2: (6, 6)}
VS = [8, 64, 257]


def problem(V, seed=0):
    return D.base_problem(40 + seed + V, 3, (6, 20), 6, V, force=FORCE)


_CLEAN = {}


def clean(V):
    """The base problem of V with the library's and the oracle's results on it, computed once."""
    if V not in _CLEAN:
        acts, labels, T, S = problem(V)
        _CLEAN[V] = (acts, labels, T, S, run_cpu(acts, labels, T, S), O.oracle_rnnt(acts, labels, T, S))
    return _CLEAN[V]


FINITE = ([D.offset(M) for M in D.OFFSETS] + [D.row_offsets(M) for M in D.ROW_OFFSETS] +
          [D.scale(k) for k in D.SCALES] + [D.constant(c) for c in D.CONSTANTS] + [D.denormal, D.mask_unused(0.5)])


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("tf", FINITE, ids=[f.__name__ for f in FINITE])
def test_finite_transforms_vs_oracle(tf, V):
    acts, labels, T, S = clean(V)[:4]
    x = tf(acts, labels, T, S)
    c, g = run_cpu(x, labels, T, S)
    cr, gr = O.oracle_rnnt(x, labels, T, S)
    tol_c, (tol_g, _) = D.cost_tol(cr, T, x), D.grad_tol(x)
    print(f"{tf.__name__} V={V}: cost err {np.abs(c - cr).max():.3e} (tol {tol_c.min():.3e}), "
          f"grad err {np.abs(g - gr).max():.3e} (tol {tol_g:.3e})")
    D.assert_costs_classed(c, cr, tol_c)
    assert_grads(g, gr, tol=tol_g)
    if tf.__name__.startswith("constant"):
        closed = np.array([D.closed_form_cost(t, s, V) for t, s in zip(T, S)])
        assert np.all(np.abs(cr - closed) <= 1e-9 * closed), (cr, closed)  # the oracle itself
        assert np.all(np.abs(c - closed) <= 1e-5 * closed), (c, closed)


def _others_untouched(b, T, S, got, ref):
    (c, g), (c0, g0) = got, ref
    for o in range(len(T)):
        if o == b:
            continue
        assert D.same_bits(c[o:o + 1], c0[o:o + 1]), (o, c, c0)
        assert D.same_bits(g[D.utt_rows(T, S, o)], g0[D.utt_rows(T, S, o)]), o


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("b", [0, 2])
def test_masked_label_is_inf_and_others_untouched(V, b):
    acts, labels, T, S = clean(V)[:4]
    x, lab = D.mask_label(b)(acts, labels, T, S)
    c, g = run_cpu(x, lab, T, S)
    cr, gr = O.oracle_rnnt(x, lab, T, S)
    assert D.cost_class(cr)[b] == "+inf" and D.cost_class(c)[b] == "+inf", (c, cr)
    D.assert_costs_classed(c, cr)
    assert_grads(g, gr)  # the same non-finite places as the oracle, the rest within 1e-4
    _others_untouched(b, T, S, (c, g), run_cpu(acts, lab, T, S))


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("b", [0, 1])
def test_masked_blank_is_inf_and_others_untouched(V, b):
    acts, labels, T, S, ref = clean(V)[:5]
    x = D.mask_blank_rows(b)(acts, labels, T, S)
    c, g = run_cpu(x, labels, T, S)
    cr, gr = O.oracle_rnnt(x, labels, T, S)
    assert D.cost_class(cr)[b] == "+inf" and D.cost_class(c)[b] == "+inf", (c, cr)
    D.assert_costs_classed(c, cr)
    assert_grads(g, gr)
    _others_untouched(b, T, S, (c, g), ref)


def _poison_failures(acts, labels, T, S, ref, b, transforms):
    """Run every transform (each poisons utterance b) and return the failures as [(name, what)]."""
    bad = []
    rows = D.utt_rows(T, S, b)
    for tf in transforms:
        x = tf(acts, labels, T, S)
        cr, gr = O.oracle_rnnt(x, labels, T, S)
        # the condition the inputs were chosen for: the oracle calls this utterance NaN (and no other)
        assert D.cost_class(cr)[b] == "nan", (tf.__name__, cr)
        assert all(k == "finite" for o, k in enumerate(D.cost_class(cr)) if o != b), (tf.__name__, cr)
        c, g = run_cpu(x, labels, T, S)
        if D.cost_class(c)[b] != "nan":
            bad.append((tf.__name__, f"cost {c[b]} (class {D.cost_class(c)[b]}), oracle nan"))
            continue
        try:
            _others_untouched(b, T, S, (c, g), ref)
            D.assert_poisoned_grads(g[rows], gr[rows], D.grad_tol(x)[0])
        except AssertionError as e:
            bad.append((tf.__name__, str(e)[:200]))
    return bad


def test_poison_every_band_row_small():
    """B = 2, (T, S) = (9, 3) and (6, 2), V = 8: one NaN or one +inf in each of the 27 in-band rows of utterance 0
    in turn. Before the log-sum-exp tested both operands for -inf, the 16 cases at rows (0,0), (1,0), (1,1), (2,0),
    (2,2), (3,0), (4,0), (5,0) came back +inf: a band-edge cell has one out-of-band (-inf) predecessor, and
    fmax(NaN, -inf) == -inf took the "no path" exit."""
    acts, labels, T, S = D.base_problem(7, 2, (6, 9), 3, 8, force={0: (9, 3), 1: (6, 2)})
    ref = run_cpu(acts, labels, T, S)
    pos = D.band_positions(9, 3)
    assert len(pos) == 27
    tfs = [D.poison(0, t, s, v) for t, s, _ in pos for v in (D.NAN, D.INF)]
    bad = _poison_failures(acts, labels, T, S, ref, 0, tfs)
    assert not bad, f"{len(bad)} of {len(tfs)} cases:\n" + "\n".join(f"  {n}: {w}" for n, w in bad)


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("b", [0, 1, 2])
def test_poison_band_positions(V, b):
    """Every first / last row and up to 3 rows of each other kind, NaN and +inf, in each utterance in turn (S = 0:
    one column of rows; T = S: one diagonal, every row both edges), plus a whole row of -inf at an interior row."""
    acts, labels, T, S, ref = clean(V)[:5]
    pos = D.pick_positions(T[b], S[b])
    tfs = [D.poison(b, t, s, v) for t, s, _ in pos for v in (D.NAN, D.INF)]
    inner = [p for p in pos if p[2] == "interior"] or [p for p in pos if p[2] not in ("first", "last")]
    tfs.append(D.all_neg_inf_row(b, inner[0][0], inner[0][1]))
    bad = _poison_failures(acts, labels, T, S, ref, b, tfs)
    assert not bad, f"{len(bad)} of {len(tfs)} cases:\n" + "\n".join(f"  {n}: {w}" for n, w in bad)


def test_band_positions_kinds():
    pos = D.band_positions(9, 3)
    assert [p[:2] for p in pos if p[2] == "first"] == [(0, 0)] and [p[:2] for p in pos if p[2] == "last"] == [(8, 3)]
    assert len(pos) == 27 and {p[2] for p in pos} == {"first", "last", "lower_edge", "upper_edge", "interior"}
    assert all(max(0, t - 6) <= s <= min(t, 3) for t, s, _ in pos)
    assert len(D.band_positions(6, 6)) == 6 and len(D.band_positions(13, 0)) == 13
    assert list(D.cost_class([1.0, np.inf, -np.inf, np.nan])) == ["finite", "+inf", "-inf", "nan"]
    assert abs(D.closed_form_cost(4, 2, 3) - (4 * np.log(3) - np.log(6))) < 1e-12
