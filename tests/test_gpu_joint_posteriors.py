"""monotonic_rnnt_joint_posteriors on the MI355X (mrnnt_joint_forward with beta + mrnnt_joint_posteriors): the arc
posteriors of the lattice of the logits the fused joint never stores, on the joint's [B, T_slots, S_slots] grid,
against the host reference of tests/_joint_lattice_cases.py (bf16(tanh(enc + pred)) @ W^T + bias in fp64, packed) with
np_posteriors on those acts, and against monotonic_rnnt_posteriors on the GPU on the same materialised acts. The grid
outputs are gathered into packed order for the helpers of tests/_posterior_checks.py.

Tolerances: those of _posterior_checks.compare (GRAD_TOL = 1e-4 absolute on blank / label / emit, GRAD_TOL * max(1, T_b)
on label_time, COST_TOL = 1e-4 relative on costs). MEASURED below holds the largest deviations from the host
reference over the cases of this file on an MI355X (every run prints its own figures: `-s`); against the materialised
acts path on the GPU they are 4.2e-7 / 6.0e-7 / 4.8e-7 / 2.8e-7 and 0 on the costs. All lie two orders of magnitude
inside the tolerances, which are used as they stand (the rule otherwise: 4 x the measured maximum).

Non-finite costs (6). A vocabulary entry masked to -inf changes the log-softmax denominator of every row, so "the
clean call" of the -inf case carries the same masked bias: the entry is one no utterance uses, and the two calls
differ only in one label of one utterance, which the masked call sets to that entry.
"""
import ctypes

import numpy as np
import pytest
import torch

import _align_checks as A
import _joint_lattice_cases as C
import _posterior_checks as P

pytestmark = pytest.mark.gpu

MEASURED = {"blank": 3.6e-7, "label": 6.1e-7, "emit": 5.8e-7, "label_time/T": 3.2e-7, "costs": 5.1e-8}

_free = {}


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(C.DEV)


def run_post(J, c, alignment=None, k=0, enc=None, bias=None, labels=None):
    """The library's result as numpy arrays, grid layout: Posteriors(blank, label [B, Tg, Sg], emit, label_time, costs)."""
    args = list(C.dev_args(c, enc=enc, bias=bias))
    if labels is not None:
        args[4] = _dev(labels)
    out = J.monotonic_rnnt_joint_posteriors(*args, alignment=_dev(alignment), max_distance_from_alignment=k)
    assert out._fields == P.Posteriors._fields
    assert all(x.dtype == torch.float32 and x.is_cuda and not x.requires_grad for x in out)
    B, Tg, Sg = len(c.T), c.enc.size(1), c.pred.size(1)
    assert out.blank.shape == (B, Tg, Sg) and out.label.shape == (B, Tg, Sg)
    assert out.emit.shape == (B, Tg) and out.label_time.shape == (B, c.labels.shape[1]) and out.costs.shape == (B,)
    return P.Posteriors(*(x.cpu().numpy() for x in out))


def packed(res, c):
    return P.Posteriors(C.gather_packed(res.blank, c.T, c.S), C.gather_packed(res.label, c.T, c.S), res.emit,
                        res.label_time, res.costs)


def free(J, name):
    """The unrestricted posteriors of a case, computed once."""
    if name not in _free:
        _free[name] = run_post(J, C.case(name))
    return _free[name]


def deviations(res, ref, T, S):
    """The figures _posterior_checks.compare bounds: max |d| of blank / label / emit, of label_time over max(1, T_b),
    and the relative cost deviation (finite references only)."""
    def dmax(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        fin = np.isfinite(y) & np.isfinite(x)
        return float(np.abs(x[fin] - y[fin]).max()) if fin.any() else 0.0
    d = {"blank": dmax(res.blank, ref.blank), "label": dmax(res.label, ref.label), "emit": 0.0, "label_time/T": 0.0}
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        d["emit"] = max(d["emit"], dmax(res.emit[b, :Tb], ref.emit[b]))
        d["label_time/T"] = max(d["label_time/T"], dmax(res.label_time[b, :Sb], ref.label_time[b]) / max(1, int(Tb)))
    d["costs"] = C.rel_dev(res.costs, ref.costs)
    return d


def report(name, what, res, ref, T, S):
    d = deviations(res, ref, T, S)
    print(f"MEASURED posteriors {name} {what}: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))


@pytest.mark.parametrize("name", C.NAMES)
def test_invariants_and_padding(J, name):
    """1: per-frame and per-label sums, sum_t emit = S_b, increasing label_time; 0 on the grid's padding rows and on
    emit's frames t >= T_b, -1 on label_time's s >= S_b."""
    c = C.case(name)
    res = free(J, name)
    assert np.all(np.isfinite(res.costs))
    P.check_invariants(packed(res, c), c.T, c.S)
    pad = C.padding_mask(res.blank.shape, c.T, c.S)
    assert pad.any() and np.all(res.blank[pad] == 0.0) and np.all(res.label[pad] == 0.0)
    for b, (Tb, Sb) in enumerate(zip(c.T, c.S)):
        assert np.all(res.emit[b, Tb:] == 0.0) and np.all(res.label_time[b, Sb:] == -1.0), b
        assert np.all(res.label[b, :Tb, Sb] == 0.0), b  # no label arc out of s = S_b


@pytest.mark.parametrize("name", C.NAMES)
def test_against_the_host_reference(J, name):
    """2a: np_posteriors on the reference acts."""
    c = C.case(name)
    res = packed(free(J, name), c)
    ref, reach = P.np_posteriors(c.acts, c.labels, c.T, c.S, blank=c.blank)
    report(name, "vs host reference", res, ref, c.T, c.S)
    P.compare(res, ref, c.T, c.S, name)
    assert np.all(res.blank[~reach] == 0.0) and np.all(res.label[~reach] == 0.0)  # unreachable rows: exactly 0


@pytest.mark.parametrize("name", ["w64", "w129", "ragged"])
def test_against_the_materialised_acts_path(J, name):
    """2b: monotonic_rnnt_posteriors on the GPU on the reference acts, materialised."""
    import monotonic_rnnt_op as op
    c = C.case(name)
    res = packed(free(J, name), c)
    m = op.monotonic_rnnt_posteriors(_dev(c.acts), _dev(c.labels), torch.from_numpy(c.T), torch.from_numpy(c.S),
                                     blank_label=c.blank)
    m = P.Posteriors(*(x.cpu().numpy() for x in m))
    ref = P.Posteriors(m.blank, m.label, [m.emit[b, :Tb] for b, Tb in enumerate(c.T)],
                       [m.label_time[b, :Sb] for b, Sb in enumerate(c.S)], m.costs.astype(np.float64))
    report(name, "vs materialised acts", res, ref, c.T, c.S)
    P.compare(res, ref, c.T, c.S, name)


@pytest.mark.parametrize("name", ["w65", "ragged"])
def test_costs_are_the_loss_and_calls_repeat_bitwise(J, name):
    """3: costs bit for bit monotonic_rnnt_joint_loss; two calls give the same bits in every output."""
    c = C.case(name)
    res = free(J, name)
    loss = J.monotonic_rnnt_joint_loss(*C.dev_args(c)).cpu().numpy()
    assert res.costs.tobytes() == loss.tobytes()
    again = run_post(J, c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res, again))


@pytest.mark.parametrize("name", ["w64", "w129"])
def test_restricted(J, name):
    """4: with the best path as the alignment and k = 1 the rows outside the band are exactly 0, the others the banded
    reference's."""
    c = C.case(name)
    al, _ = J.monotonic_rnnt_joint_align(*C.dev_args(c))
    aln = al.cpu().numpy()
    res = run_post(J, c, alignment=aln, k=1)
    bands = [A.band_of(aln[b], int(c.T[b]), 1, blank=c.blank) for b in range(len(c.T))]
    ref, reach = P.np_posteriors(c.acts, c.labels, c.T, c.S, blank=c.blank, bands=bands)
    assert np.all(np.isfinite(ref.costs)) and not reach.all()
    pk = packed(res, c)
    assert np.all(pk.blank[~reach] == 0.0) and np.all(pk.label[~reach] == 0.0)
    pad = C.padding_mask(res.blank.shape, c.T, c.S)
    assert np.all(res.blank[pad] == 0.0) and np.all(res.label[pad] == 0.0)
    report(name, "banded k=1 vs host reference", pk, ref, c.T, c.S)
    P.compare(pk, ref, c.T, c.S, name)
    P.check_invariants(pk, c.T, c.S)
    loss = J.monotonic_rnnt_joint_loss(*C.dev_args(c), al, 1).cpu().numpy()
    assert res.costs.tobytes() == loss.tobytes()


def test_c_level_null_outputs(J):
    """5: each output NULL in turn: it is skipped (its buffer keeps the fill) and the others keep their bits."""
    import _mrnnt_lib as L
    c = C.case("w65")
    full = free(J, "w65")
    prep = J._JointPrepared(*C.dev_args(c))
    costs, ws = prep.forward(with_beta=True)
    B, Tg, Sg, Sw = len(c.T), c.enc.size(1), c.pred.size(1), c.labels.shape[1]
    vp = ctypes.c_void_p
    shapes = [(B, Tg, Sg), (B, Tg, Sg), (B, Tg), (B, Sw)]
    for skip in range(5):  # 4: none skipped
        bufs = [torch.full(s, 7.0, dtype=torch.float32, device=C.DEV) for s in shapes]
        ptr = [None if i == skip else vp(x.data_ptr()) for i, x in enumerate(bufs)]
        st = L.load().mrnnt_joint_posteriors(ctypes.byref(prep.problem), vp(ws.data_ptr()), ptr[0], ptr[1], Tg, Sg,
                                             ptr[2], Tg, ptr[3], Sw, prep.stream())
        assert st == L.RNNT_STATUS_SUCCESS, L.load().mrnnt_last_error()
        torch.cuda.synchronize()
        for i, (x, want) in enumerate(zip(bufs, full[:4])):
            if i == skip:
                assert torch.all(x == 7.0), (skip, i)
            else:
                assert x.cpu().numpy().tobytes() == want.tobytes(), (skip, i)
    assert costs.cpu().numpy().tobytes() == full.costs.tobytes()


def _own_values_nan(res, clean, c, b):
    Tb, Sb = int(c.T[b]), int(c.S[b])
    assert np.all(np.isnan(res.blank[b, :Tb, :Sb + 1])) and np.all(np.isnan(res.label[b, :Tb, :Sb + 1]))
    assert np.all(np.isnan(res.emit[b, :Tb])) and np.all(res.emit[b, Tb:] == 0.0)
    assert np.all(np.isnan(res.label_time[b, :Sb])) and np.all(res.label_time[b, Sb:] == -1.0)
    pad = C.padding_mask(res.blank.shape, c.T, c.S)
    assert np.all(res.blank[pad] == 0.0) and np.all(res.label[pad] == 0.0)
    keep = [i for i in range(len(c.T)) if i != b]
    for x, y in zip(res, clean):
        assert x[keep].tobytes() == y[keep].tobytes()


def test_non_finite_costs(J):
    """6: an utterance without a path (cost +inf) and one with a NaN in its enc (cost NaN) have NaN in their own
    values only; the others keep the clean call's bits (see the module docstring for the -inf case's clean call)."""
    c = C.case("w65")
    used = set(np.concatenate([c.labels[b, :Sb] for b, Sb in enumerate(c.S)]).tolist()) | {c.blank}
    v = next(x for x in range(c.w.shape[0]) if x not in used)
    bias = c.bias.clone()
    bias[v] = -np.inf
    clean = run_post(J, c, bias=bias)
    assert np.all(np.isfinite(clean.costs))
    b = 3
    labels = c.labels.copy()
    labels[b, int(c.S[b]) // 2] = v  # utterance b now needs the masked entry
    res = run_post(J, c, bias=bias, labels=labels)
    assert res.costs[b] == np.inf
    _own_values_nan(res, clean, c, b)

    b = 0
    enc = c.enc.clone()
    enc[b, int(c.T[b]) // 2, 7] = float("nan")  # one frame of utterance b: every path crosses it
    res = run_post(J, c, enc=enc)
    assert np.isnan(res.costs[b])
    _own_values_nan(res, free(J, "w65"), c, b)
