"""monotonic_rnnt_joint_sample on the MI355X (mrnnt_joint_forward with beta + mrnnt_joint_sample): alignments drawn
from the path posterior of the logits the fused joint never stores, on the cases of tests/_joint_lattice_cases.py.

Validity and path cost hold against the joint's own logits (the host reference bf16(tanh(enc + pred)) @ W^T + bias).
The samples equal monotonic_rnnt_sample's on those logits, materialised, with the same seed, apart from close samples
(tests/_sample_checks.py). Closeness is judged here with the joint's forward parity tolerance of
tests/test_gpu_joint.py, |dc| <= 1e-5 max(1, |c_b|), in place of GRAD_TOL: the sampler reads only the forward state,
x and y of its decision rule are log-probabilities of partial paths of utterance b, within that bound of the
reference's each, and p_label = 1 / (1 + exp(x - y)) has slope <= 1/4 in x - y, so |dp_label| <= 1e-5 max(1, |c_b|) / 2.
Cap: 10 % of a case's samples, met by the reference alone. Observed close samples of the reference at K = 64, seed 2:
w1 1 of 192 (0.5 %), w65 19 of 256 (7.4 %), ragged 3 of 256 (1.2 %); w64 (13 %) and w129 (21 %) exceed the cap -- their
T = S + 3 utterances have 66 / 131 near-deterministic frames under a tolerance of 3.5e-3 / 6.4e-3 -- and take the
validity and path-cost checks only.
"""
import ctypes

import numpy as np
import pytest
import torch

import _joint_lattice_cases as C
import _sample_checks as S

pytestmark = pytest.mark.gpu

K, SEED, CAP = 64, 2, 0.10
EXACT_CASES = ("w1", "w65", "ragged")


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(C.DEV)


def run_joint(J, c, num_samples=K, seed=SEED, enc=None, **kw):
    e, p, w, bias, lab, T, S_, blank = C.dev_args(c, enc=enc)
    out = J.monotonic_rnnt_joint_sample(e, p, w, bias, lab, T, S_, num_samples, seed, blank_label=blank, **kw)
    S.check_types(out, len(c.T), num_samples)
    assert all(x.is_cuda for x in out)
    return S.Samples(*(x.cpu().numpy() for x in out))


def _valid(res, c):
    for k in range(res.alignments.shape[1]):
        S.check_valid(res.alignments[:, k, :], c.labels, c.T, c.S, blank=c.blank)


@pytest.mark.parametrize("name", C.NAMES)
def test_validity_and_path_cost(J, name):
    """Every sample is a valid alignment whose path cost is the oracle's k = 0 cost of that alignment on the joint's
    own logits; costs is the joint loss."""
    import oracle
    c = C.case(name)
    res = run_joint(J, c, num_samples=5)
    assert res.alignments.shape == (len(c.T), 5, int(c.T.max()))
    _valid(res, c)
    for k in range(5):
        ref, _ = oracle.oracle_rnnt(c.acts, c.labels, c.T, c.S, blank=c.blank,
                                    alignment=np.ascontiguousarray(res.alignments[:, k, :]), max_shift=0, grads=False)
        S.assert_costs(res.path_costs[:, k], ref)
    full, _ = oracle.oracle_rnnt(c.acts, c.labels, c.T, c.S, blank=c.blank, grads=False)
    S.assert_costs(res.costs, full)


@pytest.mark.parametrize("name", EXACT_CASES)
def test_samples_equal_the_materialised_path(J, name):
    import monotonic_rnnt_op as op
    c = C.case(name)
    res = run_joint(J, c)
    ref = S.np_sample(c.acts, c.labels, c.T, c.S, K, SEED, blank=c.blank)
    tol = 1e-5 * np.maximum(1.0, np.abs(ref.costs))
    close = S.np_sample(c.acts, c.labels, c.T, c.S, K, SEED, tol=tol, blank=c.blank).close
    print(f"MEASURED joint sample {name}: close {int(close.sum())} of {close.size}")
    assert close.mean() <= CAP, (name, float(close.mean()))
    mat = op.monotonic_rnnt_sample(_dev(c.acts), _dev(c.labels), torch.from_numpy(c.T), torch.from_numpy(c.S), K, SEED,
                                   blank_label=c.blank)
    mat_al = mat.alignments.cpu().numpy()
    _valid(res, c)
    assert res.alignments.shape == mat_al.shape
    assert np.array_equal(res.alignments[~close], mat_al[~close]), name
    for b, Tb in enumerate(c.T):  # ... which is the yardstick's row
        assert np.array_equal(res.alignments[b, ~close[b], :Tb], ref.rows[b][~close[b]]), (name, b)
    S.assert_costs(res.path_costs[~close], mat.path_costs.cpu().numpy()[~close].astype(np.float64))


def test_determinism_indexing_and_width(J):
    c = C.case("ragged")
    r64 = run_joint(J, c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(r64, run_joint(J, c)))
    r8 = run_joint(J, c, num_samples=8, first_sample=8)
    assert np.array_equal(r8.alignments, r64.alignments[:, 8:16])
    assert r8.path_costs.tobytes() == r64.path_costs[:, 8:16].tobytes()
    L = int(c.T.max()) + 5
    wide = run_joint(J, c, max_input_length=L)
    assert wide.alignments.shape == (len(c.T), K, L)
    assert np.array_equal(wide.alignments[:, :, :L - 5], r64.alignments) and np.all(wide.alignments[:, :, L - 5:] == c.blank)
    assert not np.array_equal(run_joint(J, c, seed=SEED + 1).alignments, r64.alignments)


def test_restricting_alignment(J):
    """k = 0 returns the given alignment for every sample; k = 2 stays inside the band."""
    c = C.case("ragged")
    given = np.full((len(c.T), int(c.T.max())), c.blank, np.int32)
    rng = np.random.default_rng(5)
    for b, (Tb, Sb) in enumerate(zip(c.T, c.S)):
        given[b, np.sort(rng.choice(int(Tb), int(Sb), replace=False))] = c.labels[b, :Sb]
    res = run_joint(J, c, num_samples=9, alignment=_dev(given), max_distance_from_alignment=0)
    assert np.all(res.alignments == given[:, None, :])
    res = run_joint(J, c, num_samples=9, alignment=_dev(given), max_distance_from_alignment=2)
    _valid(res, c)
    for b, Tb in enumerate(c.T):
        lo, hi = S.band_of(given[b], int(Tb), 2, blank=c.blank)
        after = np.cumsum(res.alignments[b, :, :Tb] != c.blank, axis=1)
        assert np.all(after >= lo[None, :]) and np.all(after <= hi[None, :]), b


def test_nan_utterance_and_host_refusals(J):
    """A NaN in one utterance's enc rows: its rows -1 and path costs NaN, the others bit-identical. The host checks
    refuse num_samples = 0, a short stride and a NULL output before any device call."""
    import _mrnnt_lib as L
    c = C.case("ragged")
    clean = run_joint(J, c, num_samples=6)
    enc = c.enc.clone()
    enc[1, 0, 3] = float("nan")
    res = run_joint(J, c, num_samples=6, enc=enc)
    assert np.all(res.alignments[1] == -1) and np.all(np.isnan(res.path_costs[1])) and np.isnan(res.costs[1])
    for b in (0, 2, 3):
        assert np.array_equal(res.alignments[b], clean.alignments[b])
        assert res.path_costs[b].tobytes() == clean.path_costs[b].tobytes()
    with pytest.raises(RuntimeError, match="alignments row stride"):
        run_joint(J, c, max_input_length=int(c.T.max()) - 1)
    e, p, w, bias, lab, T, S_, blank = C.dev_args(c)
    prep = J._JointPrepared(e, p, w, bias, lab, T, S_, blank)
    _, ws = prep.forward(with_beta=True)
    Tm = int(c.T.max())
    out = torch.zeros((len(c.T), 4, Tm), dtype=torch.int32, device=C.DEV)
    vp, lib = ctypes.c_void_p, L.load()

    def call(w_, k_, o, stride):
        return lib.mrnnt_joint_sample(ctypes.byref(prep.problem), w_, k_, 1, 0, o, stride, None, prep.stream())
    assert call(vp(ws.data_ptr()), 0, vp(out.data_ptr()), Tm) == L.RNNT_STATUS_INVALID_VALUE
    assert b"num_samples" in lib.mrnnt_last_error()
    assert call(vp(ws.data_ptr()), 4, None, Tm) == L.RNNT_STATUS_INVALID_VALUE
    assert b"alignments is null" in lib.mrnnt_last_error()
    assert call(None, 4, vp(out.data_ptr()), Tm) == L.RNNT_STATUS_INVALID_VALUE
    assert b"workspace is null" in lib.mrnnt_last_error()
    assert call(vp(ws.data_ptr()), 4, vp(out.data_ptr()), Tm) == L.RNNT_STATUS_SUCCESS  # path_costs may be NULL
    torch.cuda.synchronize()
    _valid(S.Samples(out.cpu().numpy(), None, None), c)
