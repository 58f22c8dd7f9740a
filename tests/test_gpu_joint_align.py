"""monotonic_rnnt_joint_align on the MI355X (mrnnt_joint_align): the best path through the lattice of the logits the
fused joint never stores, against the host reference of tests/_joint_lattice_cases.py (bf16(tanh(enc + pred)) @ W^T +
bias in fp64, packed) with np_viterbi and the oracle on those acts.

No path is compared with the reference's path on random cases: a bf16 rounding flip of one tanh (the kernel's fast
tanh against the host's) can move a near-tie. Checks 3 and 4 bound what such a flip may do to the cost.

Tolerance of the cost checks (3, 4, 6): TOL * max(1, |c|), starting from the joint's cost bound 1e-5
(tests/test_gpu_joint.py). MEASURED_MAX below is the largest deviation of the library from the host reference over
the cases of this file on an MI355X (every run prints its own figures: `-s`): 5.0e-8, the banded best-path cost of
"w129" at k = 2; checks 3 and 4 reach 4.3e-8 ("w65"), and the restricted loss of check 6 equals the align cost bit for
bit. No tanh rounding flip moved a cost on these cases, so the bound stays TOL = 1e-5 (the rule otherwise: 4 x the
measured maximum, never above 1e-3).

Sentinels (7). A vocabulary entry masked to -inf changes the log-softmax denominator of every row, so "the clean
call" of the -inf case carries the same masked bias: the entry is one no utterance uses, and the two calls differ
only in one label of one utterance, which the masked call sets to that entry.
"""
import ctypes

import numpy as np
import pytest
import torch

import _align_checks as A
import _joint_lattice_cases as C
import oracle

pytestmark = pytest.mark.gpu

MEASURED_MAX = 5.0e-8  # on an MI355X, see above
TOL = 1e-5

_free = {}


@pytest.fixture(scope="module")
def J():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import monotonic_rnnt_joint
    return monotonic_rnnt_joint


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(C.DEV)


def run_align(J, c, alignment=None, k=0, max_input_length=None, enc=None, bias=None, labels=None):
    args = list(C.dev_args(c, enc=enc, bias=bias))
    if labels is not None:
        args[4] = _dev(labels)
    out, costs = J.monotonic_rnnt_joint_align(*args, alignment=_dev(alignment), max_distance_from_alignment=k,
                                              max_input_length=max_input_length)
    assert out.dtype == torch.int32 and costs.dtype == torch.float32 and out.is_cuda
    assert not out.requires_grad and not costs.requires_grad
    return out.cpu().numpy(), costs.cpu().numpy()


def free(J, name):
    """The unrestricted alignment of a case, computed once."""
    if name not in _free:
        _free[name] = run_align(J, C.case(name))
    return _free[name]


def run_loss(J, c, alignment=None, k=0):
    return J.monotonic_rnnt_joint_loss(*C.dev_args(c), _dev(alignment), k).cpu().numpy()


def within(name, what, got, ref):
    dev = C.rel_dev(got, ref)
    print(f"MEASURED align {name} {what}: {dev:.3e}")
    assert dev <= TOL, (name, what, dev, got, ref)


@pytest.mark.parametrize("name", C.NAMES)
def test_valid_forced_paths_and_tail(J, name):
    """1, 2, 8: the labels in order; S_b = 0 all blank and T_b = S_b the labels themselves, exactly; blank from T_b."""
    c = C.case(name)
    al, costs = free(J, name)
    assert al.shape == (len(c.T), int(c.T.max())) and np.all(np.isfinite(costs))
    A.check_valid(al, c.labels, c.T, c.S, blank=c.blank)
    forced = 0
    for b, (Tb, Sb) in enumerate(zip(c.T, c.S)):
        if Sb == 0:
            assert np.all(al[b] == c.blank), b
        if Tb == Sb:
            assert np.array_equal(al[b, :Tb], c.labels[b, :Sb]), b
        forced += int(Sb == 0 or Tb == Sb)
    assert forced >= 1 or name == "ragged"


@pytest.mark.parametrize("name", C.NAMES)
def test_cost_is_the_paths_and_optimal(J, name):
    """3: the cost is the oracle's cost of the returned path on the reference acts (k = 0 leaves that path alone).
    4: it equals the reference's own best-path cost."""
    c = C.case(name)
    al, costs = free(J, name)
    own, _ = oracle.oracle_rnnt(c.acts, c.labels, c.T, c.S, blank=c.blank, alignment=al, max_shift=0, grads=False)
    within(name, "cost of the returned path", costs, own)
    best, _ = A.np_viterbi(c.acts, c.labels, c.T, c.S, blank=c.blank)
    within(name, "best-path cost", costs, best)


@pytest.mark.parametrize("name", ["w64", "w129", "ragged"])
@pytest.mark.parametrize("k", [0, 2])
def test_restriction(J, name, k):
    """5: realignment inside the band of an alignment (a random valid one): the path stays in the band and its cost is
    the banded reference's; k = 0 returns the given alignment."""
    c = C.case(name)
    rng = np.random.default_rng(5 + k)
    given = np.full((len(c.T), int(c.T.max())), c.blank, np.int32)
    for b, (Tb, Sb) in enumerate(zip(c.T, c.S)):
        given[b, np.sort(rng.choice(int(Tb), int(Sb), replace=False))] = c.labels[b, :Sb]
    al, costs = run_align(J, c, alignment=given, k=k)
    A.check_valid(al, c.labels, c.T, c.S, blank=c.blank)
    bands = [A.band_of(given[b], int(c.T[b]), k, blank=c.blank) for b in range(len(c.T))]
    for b, Tb in enumerate(c.T):
        after = np.cumsum(al[b, :Tb] != c.blank)  # label position after frame t
        assert np.all(after >= bands[b][0]) and np.all(after <= bands[b][1]), (k, b)
    ref, _ = A.np_viterbi(c.acts, c.labels, c.T, c.S, blank=c.blank, bands=bands)
    within(name, f"banded best-path cost k={k}", costs, ref)
    if k == 0:
        assert np.array_equal(al, given)


def test_c_level_in_place_and_null_costs(J):
    """5: p->alignment and alignment_out_dev the same buffer, costs_dev = NULL: the rows of the out-of-place call."""
    import _mrnnt_lib as L
    c = C.case("w65")
    al0, _ = free(J, "w65")
    want, _ = run_align(J, c, alignment=al0, k=2)
    buf = torch.from_numpy(al0.copy()).to(C.DEV)
    args = C.dev_args(c)
    prep = J._JointPrepared(*args, buf, 2)
    assert prep.alignment.data_ptr() == buf.data_ptr()
    n = ctypes.c_size_t(0)
    L.check(L.load().mrnnt_joint_workspace_size(ctypes.byref(prep.problem), ctypes.byref(n)), "size")
    ws = torch.empty(n.value, dtype=torch.uint8, device=C.DEV)
    vp = ctypes.c_void_p
    st = L.load().mrnnt_joint_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel(), vp(buf.data_ptr()),
                                    buf.size(1), None, prep.stream())
    assert st == L.RNNT_STATUS_SUCCESS, L.load().mrnnt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    st = L.load().mrnnt_joint_align(ctypes.byref(prep.problem), vp(ws.data_ptr()), ws.numel() - 1,
                                    vp(buf.data_ptr()), buf.size(1), None, prep.stream())
    assert st == L.RNNT_STATUS_INVALID_VALUE and b"workspace" in L.load().mrnnt_last_error()


@pytest.mark.parametrize("name", ["w1", "w65", "ragged"])
def test_round_trip_into_the_restricted_loss(J, name):
    """6: the joint loss restricted to the returned alignment with k = 0 is the path's cost; with k = 2 it lies
    between the unrestricted loss and the path's cost."""
    c = C.case(name)
    al, costs = free(J, name)
    within(name, "loss(alignment, k=0) vs align cost", run_loss(J, c, al, 0), costs)
    band, full = run_loss(J, c, al, 2).astype(np.float64), run_loss(J, c).astype(np.float64)
    slack = TOL * np.maximum(1.0, np.abs(costs))
    assert np.all(band <= costs + slack) and np.all(band >= full - slack), (full, band, costs)


def test_sentinels(J):
    """7: no finite path -> +inf and the row -1; a NaN in one utterance's enc -> NaN and the row -1; the other
    utterances bit for bit the clean call's (see the module docstring for the -inf case's clean call)."""
    c = C.case("w65")
    L = int(c.T.max()) + 2
    used = set(np.concatenate([c.labels[b, :Sb] for b, Sb in enumerate(c.S)]).tolist()) | {c.blank}
    v = next(x for x in range(c.w.shape[0]) if x not in used)
    bias = c.bias.clone()
    bias[v] = -np.inf
    al0, c0 = run_align(J, c, bias=bias, max_input_length=L)
    assert np.all(np.isfinite(c0))
    b = 3
    labels = c.labels.copy()
    labels[b, int(c.S[b]) // 2] = v  # utterance b now needs the masked entry
    al, costs = run_align(J, c, bias=bias, labels=labels, max_input_length=L)
    assert costs[b] == np.inf and np.all(al[b] == -1) and al.shape == (len(c.T), L)
    keep = [i for i in range(len(c.T)) if i != b]
    assert np.array_equal(al[keep], al0[keep]) and costs[keep].tobytes() == c0[keep].tobytes()

    al0, c0 = run_align(J, c, max_input_length=L)
    b = 0
    enc = c.enc.clone()
    enc[b, int(c.T[b]) // 2, 7] = float("nan")  # one frame of utterance b: every path crosses it
    al, costs = run_align(J, c, enc=enc, max_input_length=L)
    assert np.isnan(costs[b]) and np.all(al[b] == -1)
    keep = [i for i in range(len(c.T)) if i != b]
    assert np.array_equal(al[keep], al0[keep]) and costs[keep].tobytes() == c0[keep].tobytes()


def test_max_input_length(J):
    """8: L is honoured: the same rows and costs, blank in the added columns."""
    c = C.case("w64")
    al, costs = free(J, "w64")
    L = int(c.T.max()) + 5
    wide, wc = run_align(J, c, max_input_length=L)
    assert wide.shape == (len(c.T), L)
    assert np.array_equal(wide[:, :al.shape[1]], al) and np.all(wide[:, al.shape[1]:] == c.blank)
    assert wc.tobytes() == costs.tobytes()
    with pytest.raises(L_error()):
        run_align(J, c, max_input_length=int(c.T.max()) - 1)


def L_error():
    import _mrnnt_lib
    return _mrnnt_lib.MrnntError
