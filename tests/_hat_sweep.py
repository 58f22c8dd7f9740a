"""Sweep of the factorised-blank (HAT) family on stored logits -- monotonic_rnnt_hat_loss,
monotonic_rnnt_path_loss(blank_factorized=True), monotonic_rnnt_expected_cost(blank_factorized=True) -- over the axes
their position-dependent code switches on: V and the element type (vector width, chunks, full / ragged rows, the scalar
kernels), the blank and label index (lane, chunk, ragged tail), S + 1 (single-wave / halo / per-step-barrier recursion,
gradient segments of 256 rows), B, alignment bands, layouts and lengths. Shared by tests/test_gpu_hat_sweep.py and
tests/test_cpu_hat_sweep.py (only the device differs): a directed table that pins every dispatch branch, and a seeded
random generator in the manner of tests/test_gpu_fuzz.py.

Yardstick (independent of the library, float64 end to end): _hat_weight_checks.expect_yardstick -- hat_transform in
float64, the log-domain DP with an optional band, torch.autograd's gradient -- and path_yardstick. The HAT loss is
expect_yardstick without costs (wb = we = None), g_e = 0 and g_c = the per-utterance scale. (Not the float32 oracle
on a': its per-arc rounding of a' adds up over hundreds of frames.) For bf16 / fp16 the yardstick runs on the upcast
values the kernel reads. Every yardstick cost and gradient is asserted finite: no case is skipped or filtered.

Tolerances are the project's own: costs _parity.assert_costs; loss gradients GRAD_TOL plus one rounding of the acts type
(2^-8 bf16, 2^-11 fp16) as test_gpu_fuzz.check_case; path gradients _path_checks.assert_path_grads; the expected value
and its gradients _expect_checks.assert_expected / grad_tol.

The directed table: (type, V) -> the log-softmax kernel mrnnt_softmax.hip's launch_io / launch_hat_vec / launch_hat_u
choose (VL = V / E vectors of 16 bytes; U = 4 for VL >= 192, 2 for VL >= 96, else 1; a chunk is 64 U vectors, C = 64 U E
elements). The gradient (mrnnt_grad.h launch_io / launch_vec) takes the scalar kernel on the same condition and the
staged kernel with the same U otherwise; "non-full" rows end in its ragged tail.

    f32 (E = 4)
       V   vectors  branch
       2, 3     --  scalar (V % 4 != 0); V = 2 is a softmax over one label
     257     --     scalar, 2 strides of 256 elements
    1030     --     scalar, 5 strides
     100     25     16-lane rows (VL <= 64), partial
     252     63     16-lane rows, partial
     260     65     U = 1, two chunks, non-full
     320     80     U = 1, two chunks, non-full
     400    100     U = 2, single chunk, non-full
     640    160     U = 2, two chunks, non-full
    1000    250     U = 4, single chunk, non-full
    1024    256     U = 4, single chunk, full (the branch the earlier HAT tests run; here for the blank positions)
    1028    257     U = 4, two chunks, one vector in the second
    3000    750     U = 4, three chunks, non-full
    4096   1024     U = 4, four full chunks
    bf16 / fp16 (E = 8)
     100, 1028  --  scalar (V % 8 != 0), 1 and 5 strides
     264     33     16-lane rows, partial
     520     65     U = 1, two chunks, non-full
    1000    125     U = 2, single chunk, non-full
    2000    250     U = 4, single chunk, non-full
    4104    513     U = 4, three chunks (256 + 256 + 1 vectors), non-full

Blank positions of a row, intersected with [0, V): 0, V - 1, V - 2, 3V/4 - 1, 64 E - 1 and 64 E (lane 63 -> lane 0),
C - 1, C and 2C (the chunk edges). V - 1 lies in the ragged last vector, and on the scalar kernels with V > 256 in the
last 256-stride. f32 runs every position; bf16 / fp16 run three: 0, V - 1 and one edge (C, else 64 E, else 3V/4 - 1).
Labels: labels[:, 0] = (blank + 1) % V (next to the blank), labels[:, 1] = the highest non-blank index (in the ragged
tail), the rest random and never the blank. Lattice: LATTICE -- the band widths min(S, T - S) + 1 = 6, 1, 1, 10 are not
multiples of the 2 or 4 rows a wave takes per pass.

The random generator, make_case(seed): V from the table's (a quarter of the cases V = 2 or 3, the only V at which the
size rule leaves room for S + 1 > 131, so these lean to the larger s_cap), B 1..4, s_cap in {8, 60, 130, 250, 460},
T in [1, s_cap + 40), S in [0, min(T, s_cap)] (half the cases put utterance 0 at S = s_cap, T >= s_cap: S + 1 = 461
is the per-step-barrier recursion, 131 and 251 the halo recursion), the blank uniform in [0, V), logits N(0, sigma)
with sigma in {0.5, 1, 3}, signed per-utterance scales (zero included), an alignment in 30 % of the cases with k in 0..5, f32 x6 : bf16 : f16, the padded layout 25 %,
device lengths 40 %. Size rule (a case takes a few seconds): rows V <= MAX_ELEMS = 4 M elements -- s_cap <= 60 for
V >= 1000 and <= 130 for 64 < V < 1000, then utterances are taken in order while they fit, the first one shrunk (S, then
T) if it alone does not. Labels never equal the blank and logits are finite, so every utterance has a finite cost.
"""
import os

import numpy as np
import torch

import _expect_checks as E
import _hat_weight_checks as C
import _path_checks as P
from _align_checks import offsets
from _parity import GRAD_TOL, assert_costs

N_CASES = int(os.environ.get("MRNNT_HAT_FUZZ_CASES", "96"))  # the suite: 96; long sweeps: set it higher
FIRST = int(os.environ.get("MRNNT_HAT_FUZZ_FIRST", "0"))
TORCH_DTYPE = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}
ROUNDING = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}  # one rounding of the acts type
LATTICE = [(12, 5), (5, 5), (9, 0), (70, 9)]
MAX_ELEMS = 4 << 20

F32_V = [2, 3, 257, 1030, 100, 252, 260, 320, 400, 640, 1000, 1024, 1028, 3000, 4096]
HALF_V = [100, 1028, 264, 520, 1000, 2000, 4104]


def elems_per_chunk(dtype, V):
    """(E, C): elements per 16-byte vector, and per chunk of the row's kernel (the launch ladder's U)."""
    e = 4 if dtype == "f32" else 8
    vl = V // e
    u = 4 if vl >= 192 else (2 if vl >= 96 else 1)
    return e, 64 * u * e


def blank_positions(dtype, V):
    e, c = elems_per_chunk(dtype, V)
    every = sorted({b for b in (0, V - 1, V - 2, (3 * V) // 4 - 1, 64 * e - 1, 64 * e, c - 1, c, 2 * c) if 0 <= b < V})
    if dtype == "f32":
        return every
    edge = next((b for b in (c, 64 * e) if b < V), (3 * V) // 4 - 1)
    return [0, edge, V - 1]


DIRECTED = ([("f32", V, b) for V in F32_V for b in blank_positions("f32", V)] +
            [(d, V, b) for d in ("bf16", "f16") for V in HALF_V for b in blank_positions(d, V)])


def directed_case(dtype, V, blank):
    acts, labels, T, S = C.problem(V, blank, shp=LATTICE)
    labels[:, 0] = (blank + 1) % V
    labels[:, 1] = V - 1 if blank != V - 1 else V - 2
    assert not np.any(labels == blank)
    return dict(V=V, T=T, S=S, blank=blank, labels=labels, acts=acts, scale=np.array([1.0, -0.5, 2.0, 0.25], np.float32),
                align=None, k=0, dtype=dtype, padded=False, dev_lengths=False, seed=V + blank)


S_CAPS = [8, 60, 130, 250, 460]
V_SMALL = [2, 3]
V_REST = sorted(set(F32_V + HALF_V) - set(V_SMALL))


def _fit(T, S, V):
    """The size rule: the leading utterances whose rows fit MAX_ELEMS / V, the first one shrunk if it must be."""
    budget = MAX_ELEMS // V
    t, s = int(T[0]), int(S[0])
    while s * (s + 1) > budget:
        s -= 1
    t = max(s, 1, min(t, budget // (s + 1)))
    T, S = T.copy(), S.copy()
    T[0], S[0] = t, s
    rows = np.cumsum(T.astype(np.int64) * (S + 1))
    n = int(np.sum(rows <= budget))
    assert n >= 1
    return T[:n], S[:n]


def make_case(seed, data=True):
    """The case of a seed; data=False: its description alone (no labels, logits or alignment)."""
    rng = np.random.default_rng(7000 + seed)
    V = int(rng.choice(V_SMALL)) if rng.random() < 0.25 else int(rng.choice(V_REST))
    B = int(rng.integers(1, 5))
    s_cap = int(rng.choice(S_CAPS, p=[0.1, 0.1, 0.2, 0.2, 0.4] if V <= 64 else None))
    if V >= 1000:
        s_cap = min(s_cap, 60)
    elif V > 64:
        s_cap = min(s_cap, 130)
    T = rng.integers(1, s_cap + 40, B).astype(np.int32)
    S = np.array([rng.integers(0, min(int(t), s_cap) + 1) for t in T], np.int32)
    if rng.random() < 0.5:  # utterance 0 at the cap: S + 1 = 9, 61, 131, 251, 461
        T[0] = rng.integers(s_cap, s_cap + 40)
        S[0] = s_cap
    T, S = _fit(T, S, V)
    B = len(T)
    blank = int(rng.integers(0, V))
    sigma = float(rng.choice([0.5, 1.0, 3.0]))
    scale = rng.choice([1.0, -0.5, 0.0, 2.0, 0.25], B).astype(np.float32)
    aligned = bool(rng.random() < 0.3)
    k = int(rng.integers(0, 6)) if aligned else 0
    dtype = str(rng.choice(["f32"] * 6 + ["bf16", "f16"]))
    padded = bool(rng.random() < 0.25)
    dev_lengths = bool(rng.random() < 0.4)
    c = dict(V=V, T=T, S=S, blank=blank, scale=scale, k=k, dtype=dtype, padded=padded, dev_lengths=dev_lengths,
             seed=seed, s_cap=s_cap, sigma=sigma, aligned=aligned)
    if not data:
        return c
    labels = rng.integers(0, V - 1, (B, max(1, int(S.max())))).astype(np.int32)
    labels += (labels >= blank).astype(np.int32)  # never the blank
    align = None
    if aligned:
        align = np.full((B, int(T.max())), blank, np.int32)
        for b in range(B):
            align[b, np.sort(rng.choice(int(T[b]), int(S[b]), replace=False))] = labels[b, : S[b]]
    acts = (rng.standard_normal((int(offsets(T, S)[-1]), V)) * sigma).astype(np.float32)
    assert acts.size <= MAX_ELEMS and np.all(np.isfinite(acts))
    c.update(labels=labels, align=align, acts=acts)
    return c


def describe(c):
    return (f"V={c['V']} blank={c['blank']} {c['dtype']} T={list(c['T'])} S={list(c['S'])} k={c['k']} "
            f"aligned={c['align'] is not None} padded={c['padded']} device_lengths={c['dev_lengths']}")


# ---- the comparisons -------------------------------------------------------------------------------------------------

def _inputs(dev, c):
    """(the values the kernel reads [N, V] f32, pad: packed -> the layout the call takes, call keywords). The host
    implementation takes float32 only: there a reduced-precision case runs on its upcast values."""
    T, S = c["T"], c["S"]
    dtype = TORCH_DTYPE[c["dtype"]]
    up = C.upcast(c["acts"], dtype)
    pad_T, pad_S1 = C.pad_shape(T, S)
    pad = (lambda x: P.pack_to_padded(x, T, S, pad_T, pad_S1, np.nan)) if c["padded"] else (lambda x: x)
    kw = dict(dtype=dtype if dev.gpu else None, device_lengths=bool(c["dev_lengths"] and dev.gpu))
    if c.get("unaligned"):
        kw["unaligned"] = True
    return up, pad, kw, (ROUNDING[c["dtype"]] if dev.gpu else 0.0)


def _unpad(c, g):
    """The packed rows of a gradient in the call's layout; its padding rows are exact zeros."""
    if not c["padded"]:
        return g
    assert np.all(g[C._padding(c["T"], c["S"], g.shape)] == 0.0)
    return P.padded_to_packed(g, c["T"], c["S"])


def _finite(*xs):
    for x in xs:
        assert np.all(np.isfinite(x)), "the yardstick must be finite: no case is skipped"


def check_loss(dev, c, cost_only_too=False):
    """monotonic_rnnt_hat_loss: costs and gradients of the scaled costs against the yardstick, padding rows exactly 0,
    and (cost_only_too) the cost-only forward bit-identical to the cost of the gradient call."""
    T, S, blank = c["T"], c["S"], c["blank"]
    up, pad, kw, rel = _inputs(dev, c)
    _, ref_c, ref_g = C.expect_yardstick(up, c["labels"], T, S, None, None, np.zeros(len(T)), c["scale"], blank,
                                         alignment=c["align"], k=c["k"])
    _finite(ref_c, ref_g)
    cost, g = dev.hat_loss(pad(up), c["labels"], T, S, c["scale"], blank, alignment=c["align"], k=c["k"], **kw)
    g = _unpad(c, g)
    err = np.abs(g - ref_g) - rel * np.abs(ref_g)
    print(f"loss {describe(c)}: max cost error {np.abs(cost - ref_c).max():.3e}, max gradient error {err.max():.3e}")
    assert_costs(cost, ref_c)
    assert g.shape == ref_g.shape and np.all(np.isfinite(g))
    assert err.max() <= GRAD_TOL, err.max()
    if cost_only_too:
        c2, _ = dev.hat_loss(pad(up), c["labels"], T, S, None, blank, alignment=c["align"], k=c["k"], **kw)
        assert c2.tobytes() == cost.tobytes()


def check_path(dev, c, K=3):
    """monotonic_rnnt_path_loss(blank_factorized=True) over K paths (labels first and labels last among them) with
    random signed weights; rows no path visits are exact zeros."""
    T, S, blank = c["T"], c["S"], c["blank"]
    up, pad, kw, eps = _inputs(dev, c)
    al = C.make_paths(c["labels"], T, S, K, blank, seed=c["seed"])
    w = np.random.default_rng(c["seed"] + 1).standard_normal((len(T), K)).astype(np.float32)
    ref_c, ref_g, visited, wsum = C.path_yardstick(up, c["labels"], T, S, al, w, blank)
    _finite(ref_c, ref_g)
    pc, g = dev.path(pad(up), c["labels"], T, S, al, w, blank, **kw)
    g = _unpad(c, g)
    print(f"path {describe(c)}: max cost error {np.abs(pc - ref_c).max():.3e}")
    assert_costs(pc, ref_c)
    P.assert_path_grads(g, ref_g, wsum, eps)
    assert np.all(g[~visited] == 0.0)


def check_expect(dev, c):
    """monotonic_rnnt_expected_cost(blank_factorized=True) with random costs and signed g_e / g_c, inside the case's
    alignment band when it has one."""
    T, S, blank = c["T"], c["S"], c["blank"]
    up, pad, kw, eps = _inputs(dev, c)
    rng = np.random.default_rng(c["seed"] + 2)
    wb, we = E.random_costs(rng, T, S)
    ge, gc = E.upstreams(rng, len(T))
    ref = C.expect_yardstick(up, c["labels"], T, S, wb, we, ge, gc, blank, alignment=c["align"], k=c["k"])
    _finite(*ref)
    pad1 = lambda x: pad(x[:, None])[..., 0]  # noqa: E731
    e, cost, g = dev.expect(pad(up), c["labels"], T, S, pad1(wb), pad1(we), ge, gc, blank, alignment=c["align"],
                            k=c["k"], **kw)
    print(f"expect {describe(c)}")
    C.assert_expect((e, cost, _unpad(c, g)), ref, T, S, wb, we, ge, gc, eps)


def check_directed(dev, dtype, V, blank):
    c = directed_case(dtype, V, blank)
    check_loss(dev, c, cost_only_too=True)
    check_path(dev, c, 3)
    check_expect(dev, c)


def check_random(dev, seed):
    c = make_case(seed)
    check_loss(dev, c, cost_only_too=(seed % 4 == 0))
    if seed % 3 == 0:
        check_path(dev, c, 3)
    if seed % 3 == 1:
        check_expect(dev, c)


def many_utterances_case(B=300, V=100, blank=98):
    """A batch wider than the setup scan's 64-lane chunks, with T = 1 / S = 0 utterances among them. (T < 12: the
    yardstick's autograd makes a zero tensor of the whole batch per utterance.)"""
    rng = np.random.default_rng(B)
    T = rng.integers(1, 12, B).astype(np.int32)
    T[:3] = 1
    S = np.array([rng.integers(0, t + 1) for t in T], np.int32)
    S[1] = 0
    labels = rng.integers(0, V - 1, (B, int(S.max()))).astype(np.int32)
    labels += (labels >= blank).astype(np.int32)
    acts = rng.standard_normal((int(offsets(T, S)[-1]), V)).astype(np.float32)
    return dict(V=V, T=T, S=S, blank=blank, labels=labels, acts=acts, align=None, k=0, dtype="f32", padded=False,
                scale=rng.choice([1.0, -0.5, 0.0, 2.0], B).astype(np.float32), dev_lengths=False, seed=B)


# ---- a label equal to blank is no arc --------------------------------------------------------------------------------

def _others_same(off, skip, got, clean):
    """Every per-utterance output but utterance `skip`'s: bit-identical."""
    for x, x0 in zip(got, clean):
        for b in range(len(off) - 1):
            if b == skip:
                continue
            if x.shape[0] == off[-1]:  # gradient rows
                assert x[off[b]:off[b + 1]].tobytes() == x0[off[b]:off[b + 1]].tobytes(), b
            else:
                assert x[b].tobytes() == x0[b].tobytes(), b


def check_label_equal_to_blank(dev, V, blank):
    """One label of utterance 0 (S = 5) set to the blank index (include/mrnnt.h, DESIGN.md 4j: no such arc): the loss
    and the expected cost give that utterance a cost of +inf and a NaN expected value (an utterance without a finite
    ll, as check_expect_non_finite), every path of it costs +inf, and the other utterances' costs and gradient rows
    are bit-identical to a run in which that label is another index."""
    acts, labels, T, S = C.problem(V, blank, shp=LATTICE[:3])
    off = offsets(T, S)
    bad = labels.copy()
    bad[0, 2] = blank
    scale = np.array([1.0, -0.5, 2.0], np.float32)
    clean = dev.hat_loss(acts, labels, T, S, scale, blank)
    cost, g = dev.hat_loss(acts, bad, T, S, scale, blank)
    assert np.all(np.isfinite(clean[0])) and cost[0] == np.inf, cost
    _others_same(off, 0, (cost, g), clean)
    rng = np.random.default_rng(V)
    wb, we = E.random_costs(rng, T, S)
    ge, gc = E.upstreams(rng, len(T))
    clean = dev.expect(acts, labels, T, S, wb, we, ge, gc, blank)
    e, cost, g = dev.expect(acts, bad, T, S, wb, we, ge, gc, blank)
    assert np.all(np.isfinite(clean[0])) and np.isnan(e[0]) and cost[0] == np.inf, (e, cost)
    assert np.all(np.isnan(g[off[0]:off[1]]))
    _others_same(off, 0, (e, cost, g), clean)
    K = 3
    w = rng.standard_normal((len(T), K)).astype(np.float32)
    for lab in (labels, bad):  # rows that still name the old label there, and rows that name the blank there
        al = C.make_paths(lab, T, S, K, blank)
        clean = dev.path(acts, labels, T, S, C.make_paths(labels, T, S, K, blank), w, blank)
        pc, g = dev.path(acts, bad, T, S, al, w, blank)
        assert np.all(np.isfinite(clean[0])) and np.all(pc[0] == np.inf), pc
        assert np.all(g[off[0]:off[1]] == 0.0)  # no valid path: nothing to differentiate
        _others_same(off, 0, (pc, g), clean)
