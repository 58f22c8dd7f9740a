"""Cases and the host reference shared by tests/test_gpu_joint_align.py and tests/test_gpu_joint_posteriors.py.

The reference is the composition tests/test_gpu_joint.py states (its host_reference), kept as the logits themselves:
  h    = bf16(tanh(enc + pred))                 (fp32 tanh, round-to-nearest-even to bf16)
  acts = h @ weight.T + bias  (fp64, then fp32), packed rows r = off[b] + t (S_b + 1) + s
so that np_viterbi / np_posteriors / the oracle run on them. Each case is built once per process (lru_cache) and never
modified: tests that need a variant copy the tensor they change.

Shapes: max S + 1 in {1, 64, 65, 129} -- one wave, the 64 | 65 step to two waves and the 128 | 129 step to four in
launch_viterbi, and the 64 lanes of a posterior column wave -- with T just above, ragged batches of 3-5 utterances that
hold S = 0 and T = S, (H, V) in {(128, 64), (512, 100)} (V = 100: a partial vocabulary tile), blank = V - 1 once, and
one batch from test_gpu_joint.make_case.
"""
import collections
import functools

import numpy as np
import torch

from _align_checks import offsets
from test_gpu_joint import make_case

DEV = "cuda:0"

Case = collections.namedtuple("Case", ["enc", "pred", "w", "bias", "labels", "T", "S", "blank", "acts"])

#        name: (shapes [(T, S)], H, V, blank)
SHAPES = {
    "w1": ([(5, 0), (1, 0), (9, 0)], 128, 64, 0),
    "w64": ([(66, 63), (5, 0), (7, 7), (34, 31), (65, 62)], 512, 100, 99),
    "w65": ([(67, 64), (5, 0), (7, 7), (35, 32)], 512, 100, 0),
    "w129": ([(131, 128), (5, 0), (7, 7), (67, 64)], 128, 64, 0),
}
NAMES = tuple(SHAPES) + ("ragged",)


def reference_acts(enc, pred, w, bias, T, S):
    rows = []
    for b in range(len(T)):
        e = enc[b, : T[b]].float()
        p = pred[b, : S[b] + 1].float()
        h = torch.tanh(e[:, None, :] + p[None, :, :]).to(torch.bfloat16).double()  # [T, S+1, H]
        z = h @ w.double().T
        rows.append((z if bias is None else z + bias.double()).reshape(-1, w.shape[0]))
    return torch.cat(rows).float().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "ragged":
        enc, pred, w, bias, labels, T, S = make_case(4242, 4, (1, 24), 8, 128, 64)
        return Case(enc, pred, w, bias, labels, T, S, 0, reference_acts(enc, pred, w, bias, T, S))
    shapes, H, V, blank = SHAPES[name]
    rng = np.random.default_rng(1000 + len(name) + shapes[0][0])
    T = np.array([t for t, _ in shapes], np.int32)
    S = np.array([s for _, s in shapes], np.int32)
    Tm, Sm = int(T.max()), int(S.max())
    # one spare frame / label slot, as make_case: the grid of the posteriors is wider than the longest utterance
    enc = torch.from_numpy(rng.standard_normal((len(T), Tm + 1, H)).astype(np.float32)).to(torch.bfloat16)
    pred = torch.from_numpy(rng.standard_normal((len(T), Sm + 2, H)).astype(np.float32)).to(torch.bfloat16)
    w = torch.from_numpy((rng.standard_normal((V, H)) / np.sqrt(H) * 2.0).astype(np.float32)).to(torch.bfloat16)
    bias = torch.from_numpy(0.1 * rng.standard_normal(V).astype(np.float32))
    lo, hi = (1, V) if blank == 0 else (0, V - 1)  # no label equals the blank
    labels = rng.integers(lo, hi, (len(T), max(1, Sm))).astype(np.int32)
    return Case(enc, pred, w, bias, labels, T, S, blank, reference_acts(enc, pred, w, bias, T, S))


def dev_args(c, enc=None, bias=None):
    """The positional arguments of the three joint functions on the GPU (enc / bias replaceable by a variant)."""
    return (c.enc.to(DEV) if enc is None else enc.to(DEV), c.pred.to(DEV), c.w.to(DEV),
            (c.bias if bias is None else bias).to(DEV), torch.from_numpy(c.labels).to(DEV), torch.from_numpy(c.T),
            torch.from_numpy(c.S), c.blank)


def gather_packed(grid, T, S):
    """[B, grid_T, grid_S1] -> packed [N] (rows t < T_b, s <= S_b of every utterance, in lattice order)."""
    return np.concatenate([grid[b, :Tb, :Sb + 1].reshape(-1) for b, (Tb, Sb) in enumerate(zip(T, S))])


def padding_mask(shape, T, S):
    """True on the rows of the grid that belong to no lattice row."""
    m = np.ones(shape, bool)
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        m[b, :Tb, :Sb + 1] = False
    return m


def rel_dev(c, ref):
    """max |c - ref| / max(1, |ref|) over the finite references (the project's cost measure)."""
    c, ref = np.asarray(c, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(c), fin), (c, ref)
    return float((np.abs(c[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) if fin.any() else 0.0


__all__ = ["Case", "DEV", "NAMES", "case", "dev_args", "gather_packed", "offsets", "padding_mask", "reference_acts",
           "rel_dev"]
