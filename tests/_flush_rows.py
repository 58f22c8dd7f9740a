"""Shared by tests/test_cpu_flush_rows.py and tests/test_gpu_flush_rows.py: the log-occupancy of every lattice row from
the oracle's fp64 state, and the count of rows in the window the flush-dead rule decides."""
import numpy as np


def log_occupancy(al, be, cr, T, S):
    """alpha(t-1, s) + beta(t, s) - ll of every row in the packed row order (alpha(-1, s) = [s == 0]; the oracle's cost
    is -ll); -inf outside the band, NaN where the state is."""
    out, r = [], 0
    for b, (Tb, Sb) in enumerate(zip(T, S)):
        W, n = int(Sb) + 1, int(Tb) * (int(Sb) + 1)
        a = al[r:r + n].reshape(Tb, W)
        prev = np.full_like(a, -np.inf)
        prev[0, 0] = 0.0
        prev[1:] = a[:-1]
        with np.errstate(invalid="ignore"):
            out.append((prev + be[r:r + n].reshape(Tb, W) + cr[b]).reshape(-1))
        r += n
    return np.concatenate(out)


def window_rows(al, be, cr, T, S, lo=-110.0, hi=-87.6):
    """Rows with lo <= log-occupancy < hi, per utterance. -87.6 lies a quarter nat inside the GPU rule's edge
    (-126.015625 ln 2 = -87.35)."""
    occ = log_occupancy(al, be, cr, T, S)
    with np.errstate(invalid="ignore"):
        m = (occ >= lo) & (occ < hi)
    n = np.asarray(T, np.int64) * (np.asarray(S, np.int64) + 1)
    return [int(x.sum()) for x in np.split(m, np.cumsum(n)[:-1])]
