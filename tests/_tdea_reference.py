"""Host reference of θ-DEA's θ-ranking, shared by test_tdea_select.py and test_tdea_select_gpu.py.  Everything here is
numpy float64 on the float32 inputs and follows the contract in the docstring of ``evoxmi/ops/tdea.py`` operation for
operation, on top of the host reference of ``cos_best`` (``_rvea_reference.py``); nothing here imports the code under
test (``UniformSampling`` only supplies the reference directions).  The cosines are formed in row chunks."""
import functools

import numpy as np

import _rvea_reference as rv

INF = float("inf")


def directions(N, m):
    """What ``UniformSampling(N, m)`` yields (its own count of rows); N = 1 is the single direction (1/m, …, 1/m)."""
    from evoxmi.operators.sampling import UniformSampling

    if N == 1:
        return np.full((1, m), 1.0 / m, dtype=np.float32)

    return UniformSampling(N, m)()[0].numpy().astype(np.float32)


def objectives(n, m, kind, seed=0):
    """``uniform``: rand in [0, 1]^m + 0.01.  ``front``: |normal| + 1e-3 normalised to the unit sphere, every row scaled
    by 1 + 0.2·rand.  No row is zero."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return (rng.random((n, m)) + 0.01).astype(np.float32)
    assert kind == "front"
    a = np.abs(rng.standard_normal((n, m))) + 1e-3
    a = a / np.sqrt((a * a).sum(1, keepdims=True))
    return (a * (1 + 0.2 * rng.random((n, 1)))).astype(np.float32)


def masks(n):
    """``name → mask``: all rows, every 7th row out, one row only, none."""
    every7 = np.ones(n, dtype=bool)
    every7[::7] = False
    one = np.zeros(n, dtype=bool)
    one[n // 2] = True
    return {"all": np.ones(n, dtype=bool), "every7": every7, "one": one, "none": np.zeros(n, dtype=bool)}


def theta_of(w):
    w = np.asarray(w, dtype=np.float32)
    return np.where((w > np.float32(1e-4)).sum(1) == 1, np.float32(1e6), np.float32(5.0)).astype(np.float32)


def cls_val(obj32, w32):
    """``cls (n) int64, val (n) float64``."""
    obj32, w32 = np.asarray(obj32, dtype=np.float32), np.asarray(w32, dtype=np.float32)
    best, arg, nrm, _ = rv.cos_best(obj32, w32)
    cls = np.clip(arg, 0, w32.shape[0] - 1)
    with np.errstate(all="ignore"):
        c = np.where(best < -1.0, -1.0, np.where(best > 1.0, 1.0, best))
        d1 = nrm * c
        q = 1.0 - c * c
        q = np.where(q < 0.0, 0.0, q)
        d2 = nrm * np.sqrt(q)
        val = d1 + theta_of(w32).astype(np.float64)[cls] * d2
    return cls, val


def rank(cls, val, mask):
    """``t_rank (n) float32``: 1 + the count of the masked rows of the same cls that order before by (val, position), a
    NaN after every number; +inf outside the mask."""
    mask = np.asarray(mask, dtype=bool)
    n = cls.shape[0]
    t = np.full(n, INF, dtype=np.float32)
    rows = np.flatnonzero(mask)
    key = np.where(np.isnan(val), INF, val)[rows]
    nan = np.isnan(val)[rows].astype(np.int64)
    order = np.lexsort((rows, nan, key, cls[rows]))  # cls, then val, NaN after +inf, then position
    c_o = cls[rows][order]
    pos = np.arange(rows.size) - np.searchsorted(c_o, c_o)
    t[rows[order]] = (pos + 1).astype(np.float32)
    return t


def theta_rank(obj32, w32, mask):
    cls, val = cls_val(obj32, w32)
    return rank(cls, val, mask), cls, val


def clusters_are_ranked(cls, t_rank, mask, nw):
    """Whether cls lies in [0, nw), the rows outside the mask are +inf and the masked ranks of every cluster are 1 … c."""
    cls, t_rank, mask = np.asarray(cls), np.asarray(t_rank), np.asarray(mask, dtype=bool)
    if not ((cls >= 0) & (cls < nw)).all() or not np.isinf(t_rank[~mask]).all():
        return False
    for j in np.unique(cls[mask]):
        got = np.sort(t_rank[mask & (cls == j)])
        if not np.array_equal(got, np.arange(1, got.size + 1, dtype=np.float32)):
            return False
    return True


@functools.lru_cache(maxsize=None)
def cached_case(N, m, kind, factor=2, extra=0):
    """``(obj, w, cls, val)`` with n = factor·nw + extra rows; shared between tests, never modified."""
    w = directions(N, m)
    n = factor * w.shape[0] + extra
    obj = objectives(n, m, kind, 100 * N + m)
    cls, val = cls_val(obj, w)
    for a in (obj, w, cls, val):
        a.setflags(write=False)
    return obj, w, cls, val
