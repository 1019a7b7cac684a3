"""Host reference of the RVEA family's selection primitives, shared by test_rvea_select.py and test_rvea_select_gpu.py.
Everything here is numpy float64 on the float32 inputs and follows the contract in the docstring of ``evoxmi/ops/rvea.py``
operation for operation; nothing here imports the code under test (``UniformSampling`` only supplies reference vectors).
Norms and dot products loop over the objectives explicitly: ``ndarray.sum`` adds pairwise from m = 8 on.

Besides the results it reports three measures of a fixture, which say whether a float64 implementation that differs in
the last bits of ``acos`` must still give the same indices:

  a  the least gap between a row's best and second-best distinct cosine (association and regeneration);
  b  the least relative gap between the two smallest distinct ``apd`` among one vector's members;
  c  the gap between the distinct ``top`` values on either side of the truncation cut.

A fixture ``qualifies`` for the kernel comparison when a ≥ 1e-12, b ≥ 1e-9 and c ≥ 1e-12.  Exact ties are allowed: the
position decides them, in the contract as here."""
import functools

import numpy as np
import torch

INF = float("inf")


def _normalise(x):
    s = x[:, 0] * x[:, 0]
    for t in range(1, x.shape[1]):
        s = s + x[:, t] * x[:, t]
    nrm = np.sqrt(s)
    return x / nrm[:, None], nrm


def cos_best(A, B, shift=None, floor=None, clamp=False, self_zero=False, chunk=512):
    """``best (n) float64, arg (n) int64, norm (n) float64, gap``: gap is measure a of this call (inf when no row has
    two distinct cosines)."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    n, m = A.shape
    with np.errstate(all="ignore"):
        a = A.astype(np.float64)
        if shift is not None:
            a = a - np.asarray(shift, dtype=np.float32).astype(np.float64)
        if floor is not None:
            a = np.where(a < floor, np.float64(floor), a)
        ah, nrm = _normalise(a)
        bh, _ = _normalise(B.astype(np.float64))
        nan_row = np.isnan(A).any(1)
        best = np.empty(n)
        arg = np.empty(n, dtype=np.int64)
        gap = INF
        for r0 in range(0, n, chunk):
            r1 = min(r0 + chunk, n)
            c = ah[r0:r1, 0:1] * bh[None, :, 0]
            for t in range(1, m):
                c = c + ah[r0:r1, t:t + 1] * bh[None, :, t]
            bad = np.isnan(c)
            if clamp:
                c = np.where(c < 0.0, 0.0, np.where(c > 1.0, 1.0, c))
            c = np.where(bad, -INF, c)
            if self_zero:
                c[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0
            best[r0:r1] = c.max(1)
            arg[r0:r1] = c.argmax(1)  # the first position of the maximum
            second = np.where(c == best[r0:r1, None], -INF, c).max(1)
            ok = ~nan_row[r0:r1] & (second > -INF)
            if ok.any():
                gap = min(gap, float((best[r0:r1] - second)[ok].min()))
        best[nan_row] = 0.0 if self_zero else -INF
        arg[nan_row] = -1
    return best, arg, nrm, gap


def colmin(f):
    """The float32 column minimum ignoring NaN, +inf for a column without a number (what the torch side passes)."""
    f = np.asarray(f, dtype=np.float32)
    return np.where(np.isnan(f), np.float32(INF), f).min(0)


def apd_pick(arg, apd, nv):
    """``next_ind (nv) int64, empty (nv) bool, b``."""
    keyed = np.where(np.isfinite(apd), apd, INF)
    next_ind = np.zeros(nv, dtype=np.int64)
    empty = np.ones(nv, dtype=bool)
    b = INF
    for j in range(nv):
        rows = np.flatnonzero(arg == j)
        if rows.size == 0:
            continue
        empty[j] = False
        vals = keyed[rows]
        next_ind[j] = rows[np.argmin(vals)]  # the first position of the minimum
        d = np.unique(vals)
        if d.size > 1 and np.isfinite(d[1]):
            b = min(b, float((d[1] - d[0]) / d[0]))
    return next_ind, empty, b


def select(f, v, theta):
    """The APD selection: a dict with next_ind, empty, arg, apd, gamma and the measures a (association) and b."""
    f, v = np.asarray(f, dtype=np.float32), np.asarray(v, dtype=np.float32)
    m = f.shape[1]
    th = np.float64(np.float32(theta))
    with np.errstate(all="ignore"):
        gamma = np.arccos(cos_best(v, v, clamp=True, self_zero=True)[0])
        best, arg, nrm, a = cos_best(f, v, shift=colmin(f), floor=1e-32, clamp=True)
        angle = np.arccos(best)
        apd = (1.0 + ((np.float64(m) * th) * angle) / gamma[np.maximum(arg, 0)]) * nrm
    apd = np.where(arg >= 0, apd, INF)
    next_ind, empty, b = apd_pick(arg, apd, v.shape[0])
    return dict(next_ind=next_ind, empty=empty, arg=arg, apd=apd, gamma=gamma, a=a, b=b)


def truncation(obj):
    """``top, worst, c``: the most similar neighbour of every row, the n // 2 rows batch truncation removes (most crowded
    first, the lower position on equal values) and measure c."""
    top, _, _, _ = cos_best(obj, obj, self_zero=True)
    n = top.shape[0] // 2
    order = np.argsort(-top, kind="stable")
    inside, outside = top[order[n - 1]], top[order[n]] if order.size > n else -INF
    c = INF if inside == outside else float(abs(inside - outside))
    return top, order[:n], c


def qualifies(a, b, c=INF):
    return a >= 1e-12 and b >= 1e-9 and c >= 1e-12


# ---------------------------------------------------------------- fixtures
def vectors(nv, m, kind, seed):
    """``uniform``: what ``UniformSampling(nv, m)`` yields (its own count of rows); ``rand``: rand(nv, m), as RVEA*
    regenerates them."""
    if kind == "uniform":
        from evoxmi.operators.sampling import UniformSampling

        return UniformSampling(nv, m)()[0].numpy().astype(np.float32)
    return np.random.default_rng(seed + 77).random((nv, m)).astype(np.float32)


def objectives(n, m, nan_share, seed):
    """Rows on a scaled sphere shell, ``u/‖u‖ · (1 + 0.5·rand) · linspace(1, 3, m)``, ``round(nan_share·n)`` of them NaN."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, m)) + 1e-3
    f = u / np.linalg.norm(u, axis=1, keepdims=True) * (1 + 0.5 * rng.random((n, 1))) * np.linspace(1, 3, m)
    f = f.astype(np.float32)
    f[rng.permutation(n)[:int(round(nan_share * n))]] = np.nan
    return f


@functools.lru_cache(maxsize=None)
def cached_case(n, nv, m, nan_share, kind, seed):
    """``(f, v)`` of one fixture; shared between tests, never modified."""
    f, v = objectives(n, m, nan_share, seed), vectors(nv, m, kind, seed)
    f.setflags(write=False)
    v.setflags(write=False)
    return f, v


@functools.lru_cache(maxsize=None)
def cached_select(n, nv, m, nan_share, kind, seed, theta):
    f, v = cached_case(n, nv, m, nan_share, kind, seed)
    return select(f, v, theta)


def hand_cases():
    """``name → (f, v, theta)``: small inputs whose result can be read off the contract."""
    v2 = np.array([[1.0, 0.2], [0.2, 1.0]], dtype=np.float32)
    v3 = vectors(10, 3, "uniform", 0)
    nan = np.nan
    two = np.array([[2.0, 0.5], [0.4, 1.5]], dtype=np.float32)  # less the column minima: (1.6, 1e-32) and (1e-32, 1)
    return {
        "all rows NaN": (np.full((6, 3), nan, dtype=np.float32), v3, 0.3),
        "one valid row": (np.array([[nan, nan, nan], [0.5, 0.25, 1.0], [nan, nan, nan]], dtype=np.float32), v3, 0.3),
        "all rows equal": (np.full((5, 3), 0.75, dtype=np.float32), v3, 0.3),
        "a duplicated row": (np.array([[1.0, 2.0], [3.0, 0.5], [1.0, 2.0], [0.5, 3.0], [1.0, 2.0]], dtype=np.float32), v2, 0.5),
        "a row along a vector": (np.array([[0.0, 0.0], [2.0, 0.4], [0.3, 1.7]], dtype=np.float32), v2, 0.5),
        "one member each, theta 0": (two, v2, 0.0),
        "one member each, theta 1": (two, v2, 1.0),
    }


def to_torch(*arrays):
    return tuple(torch.from_numpy(np.array(a)) for a in arrays)  # copies: the cached fixtures are read-only
