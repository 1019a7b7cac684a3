"""References for the exact hypervolume (``evoxmi.ops.hv``): the formulas of its contract in plain numpy float64,
vectorised per slice, and in ``fractions.Fraction`` on the float32 inputs (exact; meant for n ≤ 64).  Also the
fixtures the CPU and the GPU tests share, and the bounds of the contract.

The numpy reference sums the contributions as the difference ``x_i·y_i − A`` (the textbook form); the code under test
sums the complement.  Both are within the bound of the exact value."""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache

import numpy as np

U = 2.0**-53


def total_bound(n: int, m: int) -> float:
    """Relative error of a total against the exact value."""
    return ((3 if m == 4 else 2) * n + 16) * U


def contrib_bound(p32: np.ndarray) -> np.ndarray:
    """Absolute error of every row's contribution: (2n + 16)·u·vol(box i)."""
    p = np.maximum(p32.astype(np.float64), 0.0)
    return (2 * len(p) + 16) * U * np.prod(p, axis=1)


# ------------------------------------------------------------------ fixtures
def fixture(n: int, m: int, seed: int = 0) -> np.ndarray:
    """Random float32 rows in [0, 1); from n = 7 on they hold an exact duplicate (rows 1, 3), a row dominated by row 2
    and tied with it in z and w (row 4), a row tied with row 2 in x with another y (row 6), a zero coordinate (row 0)
    and a negative one (row 5)."""
    rng = np.random.default_rng(1000 * m + 10 * n + seed)
    p = rng.random((n, m)).astype(np.float32)
    if n >= 7:
        p[3] = p[1]
        p[4, :2] = p[2, :2] * np.float32(0.5)
        p[4, 2:] = p[2, 2:]
        p[6, 0] = p[2, 0]
        p[6, 1] = p[2, 1] * np.float32(0.75) + np.float32(0.01)
        p[0, 0] = 0.0
        p[5, 1] = -0.25
    return p


def equal_rows(n: int, m: int) -> np.ndarray:
    return np.tile(np.random.default_rng(5).random((1, m)).astype(np.float32), (n, 1))


def few_x_values(n: int, m: int) -> np.ndarray:
    """Every x is one of 4 values: the tie rule of the x order decides most of the walk."""
    rng = np.random.default_rng(77 + m)
    p = rng.random((n, m)).astype(np.float32)
    p[:, 0] = np.array([0.2, 0.4, 0.6, 0.8], np.float32)[rng.integers(0, 4, n)]
    return p


def front(n: int, m: int, seed: int = 0, scale: float = 1.0) -> np.ndarray:
    """Rows normalised to the unit sphere, times ``scale``: a DTLZ2-like front measured from its nadir."""
    t = np.random.default_rng(300 + seed).random((n, m)) + 1e-3
    return (t / np.linalg.norm(t, axis=1, keepdims=True) * scale).astype(np.float32)


def uniform(n: int, m: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(400 + seed).random((n, m)).astype(np.float32)


# ------------------------------------------------------------------ numpy float64
def _desc(v):
    """Positions in "v descending, ties by index"."""
    return np.argsort(-v, kind="stable")


def _setup(p32):
    p = np.maximum(np.asarray(p32).astype(np.float64), 0.0) + 0.0
    n, m = p.shape
    ox = _desc(p[:, 0])
    q = p[ox]
    ranks, heights = [], []
    for c in range(2, m):
        o = _desc(p[:, c])
        r = np.empty(n, np.int64)
        r[o] = np.arange(n)
        ranks.append(r[ox])
        s = np.append(p[o, c], 0.0)
        heights.append(s[:-1] - s[1:])
    return n, m, q[:, 0], q[:, 1], ox, ranks, heights


def _areas(x, y, keep, cx=np.inf, cy=np.inf):
    """A(keep, cx, cy) of every row of ``keep (S, n)``; a skipped row is walked with y' = 0, which adds 0 and leaves pm."""
    xx = np.minimum(x, cx)
    yy = np.where(keep, np.minimum(y, cy), 0.0)
    inc = np.maximum.accumulate(yy, axis=1)
    pm = np.concatenate([np.zeros((len(keep), 1)), inc[:, :-1]], axis=1)
    return np.sum(xx * np.maximum(0.0, yy - pm), axis=1)


def hv_numpy(p32) -> float:
    n, m, x, y, ox, ranks, heights = _setup(p32)
    if n == 0:
        return 0.0
    k = np.arange(n)
    if m == 2:
        return float(_areas(x, y, np.ones((1, n), bool))[0])
    if m == 3:
        blocks = [k[s : s + 256] for s in range(0, n, 256)]  # (256, n) arrays at a time
        return float(sum(np.sum(heights[0][b] * _areas(x, y, ranks[0][None, :] <= b[:, None])) for b in blocks))
    tot = 0.0
    for l in range(n):
        if heights[1][l] > 0:
            keep = (ranks[0][None, :] <= k[:, None]) & (ranks[1][None, :] <= l)
            tot += heights[1][l] * float(np.sum(heights[0] * _areas(x, y, keep)))
    return tot


def contributions_numpy(p32) -> np.ndarray:
    n, m, x, y, ox, ranks, heights = _setup(p32)
    out = np.zeros(n)
    k = np.arange(n)
    for i in range(n):
        if m == 2:
            keep, w = (k != i)[None, :], np.ones(1)
        else:
            keep = (ranks[0][None, :] <= k[:, None]) & (k != i)[None, :]
            w = np.where(k >= ranks[0][i], heights[0], 0.0)
        out[ox[i]] = np.sum(w * (x[i] * y[i] - _areas(x, y, keep, x[i], y[i])))
    return out


# ------------------------------------------------------------------ exact rationals
def _area_fraction(x, y, keep, cx=None, cy=None):
    a, pm = Fraction(0), Fraction(0)
    for j in range(len(x)):
        if not keep[j]:
            continue
        xx = x[j] if cx is None else min(x[j], cx)
        yy = y[j] if cy is None else min(y[j], cy)
        if yy > pm:
            a += xx * (yy - pm)
            pm = yy
    return a


def _setup_fraction(p32):
    n, m, x, y, ox, ranks, _ = _setup(p32)
    fr = lambda v: [Fraction(float(t)) for t in v]
    return n, m, fr(x), fr(y), ox, ranks, None  # the float64 heights are rounded: _heights_fraction forms them exactly


def _heights_fraction(p32, c):
    p = np.maximum(np.asarray(p32).astype(np.float64), 0.0)
    s = [Fraction(float(t)) for t in p[_desc(p[:, c]), c]] + [Fraction(0)]
    return [s[k] - s[k + 1] for k in range(len(p))]


def hv_fraction(p32) -> Fraction:
    n, m, x, y, ox, ranks, _ = _setup_fraction(p32)
    if n == 0:
        return Fraction(0)
    if m == 2:
        return _area_fraction(x, y, [True] * n)
    h = _heights_fraction(p32, 2)
    if m == 3:
        return sum((h[k] * _area_fraction(x, y, ranks[0] <= k) for k in range(n) if h[k] > 0), Fraction(0))
    g = _heights_fraction(p32, 3)
    tot = Fraction(0)
    for l in range(n):
        if g[l] > 0:
            for k in range(n):
                if h[k] > 0:
                    tot += g[l] * h[k] * _area_fraction(x, y, (ranks[0] <= k) & (ranks[1] <= l))
    return tot


def contributions_fraction(p32) -> list:
    n, m, x, y, ox, ranks, _ = _setup_fraction(p32)
    out = [Fraction(0)] * n
    pos = np.arange(n)
    h = _heights_fraction(p32, 2) if m == 3 else None
    for i in range(n):
        box = x[i] * y[i]
        if m == 2:
            c = box - _area_fraction(x, y, pos != i, x[i], y[i])
        else:
            c = Fraction(0)
            for k in range(int(ranks[0][i]), n):
                if h[k] > 0:
                    c += h[k] * (box - _area_fraction(x, y, (ranks[0] <= k) & (pos != i), x[i], y[i]))
        out[int(ox[i])] = c
    return out


# ------------------------------------------------------------------ shared, computed once
_KINDS = {"fixture": fixture, "equal": equal_rows, "few_x": few_x_values, "front": front, "uniform": uniform}


@lru_cache(maxsize=None)
def _points(kind, n, m):
    p = _KINDS[kind](n, m)
    p.setflags(write=False)
    return p


def points(kind: str, n: int, m: int) -> np.ndarray:
    """The read-only float32 rows of a named fixture."""
    return _points(kind, n, m)


@lru_cache(maxsize=None)
def total_exact(kind, n, m) -> Fraction:
    return hv_fraction(points(kind, n, m))


@lru_cache(maxsize=None)
def contrib_exact(kind, n, m) -> tuple:
    return tuple(contributions_fraction(points(kind, n, m)))


@lru_cache(maxsize=None)
def total_f64(kind, n, m) -> float:
    return hv_numpy(points(kind, n, m))


@lru_cache(maxsize=None)
def _contrib_f64(kind, n, m):
    c = contributions_numpy(points(kind, n, m))
    c.setflags(write=False)
    return c


def contrib_f64(kind, n, m) -> np.ndarray:
    return _contrib_f64(kind, n, m)


def rel_err(value: float, exact: Fraction) -> float:
    """|value − exact| / exact, itself exact before the last division; 0 when both are 0."""
    if exact == 0:
        return 0.0 if value == 0 else float("inf")
    return float(abs(Fraction(float(value)) - exact) / exact)


def abs_err(values, exact) -> np.ndarray:
    return np.array([float(abs(Fraction(float(v)) - e)) for v, e in zip(values, exact)])
