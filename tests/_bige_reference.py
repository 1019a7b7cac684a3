"""Host reference of BiGE's bi-goal estimate, shared by test_bige_select.py and test_bige_select_gpu.py.  Everything
here is numpy float64 on the float32 inputs and follows the contract in the docstring of ``evoxmi/ops/bige.py``
operation for operation; nothing here imports the code under test.  Sums over the objectives loop explicitly
(``ndarray.sum`` adds pairwise from m = 8 on), and the pairs are formed in row chunks, so no (n, n, m) tensor is built.

``r`` is an input, as in the contract: the float32 word the device computes.  ``radius`` evaluates the same expression
with torch on the CPU; where a device's ``pow`` rounds differently the caller passes the device's own word."""
import functools

import numpy as np
import torch

INF = float("inf")


def objectives(n, m, kind, seed=0):
    """``uniform``: rand in [0, 1]^m.  ``front``: |normal| + 1e-3 normalised to the unit sphere."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, m)).astype(np.float32)
    assert kind == "front"
    a = np.abs(rng.standard_normal((n, m))) + 1e-3
    return (a / np.sqrt((a * a).sum(1, keepdims=True))).astype(np.float32)


def masks(n):
    """``name → mask``: all rows, every 7th row out, one row only, none."""
    every7 = np.ones(n, dtype=bool)
    every7[::7] = False
    one = np.zeros(n, dtype=bool)
    one[n // 2] = True
    return {"all": np.ones(n, dtype=bool), "every7": every7, "one": one, "none": np.zeros(n, dtype=bool)}


def radius(mask, m):
    """The float32 word ``1 / mask.sum().float() ** (1 / m)`` as torch evaluates it on the CPU."""
    return np.float32((1 / torch.tensor(int(np.asarray(mask).sum())).to(torch.float32) ** (1 / m)).item())


def estimate(fit32, mask, r, chunk=256):
    """``bi (n, 2) float32, pr (n) float64, cd (n) float64, thr_gap``: ``thr_gap`` is the smallest |d − r| / r over the
    pairs of distinct masked rows (inf without a pair): how far the fixture is from a ``d < r`` decision that a
    differently rounded distance would flip."""
    f32 = np.asarray(fit32, dtype=np.float32)
    mask = np.asarray(mask, dtype=bool)
    n, m = f32.shape
    r = np.float64(np.float32(r))
    pr = np.full(n, INF)
    cd = np.full(n, INF)
    rows = np.flatnonzero(mask)
    gap = INF
    if rows.size:
        fm = f32[rows]
        lo = fm.min(0).astype(np.float64)
        span = np.maximum(fm.max(0).astype(np.float64) - lo, 1e-6)
        x = (fm.astype(np.float64) - lo) / span
        p = x[:, 0].copy()
        for t in range(1, m):
            p = p + x[:, t]
        c = np.zeros(rows.size)
        for r0 in range(0, rows.size, chunk):
            r1 = min(r0 + chunk, rows.size)
            d2 = None
            for t in range(m):
                dl = x[r0:r1, t:t + 1] - x[None, :, t]
                d2 = dl * dl if d2 is None else d2 + dl * dl
            d = np.sqrt(d2)
            pi, pj = p[r0:r1, None], p[None, :]
            w = 1.0 + (pi >= pj) + (pi > pj)
            with np.errstate(all="ignore"):
                h = 0.5 * (w * (1.0 - d / r))
                sh = np.where(d < r, h * h, 0.0)
                off = np.ones_like(d, dtype=bool)
                off[np.arange(r1 - r0), np.arange(r0, r1)] = False
                sh = np.where(off, sh, 0.0)
                if rows.size > 1 and np.isfinite(r):
                    gap = min(gap, float((np.abs(d - r) / r)[off].min()))
            # pairwise: its own error is about log2(n) roundings.  A pair at distance 0 is exactly 1; those are counted
            # and added last, so equal rows, whose other terms are the same words at the same positions, get equal sums
            dup = off & (d2 == 0.0) & (sh == 1.0)
            c[r0:r1] = np.sqrt(np.where(dup, 0.0, sh).sum(1) + dup.sum(1))
        pr[rows] = p
        cd[rows] = c
    bi = np.stack([pr, cd], 1).astype(np.float32)
    return bi, pr, cd, gap


@functools.lru_cache(maxsize=None)
def cached_objectives(n, m, kind, seed=0):
    a = objectives(n, m, kind, seed)
    a.setflags(write=False)
    return a
