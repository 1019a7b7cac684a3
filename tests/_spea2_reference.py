"""Host references of SPEA2's fitness parts and truncation rule, shared by test_spea2_select.py and
test_spea2_select_gpu.py.  Everything here is numpy on float64 (or int64) evaluations of the float32
objectives; nothing imports the code under test."""
import functools

import numpy as np


def objectives(n, m, kind, seed=0):
    """``uniform``: rand in [0, 1]^m.  ``front``: |normal| + 1e-3 normalised to the unit sphere (every row
    non-dominated).  ``grid``: points of a coarse dyadic grid (multiples of 1/16 in [0, 4)), float32-exact."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, m)).astype(np.float32)
    if kind == "front":
        a = np.abs(rng.standard_normal((n, m))) + 1e-3
        return (a / np.sqrt((a * a).sum(1, keepdims=True))).astype(np.float32)
    assert kind == "grid"
    return (rng.integers(0, 64, (n, m)) / 16.0).astype(np.float32)


def d2_rows(o, rows):
    """float64 squared distances (len(rows), n) of the rows ``rows`` to every row, summed over the objectives in
    ascending order; a NaN is +inf."""
    d = np.zeros((len(rows), o.shape[0]))
    with np.errstate(invalid="ignore"):
        for k in range(o.shape[1]):
            diff = o[rows, k, None] - o[None, :, k]
            d += diff * diff
    d[np.isnan(d)] = np.inf
    return d


# ---------------------------------------------------------------- fitness
def fitness_parts(obj32, chunk=512):
    """``(S, nd, R, D)``: S and R exact in int64, nd bool, D in float64 (second smallest d2 over the other rows, with
    multiplicity).  Row chunks: no (n, n, m) tensor."""
    o32 = np.asarray(obj32, dtype=np.float32)
    o = o32.astype(np.float64)
    n = o.shape[0]
    S = np.zeros(n, dtype=np.int64)
    dominated_by = []  # per chunk: dom[i, j] for i in the chunk
    for i0 in range(0, n, chunk):
        a = o32[i0:i0 + chunk, None, :]
        with np.errstate(invalid="ignore"):
            dom = (a <= o32[None, :, :]).all(-1) & (a < o32[None, :, :]).any(-1)  # row i dominates row j
        S[i0:i0 + chunk] = dom.sum(1)
        dominated_by.append(dom)
    R = np.zeros(n, dtype=np.int64)
    nd = np.ones(n, dtype=bool)
    for c, dom in enumerate(dominated_by):
        R += (dom * S[c * chunk:c * chunk + dom.shape[0], None]).sum(0)
        nd &= ~dom.any(0)
    D = np.zeros(n)
    for i0 in range(0, n, chunk):
        rows = np.arange(i0, min(i0 + chunk, n))
        d = d2_rows(o, rows)
        d[np.arange(len(rows)), rows] = np.inf
        second = np.partition(d, 1, axis=1)[:, 1]
        D[rows] = 1.0 / (np.sqrt(second) + 2.0)
    return S, nd, R, D


# ---------------------------------------------------------------- truncation
def dense_truncation(obj32, mask, k):
    """The rule on a dense float64 (n, n) matrix of d2: k times the live masked row whose nearest live masked
    neighbour is closest leaves, the lowest index among equals (so the lower row of the exactly tied closest pair).
    Returns the removal order."""
    o = np.asarray(obj32, dtype=np.float32).astype(np.float64)
    n = o.shape[0]
    mask = np.asarray(mask, dtype=bool)
    d = d2_rows(o, np.arange(n))
    d[np.arange(n), np.arange(n)] = np.inf
    d[~mask, :] = np.inf
    d[:, ~mask] = np.inf
    live = mask.copy()
    order = []
    for _ in range(k):
        cand = np.flatnonzero(live)
        x = int(cand[np.argmin(d[cand].min(1))])
        order.append(x)
        live[x] = False
        d[x, :] = np.inf
        d[:, x] = np.inf
    return np.array(order, dtype=np.int64)


def _nearest(o, r, live):
    """(d2, index) of the nearest live row to r other than r in float64, the highest index among equals;
    (inf, −1) where no distance is finite."""
    cand = np.flatnonzero(live)
    cand = cand[cand != r]
    if cand.size == 0:
        return np.inf, -1
    d = d2_rows(o[np.concatenate([[r], cand])], np.array([0]))[0, 1:]
    best = d.min()
    if not np.isfinite(best):
        return np.inf, -1
    return float(best), int(cand[np.flatnonzero(d == best)[-1]])


def _all_nearest(o, live):
    """``_nearest`` of every live row, in row chunks."""
    n = o.shape[0]
    nn = np.full(n, np.inf)
    ni = np.full(n, -1, dtype=np.int64)
    rows = np.flatnonzero(live)
    for c0 in range(0, rows.size, 512):
        rr = rows[c0:c0 + 512]
        d = d2_rows(o, rr)
        d[:, ~live] = np.inf
        d[np.arange(rr.size), rr] = np.inf
        best = d.min(1)
        for a, r in enumerate(rr):
            if np.isfinite(best[a]):
                nn[r] = best[a]
                ni[r] = np.flatnonzero(d[a] == best[a])[-1]
    return nn, ni


def incremental_truncation(obj32, mask, k):
    """The same rule without the matrix: every live masked row keeps its nearest neighbour, and a removal rescans
    only the rows whose stored neighbour left.  Returns ``(order, gap, pairs, rescans)``: ``gap`` is the least, over
    the steps with at least three live rows, of (third smallest − smallest) / smallest nearest-neighbour d2 (inf where
    the smallest is 0 or the third is inf), and ``pairs`` whether at every such step exactly two rows were at the
    minimum."""
    o = np.asarray(obj32, dtype=np.float32).astype(np.float64)
    live = np.asarray(mask, dtype=bool).copy()
    nn, ni = _all_nearest(o, live)
    order, gap, pairs, rescans = [], np.inf, True, 0
    for _ in range(k):
        cand = np.flatnonzero(live)
        v = nn[cand]
        x = int(cand[np.argmin(v)])
        if cand.size >= 3:
            three = np.partition(v, 2)[:3]
            three.sort()
            pairs = pairs and three[0] == three[1] and three[2] > three[1]
            if three[0] > 0 and np.isfinite(three[2]):
                gap = min(gap, (three[2] - three[0]) / three[0])
        order.append(x)
        live[x] = False
        for r in np.flatnonzero(live & (ni == x)):
            nn[r], ni[r] = _nearest(o, r, live)
            rescans += 1
    return np.array(order, dtype=np.int64), float(gap), bool(pairs), rescans


def replay_slack(obj32, mask, order):
    """The certificate: replay a removal order in float64 and return the largest ratio, over the steps, of the
    removed row's nearest-neighbour d2 to the least nearest-neighbour d2 over the live masked rows (1 where both are
    0 or both +inf).  Incremental: a removal rescans only the rows that lost their neighbour."""
    o = np.asarray(obj32, dtype=np.float32).astype(np.float64)
    live = np.asarray(mask, dtype=bool).copy()
    nn, ni = _all_nearest(o, live)
    worst = 1.0
    for x in np.asarray(order).tolist():
        assert live[x], f"row {x} is removed twice or is outside the mask"
        least = nn[live].min()
        if nn[x] != least:
            worst = max(worst, float(nn[x] / least) if least > 0 else float("inf"))
        live[x] = False
        for r in np.flatnonzero(live & (ni == x)):
            nn[r], ni[r] = _nearest(o, r, live)
    return worst


@functools.lru_cache(maxsize=None)
def cached_objectives(n, m, kind, seed=0):
    a = objectives(n, m, kind, seed)
    a.setflags(write=False)
    return a
