"""Host references of BCE-IBEA's PC selection and exploration, shared by test_bce_select.py and
test_bce_select_gpu.py.  Everything here is numpy on float64 evaluations of the float32 objectives and follows
the contract in ``csrc/kernels/bce_select.hip``; nothing imports the code under test.

The removal keeps, for every masked row, the list of the rows whose factor R is not 1 (its neighbours within the
niche radius): a product is the product of that list's live entries and a removal recomputes only its neighbours."""
import functools

import numpy as np

from _spea2_reference import cached_objectives, objectives  # noqa: F401  (the shared inputs)

U = 2.0**-24
SPAN_MIN = float(np.float32(1e-12))


def nd_mask(obj32):
    """The rows no row dominates (all ≤ and any <, on the float32 values; NaN compares false)."""
    o = np.asarray(obj32, dtype=np.float32)
    n = o.shape[0]
    nd = np.ones(n, dtype=bool)
    for i0 in range(0, n, 512):
        a = o[i0:i0 + 512]
        le, lt = np.ones((a.shape[0], n), dtype=bool), np.zeros((a.shape[0], n), dtype=bool)
        with np.errstate(invalid="ignore"):
            for k in range(o.shape[1]):
                le &= a[:, k, None] <= o[None, :, k]
                lt |= a[:, k, None] < o[None, :, k]
        nd &= ~(le & lt).any(0)  # row i dominates row j
    return nd


def spans(o, mask):
    with np.errstate(invalid="ignore"):
        return np.maximum(np.fmax.reduce(o[mask], 0) - np.fmin.reduce(o[mask], 0), SPAN_MIN)


def d2_rows(a, b, span):
    """float64 squared distances (len(a), len(b)) of the span-normalised differences, the difference first, summed
    over the objectives in ascending order; a NaN is +inf."""
    d = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore"):
        for k in range(a.shape[1]):
            diff = (a[:, k, None] - b[None, :, k]) / span[k]
            d += diff * diff
    d[np.isnan(d)] = np.inf
    return d


def niche(obj32, mask=None):
    """``(t, r, span)``: t_i = sqrt(third smallest d2) over the other masked rows (+inf with fewer than three, 0
    outside the mask) and r = Σ t_i / #mask."""
    o = np.asarray(obj32, dtype=np.float32).astype(np.float64)
    n = o.shape[0]
    mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    rows = np.flatnonzero(mask)
    span = spans(o, mask)
    t = np.zeros(n)
    for c0 in range(0, rows.size, 512):
        rr = rows[c0:c0 + 512]
        d = d2_rows(o[rr], o[rows], span)
        d[np.arange(rr.size), c0 + np.arange(rr.size)] = np.inf
        if rows.size >= 4:
            t[rr] = np.sqrt(np.partition(d, 2, axis=1)[:, 2])
        else:
            t[rr] = np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        r = t[rows].sum() / rows.size
    return t, float(r), span


class _Products:
    """P_j of the live masked rows from neighbour lists, in float64."""

    def __init__(self, obj32, mask):
        o = np.asarray(obj32, dtype=np.float32).astype(np.float64)
        self.mask = np.asarray(mask, dtype=bool)
        self.live = self.mask.copy()
        _, self.r, span = niche(obj32, self.mask)
        rows = np.flatnonzero(self.mask)
        n = o.shape[0]
        self.nb = [np.zeros(0, dtype=np.int64)] * n  # the rows whose factor is not 1
        self.fac = [np.zeros(0)] * n
        for c0 in range(0, rows.size, 512):
            rr = rows[c0:c0 + 512]
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.sqrt(d2_rows(o[rr], o[rows], span)) / self.r
            R = np.where(q > 1, 1.0, q)  # a NaN quotient stays NaN
            R[np.arange(rr.size), c0 + np.arange(rr.size)] = 1.0
            for a, j in enumerate(rr):
                hit = np.flatnonzero(~(R[a] == 1.0))
                self.nb[j] = rows[hit]
                self.fac[j] = R[a, hit]
        self.P = np.ones(n)
        for j in rows:
            self.P[j] = self.product(j)
        self.factors = max((len(self.nb[j]) for j in rows), default=0)

    def live_neighbours(self, j):
        return self.nb[j][self.live[self.nb[j]]]

    def product(self, j):
        return float(np.prod(self.fac[j][self.live[self.nb[j]]]))

    def remove(self, x):
        self.live[x] = False
        hit = self.live_neighbours(x)
        for j in hit:
            self.P[j] = self.product(j)
        return len(hit)


def removal(obj32, mask, k):
    """The contract's removal in float64: k times the live masked row of least P (a NaN first), the lowest index
    among equals, leaves.  Returns ``(order, gap, ties_ok, ties, factors, rescans)``: ``gap`` the least, over the
    steps, relative gap (P₂ − P₁) / P₂ of the two smallest live products that are not exactly tied, ``ties`` the
    number of steps where they are, ``ties_ok`` whether every such tie is a pair of rows that are each other's only
    live neighbour within r, ``factors`` the most factors below 1 of any product."""
    pr = _Products(obj32, mask)
    order, gap, ties_ok, ties, rescans = [], np.inf, True, 0, 0
    for _ in range(k):
        cand = np.flatnonzero(pr.live)
        v = pr.P[cand]
        nan = np.isnan(v)
        if nan.any():
            x = int(cand[np.flatnonzero(nan)[0]])
        else:
            x = int(cand[np.argmin(v)])
            if cand.size >= 2:
                two = np.argpartition(v, 1)[:2]
                p1, p2 = sorted(v[two])
                if p1 == p2:
                    ties += 1
                    a, b = (int(c) for c in cand[np.flatnonzero(v == p1)[:2]])
                    la, lb = pr.live_neighbours(a), pr.live_neighbours(b)
                    ties_ok = ties_ok and la.tolist() == [b] and lb.tolist() == [a] and int((v == p1).sum()) == 2
                else:
                    gap = min(gap, (p2 - p1) / p2)
        order.append(x)
        rescans += pr.remove(x)
    return np.array(order, dtype=np.int64), float(gap), bool(ties_ok), ties, pr.factors, rescans


def replay_ratio(obj32, mask, order):
    """The certificate: replay a removal order in float64 and return ``(worst, factors)``, the largest ratio over the
    steps of the removed row's P to the least P over the live masked rows (1 where both are 0; inf where a live row
    has a NaN product and the removed one has not)."""
    pr = _Products(obj32, mask)
    worst = 1.0
    for x in np.asarray(order).tolist():
        assert pr.live[x], f"row {x} is removed twice or is outside the mask"
        v = pr.P[pr.live]
        if np.isnan(v).any():
            if not np.isnan(pr.P[x]):
                worst = np.inf
        else:
            least = v.min()
            if pr.P[x] != least:
                worst = max(worst, pr.P[x] / least if least > 0 else np.inf)
        pr.remove(x)
    return float(worst), pr.factors


def product_bound(factors, m, n):
    """The float32 relative error bound of a product of ``factors`` factors below 1, first order in u = 2⁻²⁴ (see the
    docstring of test_bce_select_gpu.py): every factor within (m + 10 + depth)·u, depth = ⌈n / 256⌉ + 9 the additions
    on the longest path of the sum of r, and factors − 1 multiplications."""
    depth = -(-n // 256) + 9
    return max(factors * (m + 11 + depth) - 1, 0) * U


def select_indices(n, mask, order, n_keep):
    """The (n_keep,) indices the contract returns for a removal order: the kept masked rows ascending, padded with
    the first masked row."""
    keep = np.asarray(mask, dtype=bool).copy()
    keep[np.asarray(order, dtype=np.int64)] = False
    idx = np.flatnonzero(keep)[:n_keep]
    first = np.flatnonzero(mask)[0]
    return np.concatenate([idx, np.full(n_keep - idx.size, first, dtype=np.int64)])


def exploration(pc32, npc32, n_nd, rel=1e-4):
    """``(s, near)``: s_i whether at most one NPC row lies within n_nd / N · r0 of PC row i (r0 the mean niche radius
    over all PC rows, PC's spans), and ``near_i`` whether some NPC distance is within ``rel`` relative of that radius."""
    pc = np.asarray(pc32, dtype=np.float32).astype(np.float64)
    npc = np.asarray(npc32, dtype=np.float32).astype(np.float64)
    N = pc.shape[0]
    _, r0, span = niche(pc32)
    rr = n_nd / N * r0
    d = np.sqrt(d2_rows(pc, npc, span))
    return (d <= rr).sum(1) <= 1, (np.abs(d - rr) <= rel * rr).any(1)


@functools.lru_cache(maxsize=None)
def cached_removal(n, m, kind, seed, all_rows):
    obj = cached_objectives(n, m, kind, seed)
    mask = np.ones(n, dtype=bool) if all_rows else nd_mask(obj)
    return obj, mask, removal(obj, mask, int(mask.sum()) - int(mask.sum()) // 2)
