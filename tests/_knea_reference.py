"""Host reference of KnEA's knee-point selection, shared by test_knea_select.py and test_knea_select_gpu.py.  Everything
here is numpy float64 on the float32 objectives and follows the contract in ``csrc/kernels/knea_select.hip`` (and the
docstring of ``evoxmi/ops/knea.py``) operation for operation; nothing here imports the code under test.

Besides the result, ``select`` returns the *qualifiers* of its input, which say how far the input is from a decision
that a few float64 ulps could turn:

* ``a``: the smallest relative distance of a float64 key from a float32 rounding boundary;
* ``b``: the smallest ``| |d| − R_j | / R_j`` over all box comparisons with ``d ≠ 0`` and ``R_j > 0``;
* ``c``: the largest condition number of a solved ``E``;
* ``gap``: the smallest relative distance between two distinct float32 keys of a front (what a float32 evaluation of
  the keys, the host path's, must not bridge to keep the scan order);
* ``dif``: the sign of ``dif`` at the cut;
* ``fallbacks``: the number of fallback planes.

A fixture qualifies for exact comparison with the kernel when a ≥ 1e-12, b ≥ 1e-9 and c ≤ 1e8: kernel and reference
perform the same float64 operations in the same order (the kernel is compiled without FMA contraction) and differ only
by the ulp of ``exp`` in r."""
import functools

import numpy as np


# ---------------------------------------------------------------- inputs
def objectives(n, m, kind, seed):
    """``uniform``: rand in [0, 1]^m.  ``front``: |normal| + 1e-3 normalised to the unit sphere.  Seeded with
    ``torch.manual_seed``."""
    import torch

    torch.manual_seed(seed)
    if kind == "uniform":
        return torch.rand(n, m).numpy()
    assert kind == "front"
    a = torch.randn(n, m).abs() + 1e-3
    return (a / torch.linalg.norm(a, dim=1, keepdim=True)).numpy()


def case(n, m, layers, kind, seed):
    """``(obj, rank)``: objectives of ``kind`` scaled by ``1 + 0.25·rank``, ``rank`` a sorted random layer index in
    which every one of the ``layers`` layers occurs (int64)."""
    rng = np.random.default_rng(seed + 1)
    rank = np.sort(np.concatenate([np.arange(layers), rng.integers(0, layers, n - layers)])).astype(np.int64)
    obj = objectives(n, m, kind, seed) * (1 + 0.25 * rank[:, None]).astype(np.float32)
    return np.ascontiguousarray(obj, dtype=np.float32), rank


@functools.lru_cache(maxsize=None)
def cached_case(n, m, layers, kind, seed):
    return case(n, m, layers, kind, seed)


# ---------------------------------------------------------------- the reference
def solve_plane(E):
    """``E·x = 1`` by Gaussian elimination with partial pivoting (the first row on equal magnitudes), in the kernel's
    operation order; None when a pivot is exactly 0 (or NaN) or a component is not finite."""
    m = E.shape[0]
    A = np.concatenate([E.astype(np.float64), np.ones((m, 1))], 1)
    with np.errstate(all="ignore"):
        for c in range(m):
            piv, best = c, abs(A[c, c])
            for r in range(c + 1, m):
                if abs(A[r, c]) > best:
                    piv, best = r, abs(A[r, c])
            if not best > 0.0:
                return None
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
            for r in range(c + 1, m):
                fct = A[r, c] / A[c, c]
                for k in range(c, m + 1):
                    A[r, k] = A[r, k] - fct * A[c, k]
        x = np.zeros(m)
        for c in range(m - 1, -1, -1):
            s = A[c, m]
            for k in range(c + 1, m):
                s = s - A[c, k] * x[k]
            x[c] = s / A[c, c]
    return x if np.isfinite(x).all() else None


def _boundary_distance(acc):
    """Relative distance of every float64 ``acc`` from the nearest point where its float32 rounding changes."""
    k = acc.astype(np.float32)
    lo = (k.astype(np.float64) + np.nextafter(k, np.float32(-np.inf)).astype(np.float64)) / 2
    hi = (k.astype(np.float64) + np.nextafter(k, np.float32(np.inf)).astype(np.float64)) / 2
    with np.errstate(all="ignore"):
        return np.minimum(np.abs(acc - lo), np.abs(acc - hi)) / np.abs(acc)


def select(obj32, rank, N, r, t, knee_rate, ties="ascending"):
    """``(idx, knee, r, t, qual)`` of the contract for ``obj32`` (n, m) float32 and the sorted ``rank`` (n,).  ``ties``:
    exact key ties by ascending position (the contract) or by ``descending`` position (to tell whether a fixture's
    result depends on the order of tied keys at all)."""
    obj32 = np.asarray(obj32, dtype=np.float32)
    rank = np.asarray(rank)
    obj = obj32.astype(np.float64)
    n, m = obj.shape
    assert 1 <= N < n and (np.diff(rank) >= 0).all()
    sgn = 1 if ties == "ascending" else -1
    last = int(rank[N])
    knee = np.zeros(n, dtype=bool)
    r, t = float(r), float(t)
    qual = {"a": np.inf, "b": np.inf, "c": 0.0, "gap": np.inf, "dif": 0, "fallbacks": 0, "knees": []}
    key = np.zeros(n, dtype=np.float32)
    for i in range(last + 1):
        pos = np.flatnonzero(rank == i)
        f = obj[pos]
        F = pos.size
        mx, mn = f.max(0), f.min(0)
        e = np.argmax(f, 0)  # the first maximum
        plane = solve_plane(f[e]) if len(set(e.tolist())) == m else None
        if plane is None:
            qual["fallbacks"] += 1
            plane = 1.0 / np.maximum(f[e, np.arange(m)], 1e-6)
        else:
            qual["c"] = max(qual["c"], float(np.linalg.cond(f[e])))
        acc = np.zeros(F)
        for j in range(m):
            acc = acc + f[:, j] * plane[j]
        qual["a"] = min(qual["a"], float(_boundary_distance(acc).min()))
        k32 = acc.astype(np.float32)
        k32 = np.where(k32 == 0, np.float32(0), k32)
        key[pos] = k32
        u = np.unique(k32).astype(np.float64)
        if u.size > 1:
            qual["gap"] = min(qual["gap"], float((np.diff(u) / np.abs(u[1:])).min()))
        order = np.lexsort((sgn * np.arange(F), k32))
        r = r * float(np.exp(-(1.0 - t / knee_rate) / m))
        R = (mx - mn) * r
        marked = np.ones(F, dtype=bool)
        for s in order:
            if not marked[s]:
                continue
            d = np.abs(f - f[s])
            inside = (d < R).all(1)
            inside[s] = False
            marked[inside] = False
            ok = (d != 0) & (R > 0)
            if ok.any():
                with np.errstate(all="ignore"):
                    qual["b"] = min(qual["b"], float((np.abs(d - R) / R)[ok].min()))
        knee[pos] = marked
        t = float(marked.sum()) / F
        qual["knees"].append((int(F), int(marked.sum())))
    selected = (rank < last) | knee
    dif = int(selected.sum()) - N
    qual["dif"] = int(np.sign(dif))
    pos = np.flatnonzero(rank == last)
    if dif > 0:
        cand = pos[knee[pos]]
        selected[cand[np.lexsort((sgn * cand, -key[cand].astype(np.float64)))][:dif]] = False
    elif dif < 0:
        cand = pos[~knee[pos]]
        selected[cand[np.lexsort((sgn * cand, key[cand]))][:-dif]] = True
    idx = np.flatnonzero(selected)
    assert idx.size == N
    return idx.astype(np.int64), knee, r, t, qual


def qualifies(qual, a=1e-12, b=1e-9, c=1e8):
    return qual["a"] >= a and qual["b"] >= b and qual["c"] <= c


@functools.lru_cache(maxsize=None)
def cached_select(n, m, layers, kind, seed, N, r, t, knee_rate=0.5):
    obj, rank = cached_case(n, m, layers, kind, seed)
    return select(obj, rank, N, r, t, knee_rate)


# ---------------------------------------------------------------- hand cases
def hand_cases():
    """``name → (obj, rank, N, r, t)``: small inputs whose result can be read off the contract (test_knea_select.py
    does that for the reference; test_knea_select_gpu.py runs the kernel on the same inputs)."""
    f32 = np.float32
    cases = {}
    # a front of one row: it is its own m extremes (fallback plane), R = 0, a knee
    cases["one_row_front"] = (np.array([[0.5, 0.5], [1, 3], [2, 2.5], [3, 1]], dtype=f32), np.array([0, 1, 1, 1]), 2, 0.3, 0.0)
    # all rows equal: R = 0, nothing is unmarked, every row a knee; the cut drops the lowest positions (equal keys)
    cases["all_equal"] = (np.full((6, 3), 0.25, dtype=f32), np.zeros(6, dtype=np.int64), 4, 1.0, 0.0)
    # rows 4 … 8 are exact copies: only the first is a knee (r stays 0.01: t = knee_rate)
    obj = objectives(12, 3, "front", 5).copy()
    obj[5:9] = obj[4]
    cases["copies"] = (obj, np.zeros(12, dtype=np.int64), 6, 0.01, 0.5)
    # a zero column: E is singular with an exact zero pivot (fallback plane), R_1 = 0, every row a knee
    obj = objectives(10, 3, "uniform", 6).copy()
    obj[:, 1] = 0
    cases["zero_column"] = (obj, np.zeros(10, dtype=np.int64), 5, 1.0, 0.0)
    # eight copies of one row and two others, r small: 3 knees (rows 0, 1, 9)
    obj = np.array([[1, 0.1]] + [[0.5, 0.5]] * 8 + [[0.1, 1]], dtype=f32)
    rank = np.zeros(10, dtype=np.int64)
    cases["dif_negative"] = (obj, rank, 6, 0.01, 0.5)  # rows 2, 3, 4 complete the cut (equal keys: by position)
    cases["dif_zero"] = (obj, rank, 3, 0.01, 0.5)
    cases["dif_positive"] = (obj, rank, 2, 0.01, 0.5)
    return cases
