"""Host reference of MOEA/D-M2M's association, shared by test_m2m_select.py and test_m2m_select_gpu.py.  Everything
here is numpy on the float32 objectives and follows the contract in ``csrc/kernels/m2m_select.hip``: per region a
brute-force dominance peel over its members, float32 crowding distance on the cut front in the stated operation order,
stable sorts.  Nothing here imports the code under test; ``cached_oracle`` (the CPU torch path, the kernel's oracle)
imports it when called."""
import functools

import numpy as np


# ---------------------------------------------------------------- inputs
def objectives(n, m, kind, seed):
    """``uniform``: rand in [0, 1]^m.  ``front``: |normal| + 1e-3 normalised to the unit sphere, so every row is
    non-dominated and crowding decides everything.  Seeded with ``torch.manual_seed``."""
    import torch

    torch.manual_seed(seed)
    if kind == "uniform":
        return torch.rand(n, m).numpy()
    assert kind == "front"
    a = torch.randn(n, m).abs() + 1e-3
    return (a / torch.linalg.norm(a, dim=1, keepdim=True)).numpy()


def case(n, m, K, S, kind, seed=None):
    """``(obj, region, rad)``: objectives of ``kind``, the region of every row (the direction of greatest cosine among
    K seeded random positive directions; one region when K = 1), and S seeded rows to pad with."""
    seed = n if seed is None else seed
    obj = objectives(n, m, kind, seed)
    rng = np.random.default_rng(seed + 1)
    w = np.abs(rng.standard_normal((K, m))) + 1e-3
    o = obj.astype(np.float64)
    cos = (o / np.linalg.norm(o, axis=1, keepdims=True)) @ (w / np.linalg.norm(w, axis=1, keepdims=True)).T
    region = np.argmax(cos, 1).astype(np.int64)
    rad = rng.integers(0, n, S).astype(np.int64)
    return obj, region, rad


# ---------------------------------------------------------------- the reference
def dominance(o):
    """``dom[i, j]``: row i dominates row j (≤ everywhere, < somewhere, on the float32 values; NaN compares false)."""
    c = o.shape[0]
    dom = np.zeros((c, c), dtype=bool)
    with np.errstate(invalid="ignore"):
        for i0 in range(0, c, 512):
            a = o[i0:i0 + 512]
            le, lt = np.ones((a.shape[0], c), dtype=bool), np.zeros((a.shape[0], c), dtype=bool)
            for k in range(o.shape[1]):
                le &= a[:, k, None] <= o[None, :, k]
                lt |= a[:, k, None] < o[None, :, k]
            dom[i0:i0 + 512] = le & lt
    return dom


def crowding(o):
    """float32 crowding distance of the rows of ``o`` among themselves: per objective a stable sort (NaN last), the
    extremes +inf, an interior row (next − prev) / (last − first); the terms added in objective order from 0."""
    F, m = o.shape
    dist = np.zeros(F, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(m):
            c = o[:, k].astype(np.float32)
            order = np.argsort(c, kind="stable")
            sc = c[order]
            d = np.empty(F, dtype=np.float32)
            if F > 2:
                d[order[1:-1]] = (sc[2:] - sc[:-2]) / np.float32(sc[-1] - sc[0])
            d[order[0]] = np.inf
            d[order[-1]] = np.inf
            dist = (dist + d).astype(np.float32)
    return dist


def select(obj32, region, rad, K, S):
    """``(part, counts, worst, info)`` of the contract; ``info`` lists per region ``(c, fronts peeled, cut front
    size, rows still needed from it)`` (zeros where the region is padded)."""
    obj = np.asarray(obj32, dtype=np.float32)
    region, rad = np.asarray(region), np.asarray(rad, dtype=np.int64)
    part = np.empty(K * S, dtype=np.int64)
    counts, worst, info = np.zeros(K, dtype=np.int32), np.full(K, -1, dtype=np.int32), []
    for k in range(K):
        rows = np.flatnonzero(region == k)
        c = counts[k] = rows.size
        if c < S:
            part[k * S:(k + 1) * S] = np.concatenate([rows, rad[c:S]])
            info.append((int(c), 0, 0, 0))
            continue
        o = obj[rows]
        dom = dominance(o)
        cnt = dom.sum(0).astype(np.int64)
        left = np.ones(c, dtype=bool)
        chosen, r = [], 0
        while True:
            front = np.flatnonzero(left & (cnt == 0))
            assert front.size > 0
            if len(chosen) + front.size >= S:
                break
            chosen.extend(rows[front].tolist())
            left[front] = False
            cnt -= dom[front].sum(0)
            r += 1
        need = S - len(chosen)
        cd = crowding(o[front])
        by_cd = np.argsort(-cd, kind="stable")  # NaN last, ties by slot = by row
        chosen.extend(rows[front[by_cd[:need]]].tolist())
        part[k * S:(k + 1) * S] = chosen
        worst[k] = r
        info.append((int(c), r + 1, int(front.size), int(need)))
    return part, counts, worst, info


def qualifies(info, S):
    """``(a region below S, a region above S, a region whose cut front is larger than what is still needed)``."""
    return (any(c < S for c, *_ in info), any(c > S for c, *_ in info), any(F > need > 0 for _, _, F, need in info))


# ---------------------------------------------------------------- cached cases and oracles
@functools.lru_cache(maxsize=None)
def cached_case(n, m, K, S, kind, seed=None):
    return case(n, m, K, S, kind, seed)


def oracle(obj, region, rad, K, S):
    """The kernel's oracle: ``ops.m2m.select`` on CPU tensors (the torch path), as numpy ``(part, counts, worst)``."""
    import torch

    from evoxmi.ops import m2m

    part, counts, worst = m2m.select(torch.from_numpy(np.ascontiguousarray(obj)), torch.from_numpy(np.ascontiguousarray(region)),
                                     torch.from_numpy(np.ascontiguousarray(rad)), K, S, return_info=True)
    return part.numpy(), counts.numpy(), worst.numpy()


@functools.lru_cache(maxsize=None)
def cached_oracle(n, m, K, S, kind, seed=None):
    obj, region, rad = cached_case(n, m, K, S, kind, seed)
    return oracle(obj, region, rad, K, S)
