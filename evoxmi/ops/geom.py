"""k-nearest rows (K17) and Monte-Carlo hypervolume dominance counts (K18).

Device path: ``csrc/kernels/mo_geom.hip`` (fused distance + register top-T, no N×M
matrix; tiled sample×point dominance tests with a deterministic per-point reduction).
The CPU branches below are the numerics oracles the GPU tests compare against.
"""
from __future__ import annotations

import torch

from . import _ext

KNN_MAX_T, KNN_MAX_M, HV_MAX_M = 32, 64, 16
HYPE_MAX_N, HYPE_MAX_SAMPLES = 2048, 1 << 20  # hype_fitness.hip: rows and samples per run


def _sqdist_rows(X, Y, chunk=512):
    out = []
    for s in range(0, X.shape[0], chunk):
        blk = X[s : s + chunk]
        out.append(((blk[:, None, :] - Y[None, :, :]) ** 2).sum(-1))
    return torch.cat(out, 0) if out else X.new_zeros((0, Y.shape[0]))


def knn(X: torch.Tensor, Y: torch.Tensor, T: int):
    """(distances (N, T), indices (N, T) int64) of the T nearest rows of ``Y`` for every
    row of ``X``, ascending by (squared euclidean distance, index) — a stable argsort of
    the direct-form distance row, as the reference's ``argsort(pairwise_euclidean_dist)``.
    NaN distances rank first (reported as NaN); inf distances are ordinary candidates."""
    X = X.to(torch.float32).contiguous()
    Y = Y.to(torch.float32).contiguous()
    T = int(T)
    if X.is_cuda and T <= KNN_MAX_T and X.shape[1] <= KNN_MAX_M:
        d, i = _ext.ops().knn(X, Y, T)
        return d, i.long()
    out_d, out_i = [], []
    for s in range(0, X.shape[0], 512):
        d2 = _sqdist_rows(X[s : s + 512], Y, 512)
        # a NaN distance ranks first so the nearest distance propagates it (as
        # torch.cdist(..).min() and the reference's min do); the kernel uses the same order
        key = torch.where(torch.isnan(d2), torch.full_like(d2, float("-inf")), d2)
        i = torch.argsort(key, dim=1, stable=True)[:, :T]
        out_d.append(torch.sqrt(torch.gather(d2, 1, i)))
        out_i.append(i)
    return torch.cat(out_d), torch.cat(out_i)


def min_dist(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """Distance from every row of ``X`` to its nearest row of ``Y`` (IGD / GD)."""
    return knn(X, Y, 1)[0][:, 0]


def hv_count(samples: torch.Tensor, points: torch.Tensor, strict: bool) -> torch.Tensor:
    """For each sample, the number of points dominating it: ``sample < point`` in every
    objective (strict, the HV metric on |objs − ref|) or ``point ≤ sample`` (HypE)."""
    samples = samples.to(torch.float32).contiguous()
    points = points.to(torch.float32).contiguous()
    if samples.is_cuda and samples.shape[1] <= HV_MAX_M:
        return _ext.ops().hv_count(samples, points, int(bool(strict))).long()
    out = []
    step = max(1, (1 << 22) // max(points.shape[0], 1))
    for s0 in range(0, samples.shape[0], step):
        s = samples[s0 : s0 + step]
        dom = (s[:, None, :] < points[None, :, :]) if strict else (points[None, :, :] <= s[:, None, :])
        out.append(dom.all(-1).sum(1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64, device=samples.device)


def hv_contrib(samples: torch.Tensor, points: torch.Tensor, count: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """HypE: f_i = Σ_s [point_i ≤ sample_s] · α[count_s − 1]."""
    samples = samples.to(torch.float32).contiguous()
    points = points.to(torch.float32).contiguous()
    alpha = alpha.to(torch.float32).contiguous()
    if samples.is_cuda and samples.shape[1] <= HV_MAX_M:
        return _ext.ops().hv_contrib(samples, points, count.to(torch.int32).contiguous(), alpha)
    f = torch.zeros(points.shape[0], device=points.device)
    w = torch.where(count > 0, alpha[(count - 1).clamp(min=0)], torch.zeros((), device=alpha.device))
    for s0 in range(0, samples.shape[0], 2048):
        s = samples[s0 : s0 + 2048]
        dom = (points[:, None, :] <= s[None, :, :]).all(-1)
        f = f + torch.where(dom, w[s0 : s0 + 2048][None, :], torch.zeros((), device=f.device)).sum(1)
    return f


def hype_fused_ok(n: int, m: int, n_sample: int) -> bool:
    """The per-run shapes ``hype_fitness.hip`` takes (``evx_hype_fused_ok`` checks the same in the op)."""
    return 1 <= n <= HYPE_MAX_N and 1 <= m <= HV_MAX_M and 1 <= n_sample <= HYPE_MAX_SAMPLES


def hype_fitness(points: torch.Tensor, ref: torch.Tensor, alpha: torch.Tensor, key: torch.Tensor, n_sample: int) -> torch.Tensor:
    """HypE's unscaled Monte-Carlo fitness ``f_i = Σ_s [p_i ≤ x_s in every objective] · α[c_s − 1]`` with
    ``c_s = #{i : p_i ≤ x_s}`` (terms with ``c_s = 0`` drop out) over the samples
    ``x = uniform(key, (n_sample, m)) * (ref − f_min) + f_min``, ``f_min`` the column minimum of ``points``.

    ``points`` (n, m), ``ref`` (m,), ``key`` (2,) give ``f`` (n,); ``points`` (B, n, m), ``ref`` (B, m), ``key`` (B, 2) are B
    independent runs and give (B, n), row b being the call on run b.  ``alpha`` (n,) is shared by the runs.

    Contract: ``f`` equals bit for bit ``hv_contrib(x, points, hv_count(x, points, False), alpha)``.  On a HIP device, for
    float32 operands with ``hype_fused_ok(n, m, n_sample)``, that is two launches of ``hype_fitness.hip`` for all B runs which
    write no sample array: sample s, objective k is element ``s·m + k`` of the Philox stream of ``key`` (same block, word and
    24-bit mapping as ``random.uniform``), scaled in float32 with two roundings; partial t of 256 adds the terms of
    ``s = t, t + 256, …`` in increasing s from 0 and the partials reduce by the tree ``o = 128, …, 1``, which is
    ``hv_contrib``'s order.  Everywhere else (CPU tensors, other dtypes, shapes outside the caps) it is that composition itself,
    run by run for 3-D points."""
    n_sample = int(n_sample)
    n, m = points.shape[-2:]
    if points.is_cuda and key.device == points.device and points.dtype == ref.dtype == alpha.dtype == torch.float32:
        if hype_fused_ok(n, m, n_sample):
            return _ext.ops().hype_fitness(points.contiguous(), ref.contiguous(), alpha.contiguous(), key.contiguous(), n_sample)
        if points.dim() == 3:
            raise NotImplementedError(f"hype_fitness: batched runs need n <= {HYPE_MAX_N}, m <= {HV_MAX_M} and n_sample <= "
                                      f"{HYPE_MAX_SAMPLES} per run, got n = {n}, m = {m}, n_sample = {n_sample}")
    if points.dim() == 3:
        return torch.stack([hype_fitness(p, r, alpha, k, n_sample) for p, r, k in zip(points, ref, key)])
    from . import random as rnd

    f_min = points.min(0).values
    samples = rnd.uniform(key, (n_sample, m)).to(points.device) * (ref - f_min) + f_min
    return hv_contrib(samples, points, hv_count(samples, points, strict=False), alpha)
