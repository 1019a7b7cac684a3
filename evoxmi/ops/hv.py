"""Exact hypervolume of n boxes ``[0, p_i]`` at m = 2, 3, 4 objectives, and the exclusive contribution of every row at
m = 2, 3 (``hv_exact.hip`` on a HIP device with float32 points, a vectorised float64 torch path elsewhere).

The contract.  ``p (n, m)`` are the points with negative coordinates clamped to 0 (such a row has an empty box); all
arithmetic is float64 on them, without FMA contraction in the kernels.  ``HV(p)`` is the volume of the union of the boxes.

The primitive ``A(keep, cx, cy)``: walk the rows by x descending, ties by original index; skip the rows outside ``keep``;
clip the others to ``x' = min(x_j, cx)``, ``y' = min(y_j, cy)`` (no clip: ``cx = cy = +inf``); ``pm`` is the maximum of
the ``y'`` seen before the row, 0 at the start; ``A = Σ x' · max(0, y' − pm)``, the area of the union of the kept,
clipped rectangles.  Clipping by a constant keeps the order, so one sort serves every call.

* ``zrank_j`` is the position of row j in "z descending, ties by index", ``z_(k)`` the sorted values with ``z_(n) = 0``
  and ``h_k = z_(k) − z_(k+1)``; ``wrank`` and ``g_l`` are the same over the fourth coordinate.
* totals: ``HV = A(all)`` at m = 2, ``Σ_k h_k · A(zrank ≤ k)`` at m = 3 and
  ``Σ_l g_l · Σ_k h_k · A(wrank ≤ l and zrank ≤ k)`` at m = 4; slices of height 0 are skipped.
* contribution of row i, ``c_i = HV(p) − HV(p without i)``: ``c_i = x_i·y_i − A(j ≠ i, clip (x_i, y_i))`` at m = 2 and
  ``Σ_{k ≥ zrank_i} h_k · (x_i·y_i − A(j ≠ i and zrank_j ≤ k, clip (x_i, y_i)))`` at m = 3.  The difference is summed in
  the complementary form: with ``d_j = max(0, y'_j − pm_j)`` and ``pm_end`` the last maximum,
  ``x_i·y_i − A = x_i · (y_i − pm_end) + Σ_j (x_i − x'_j) · d_j``, every term of which is ≥ 0 and at most the area of
  box i.  So the rounding error scales with box i, not with the whole hypervolume, and nothing cancels.

Bounds for finite inputs, u = 2⁻⁵³, against the exact rational value on the same float32 points.  Every term summed is
non-negative, so the error is the number of roundings on the longest path times u: a handful of subtractions and
products per term, fewer than n additions inside ``A`` and fewer than n across the slices (fewer than 2n at m = 4).

* totals: relative error ≤ (2n + 16)·u at m ≤ 3 and ≤ (3n + 16)·u at m = 4;
* contributions: absolute error ≤ (2n + 16)·u·vol(box i);
* a row whose box lies inside another row's box, an exact duplicate included, gets exactly 0: in every slice of positive
  height the covering row is kept; the rows before it have ``x' = x_i``, and after it ``d = 0``.

The order of every sum is fixed (no float atomics), so a second call is bitwise equal.  The two paths sum in different
orders and agree within the bounds, not bitwise.  With NaN or ±inf the launches end and the shapes hold, nothing more.

On the device: torch's stable sort of the three or four columns, two small launches that build the ranks, the heights and
the x-ordered rows, one scan launch with a wave64 per slice, and for the total one reduction in a fixed order.  Nothing is
read on the host, the launch count depends on (n, m) alone, and the scratch is O(n) words, so a call captures into a graph.
"""
from __future__ import annotations

import torch

from . import _ext

# rows; not structural: they keep a call within tens of milliseconds (the scan does n²/64 chunk steps for a total at m = 3,
# n³/64 at m = 4 and n³/128 for the contributions at m = 3)
N_CAP = {2: 32768, 3: 32768, 4: 2048}
N_CAP_CONTRIB = {2: 32768, 3: 2048}
_CHUNK = 1 << 22  # elements of one (slices, n) block of the torch path


def on_device(n: int, m: int, device, contributions: bool = False) -> bool:
    """Whether n float32 rows of m objectives on ``device`` run the kernels."""
    cap = (N_CAP_CONTRIB if contributions else N_CAP).get(m, 0)
    return torch.device(device).type == "cuda" and 1 <= n <= cap


def _check(points: torch.Tensor, caps: dict, what: str):
    if points.dim() != 2:
        raise ValueError(f"{what}: points must be (n, m), got {tuple(points.shape)}")
    n, m = points.shape
    other = "the Monte-Carlo estimators (metrics.HV) or metrics.exact_hv on the host"
    if m not in caps:
        raise ValueError(f"{what} is offered at m in {sorted(caps)}, got m = {m}; use {other}")
    if n > caps[m]:
        raise ValueError(f"{what} at m = {m} is capped at n <= {caps[m]} rows, got n = {n}; use {other}")
    return n, m


def _sorted_columns(points: torch.Tensor):
    """The (m, n) transpose clamped at 0 (−0 becomes +0, so that equal values have one bit pattern), its rows sorted
    descending by a stable sort, and the original positions."""
    pT = (points.t().clamp(min=0) + 0.0).contiguous()
    vals, idx = torch.sort(pT, dim=1, descending=True, stable=True)
    return pT, vals, idx


def _areas(x, y, keep, cx=None, cy=None):
    """``A`` of the S slices ``keep (S, n)`` over the x-ordered rows ``x, y (n,)``; with a clip ``cx, cy (S,)`` the
    complement ``cx·cy − A`` in the form of the contract."""
    S = keep.shape[0]
    if cx is None:
        xx, yy = x[None, :], torch.where(keep, y[None, :], 0.0)
    else:
        xx, yy = torch.minimum(x[None, :], cx[:, None]), torch.where(keep, torch.minimum(y[None, :], cy[:, None]), 0.0)
    inc = torch.cummax(yy, dim=1).values
    prev = torch.cat([inc.new_zeros(S, 1), inc[:, :-1]], dim=1)
    d = (yy - prev).clamp(min=0)
    if cx is None:
        return (xx * d).sum(1)
    return cx * (cy - inc[:, -1]) + ((cx[:, None] - xx) * d).sum(1)


def _torch_setup(points):
    n, m = points.shape
    pT, vals, idx = _sorted_columns(points.to(torch.float64))
    ox = idx[0]
    x, y = vals[0], pT[1][ox]
    pos = torch.arange(n, device=points.device)
    ranks, heights = [], []
    for c in range(2, m):
        rank = torch.empty_like(pos)
        rank[idx[c]] = pos
        ranks.append(rank[ox])
        heights.append(vals[c] - torch.cat([vals[c][1:], vals[c].new_zeros(1)]))
    return n, m, x, y, ox, pos, ranks, heights


def _torch_exact(points):
    n, m, x, y, ox, pos, ranks, heights = _torch_setup(points)
    if m == 2:
        return _areas(x, y, torch.ones(1, n, dtype=torch.bool, device=points.device))[0]
    total = x.new_zeros(())
    nsl = n if m == 3 else n * n
    step = max(1, _CHUNK // n)
    for s0 in range(0, nsl, step):  # over blocks of slices, never over points
        s = torch.arange(s0, min(nsl, s0 + step), device=points.device)
        if m == 3:
            keep, wgt = ranks[0][None, :] <= s[:, None], heights[0][s]
        else:
            l, k = s // n, s % n
            keep = (ranks[1][None, :] <= l[:, None]) & (ranks[0][None, :] <= k[:, None])
            wgt = heights[1][l] * heights[0][k]
        total = total + (wgt * _areas(x, y, keep)).sum()
    return total


def _torch_contributions(points):
    n, m, x, y, ox, pos, ranks, heights = _torch_setup(points)
    c = x.new_zeros(n)
    nsl = n if m == 2 else n * n
    step = max(1, _CHUNK // n)
    for s0 in range(0, nsl, step):
        s = torch.arange(s0, min(nsl, s0 + step), device=points.device)
        if m == 2:
            i, keep, wgt = s, pos[None, :] != s[:, None], None
        else:
            i, k = s // n, s % n
            keep = (pos[None, :] != i[:, None]) & (ranks[0][None, :] <= k[:, None])
            wgt = torch.where(k >= ranks[0][i], heights[0][k], 0.0)
        part = _areas(x, y, keep, x[i], y[i])
        c.index_add_(0, i, part if wgt is None else wgt * part)
    out = torch.empty_like(c)
    out[ox] = c
    return out


def exact(points: torch.Tensor) -> torch.Tensor:
    """The hypervolume of the boxes ``[0, p_i]`` of ``points (n, m)``, m = 2, 3, 4, as a 0-d float64 tensor on the input's
    device; 0 for n = 0.  A ``ValueError`` outside ``N_CAP`` or at another m."""
    n, m = _check(points, N_CAP, "the exact hypervolume")
    if n == 0:
        return torch.zeros((), dtype=torch.float64, device=points.device)
    if points.dtype == torch.float32 and on_device(n, m, points.device):
        return _ext.ops().hv_exact(*_sorted_columns(points))
    return _torch_exact(points)


def contributions(points: torch.Tensor) -> torch.Tensor:
    """``c (n,) float64`` on the input's device: ``c_i = HV(points) − HV(points without row i)``, m = 2, 3.  A
    ``ValueError`` outside ``N_CAP_CONTRIB`` or at another m."""
    n, m = _check(points, N_CAP_CONTRIB, "the hypervolume contributions")
    if n == 0:
        return torch.zeros(0, dtype=torch.float64, device=points.device)
    if points.dtype == torch.float32 and on_device(n, m, points.device, contributions=True):
        return _ext.ops().hv_contributions(*_sorted_columns(points))
    return _torch_contributions(points)
