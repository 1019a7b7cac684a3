"""The RVEA family's selection primitives: the best cosine of every row to a set of vectors, and the angle-penalised
distance (APD) selection on top of it (``rvea_select.hip`` on a HIP device, the dense torch expressions elsewhere).
RVEA, RVEA* and LMOCSO select with ``select``; RVEA*'s vector regeneration and batch truncation use ``cos_best``.

The kernels' contract.  All arithmetic is float64 on the float32 inputs, in the operation order written here, without
FMA contraction; a host implementation of the same operations reproduces the cosines bit for bit and everything else
to an ulp of ``acos``.

``cos_best(A (n, m), shift (m) or none, floor, B (k, m), clamp, self_zero)`` → ``best (n) float64``, ``arg (n) int32``:

* row vector: ``a = (double)A_i − (double)shift`` if a shift is given, then ``max(a, floor)`` if a floor is given (a
  NaN stays a NaN);
* norm: ``|a| = sqrt(((a_0² + a_1²) + a_2²) + …)``; normalised row: ``â_k = a_k / |a|``;
* ``b̂_j`` is formed the same way from ``B_j``, without shift or floor, once, by a preparatory launch into a float64
  scratch of k·m words;
* cosine: ``c_ij = ((â_0·b̂_j0 + â_1·b̂_j1) + â_2·b̂_j2) + …``, which is symmetric bit for bit when A = B, so mutual nearest
  neighbours tie exactly;
* a NaN ``c`` counts as −∞; otherwise, with ``clamp``, ``c ← min(max(c, 0), 1)``;
* with ``self_zero`` (which needs A = B) the entry j = i counts as exactly 0, also for a row that holds a NaN;
* ``best_i = max_j c_ij`` and ``arg_i`` the lowest j that attains it; ``arg_i = 0`` when every entry is −∞;
* a row of A that holds a NaN gives ``arg_i = −1``, and ``best_i = 0`` with ``self_zero``, −∞ without.

The APD epilogue runs in the launch of the association ``cos_best(f, colmin, 1e-32, v, clamp)``.  For every row with
``arg_i ≥ 0``: ``angle_i = acos(best_i)``, ``norm_i = |a|`` and
``apd_i = (1 + (((double)m · (double)θ) · angle_i) / γ_{arg_i}) · norm_i``, with θ read from a float32 device word and
``γ_j = acos(best_j)`` of ``cos_best(v, none, none, v, clamp, self_zero)``.

``apd_pick(arg (n), apd (n), nv)`` → ``next_ind (nv) int64``, ``empty (nv) bool``: for vector j, among the rows with
``arg == j``, the one of least ``apd``, the lowest position on equal values; a non-finite ``apd`` compares as +∞;
``empty_j`` is true when the vector has no member, and then ``next_ind_j = 0``.  The pick is an integer atomic min of
the ordered bits of ``apd`` per vector, then an atomic min of the positions that hold it: neither depends on scheduling.

That holds for finite objectives plus whole-NaN padding rows, and reference vectors that are finite, non-zero and
pairwise not parallel (γ > 0).  A row with ±∞, a zero or non-finite vector, or γ = 0 get only this: the launches end,
``next_ind`` lies in [0, n) and ``arg`` in [−1, k).  (The torch path lets a NaN win an ``argmin`` there.)

The torch path is the expressions ``ref_vec_guided``, ``rv_regeneration`` and ``batch_truncation`` held before, in
float32; it is the CPU path, the path above the caps, and the oracle of the float32 behaviour."""
from __future__ import annotations

import torch

from ..utils.common import cos_dist
from . import _ext

M_CAP = 16  # rvea_select.hip: â stays in registers
N_CAP = 32768  # rows and vectors; not structural: it bounds the scratch (RVEA* at pop 8192 merges n = 24576 rows)


def on_device(n: int, k: int, m: int, device) -> bool:
    """Whether n rows against k vectors of m objectives on ``device`` run the kernels."""
    return torch.device(device).type == "cuda" and 1 <= n <= N_CAP and 1 <= k <= N_CAP and 1 <= m <= M_CAP


def _kernel_path(a, b):
    return a.dim() == 2 and b.dim() == 2 and a.dtype == torch.float32 and b.dtype == torch.float32 and on_device(
        a.shape[0], b.shape[0], a.shape[1], a.device)


def cos_best(a: torch.Tensor, b: torch.Tensor, *, shift=None, floor=None, clamp: bool = False, self_zero: bool = False):
    """``(best, arg)``: for every row of ``a`` (n, m), less ``shift`` (m,) and raised to ``floor`` where given, the largest
    cosine to a row of ``b`` (k, m) and the first position that holds it, int64, −1 for a row that holds a NaN.  On a HIP
    device within the caps ``best`` is float64 (two launches, no (n, k) array, no host read); elsewhere it is the dense
    float32 expression.  The inputs are left as they are."""
    if _kernel_path(a, b):
        best, arg = _ext.ops().rvea_cos_best(a.contiguous(), None if shift is None else shift.to(torch.float32).contiguous(),
                                             None if floor is None else float(floor), b.contiguous(), bool(clamp), bool(self_zero))
        return best, arg.to(torch.int64)
    obj = a if shift is None else a - shift
    if floor is not None:
        obj = torch.clamp(obj, min=floor)
    cosine = cos_dist(obj, b)
    if self_zero:
        cosine = cosine.masked_fill(torch.eye(cosine.shape[0], dtype=torch.bool, device=a.device), 0)
    if clamp:
        cosine = cosine.clamp(0, 1)
    cosine = torch.nan_to_num(cosine, nan=-float("inf"))
    arg = torch.argmax(cosine, 1)
    return cosine.max(1).values, torch.where(torch.isnan(a).any(1), torch.full_like(arg, -1), arg)


def _select_torch(f, v, theta):
    n, m = f.shape
    nv = v.shape[0]
    obj = f - torch.nan_to_num(f, nan=float("inf")).min(0).values
    obj = torch.clamp(obj, min=1e-32)
    cosine = cos_dist(v, v)
    cosine = cosine.masked_fill(torch.eye(nv, dtype=torch.bool, device=v.device), 0)
    cosine = cosine.clamp(0, 1)
    gamma = torch.arccos(cosine).min(1).values
    angle = torch.arccos(cos_dist(torch.nan_to_num(obj, nan=0.0), v).clamp(0, 1))
    nan_mask = torch.isnan(obj).any(1)
    associate = torch.argmin(angle, 1)
    associate = torch.where(nan_mask, torch.full_like(associate, -1), associate)
    norm = torch.sqrt((torch.nan_to_num(obj, nan=0.0) ** 2).sum(1))
    member = associate[:, None] == torch.arange(nv, device=v.device)[None, :]  # (n, nv)
    apd = (1 + m * theta * angle / gamma[None, :]) * norm[:, None]
    apd = torch.where(member, apd, torch.full_like(apd, float("inf")))
    next_ind = torch.argmin(apd, 0)
    empty = ~member.any(0)
    return next_ind, empty


def select(f: torch.Tensor, v: torch.Tensor, theta, return_info: bool = False):
    """``(next_ind, empty)``: RVEA's APD selection of the rows ``f`` (n, m), NaN rows being padding, on the reference
    vectors ``v`` (nv, m): ``next_ind`` (nv,) int64 the row each vector keeps and ``empty`` (nv,) bool the vectors
    without a member.  ``theta`` is a Python float or a 0-dim tensor.  On a HIP device within the caps five launches of
    ``rvea_select.hip`` that read nothing on the host and build no (n, nv) array (``return_info`` adds ``arg``, ``apd`` and
    ``gamma``); elsewhere the dense float32 expressions."""
    if _kernel_path(f, v):
        if not isinstance(theta, torch.Tensor):
            theta = torch.tensor(float(theta), dtype=torch.float32)
        theta = theta.to(device=f.device, dtype=torch.float32)
        shift = torch.nan_to_num(f, nan=float("inf")).min(0).values  # exact in torch
        next_ind, empty, arg, apd, gamma = _ext.ops().rvea_select(f.contiguous(), shift, 1e-32, v.contiguous(), theta)
        return (next_ind, empty, arg.to(torch.int64), apd, gamma) if return_info else (next_ind, empty)
    if return_info:
        raise ValueError("return_info is the kernels' only")
    return _select_torch(f, v, theta)
