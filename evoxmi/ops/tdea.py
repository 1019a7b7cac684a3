"""θ-DEA's θ-ranking: every row joins its closest reference direction and is ranked inside it by the penalised distance
d1 + θ·d2 (``rvea_select.hip`` and ``tdea_select.hip`` on a HIP device, the dense torch expression
``algorithms.mo.tdea.theta_nd_sort`` elsewhere).

The kernels' contract, on top of ``ops.rvea.cos_best(obj, w)`` (no shift, no floor, no clamp) and its contract.  All
arithmetic is float64 on the float32 inputs, in the operation order written here, without FMA contraction; a host
implementation of the same operations reproduces ``cls``, ``val`` and ``t_rank`` exactly.

``theta_rank(obj (n, m), w (nw, m), mask (n))`` → ``t_rank (n) float32``; ``obj`` is the normalised objectives:

* ``cls_i = arg_i``, the lowest position of the largest float64 cosine ``best_i`` (for non-negative rows the direction
  of smallest d2); a NaN row's −1 becomes 0;
* ``c = min(max(best_i, −1), 1)``; ``|a| = sqrt(((a_0² + a_1²) + a_2²) + …)`` with ``a = (double)obj_i``;
* ``d1 = |a| · c`` and ``d2 = |a| · sqrt(max(1 − c · c, 0))``;
* ``θ_j`` is 1e6 where exactly one component of ``w_j`` exceeds 1e-4, else 5; torch computes it, a float32 (nw,) array;
* ``val_i = d1 + (double)θ_cls · d2``;
* a masked row: ``t_rank_i = 1 + #{ j masked, cls_j = cls_i, (val_j, j) < (val_i, i) lexicographically }``, an exact
  count; a NaN ``val`` orders after every number;
* a row outside the mask: ``t_rank_i = +inf``.

That holds for finite rows of positive norm and finite, non-zero ``w``.  For anything else the launches end, ``cls``
lies in [0, nw) and the masked rows of a cluster still get the distinct ranks 1 … c.

Four launches (two of them ``cos_best``'s), no host read, no (n, nw) array and no sort."""
from __future__ import annotations

import torch

from . import _ext
from .rvea import M_CAP, N_CAP, _kernel_path  # the caps and the dispatch are cos_best's

__all__ = ["M_CAP", "N_CAP", "theta_rank", "theta_of"]


def theta_of(w: torch.Tensor) -> torch.Tensor:
    """θ of every direction: 1e6 on the axes (exactly one component above 1e-4), 5 elsewhere; float32 (nw,)."""
    nw = w.shape[0]
    return torch.where((w > 1e-4).sum(1) == 1, torch.full((nw,), 1e6, device=w.device), torch.full((nw,), 5.0, device=w.device))


def theta_rank(obj: torch.Tensor, w: torch.Tensor, mask: torch.Tensor, return_parts: bool = False):
    """``t_rank`` (n,) float32: the rank of every masked row of ``obj`` (n, m) inside its direction of ``w`` (nw, m) by
    d1 + θ·d2, +inf outside the mask.  On a HIP device within the caps the kernels (``return_parts`` adds ``cls``, int64,
    and ``val``, float64); elsewhere the dense float32 expression of ``algorithms.mo.tdea``."""
    if _kernel_path(obj, w):
        mask = mask.to(device=obj.device, dtype=torch.bool).contiguous()
        t_rank, cls, val = _ext.ops().tdea_theta_rank(obj.contiguous(), w.contiguous(), theta_of(w).contiguous(), mask)
        return (t_rank, cls.to(torch.int64), val) if return_parts else t_rank
    if return_parts:
        raise ValueError("return_parts is the kernels' only")
    from ..algorithms.mo.tdea import theta_nd_sort

    return theta_nd_sort(obj, w, mask)
