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

Four launches (two of them ``cos_best``'s), no host read, no (n, nw) array and no sort.

``theta_rank`` on ``obj`` (B, n, m), and ``tdea_theta_rank`` under ``vmap`` (``evoxmi/ops/batching.py``), rank B independent runs in
one launch of ``tdea_small.hip``: a workgroup per run with the run's b̂, θ, ``cls`` and ``val`` in LDS, the same operations
(``csrc/include/evoxmi_rvea.h`` and ``evoxmi_tdea.h`` hold them for both paths), so every run gets the words of the launches above.
There the count runs over the rows of the own cluster only, whose member lists are built in LDS.  Its caps per run are those of
``ops.rvea.small_ok``; above them it raises, it does not go run by run."""
from __future__ import annotations

import torch

from . import _ext
from .nds import _in_vmap
from .rvea import M_CAP, N_CAP, _kernel_path, check_small_caps  # the caps and the dispatch are cos_best's, the batched caps rvea_small's

__all__ = ["M_CAP", "N_CAP", "theta_rank", "theta_of"]


def theta_of(w: torch.Tensor) -> torch.Tensor:
    """θ of every direction: 1e6 on the axes (exactly one component above 1e-4), 5 elsewhere; float32 (nw,), or (B, nw) of
    w (B, nw, m)."""
    nw = w.shape[-2]
    return torch.where((w > 1e-4).sum(-1) == 1, torch.full((nw,), 1e6, device=w.device), torch.full((nw,), 5.0, device=w.device))


def _theta_rank_torch(obj, w, mask):
    from ..algorithms.mo.tdea import theta_nd_sort

    return theta_nd_sort(obj, w, mask)


def _theta_rank_runs(obj, w, mask, return_parts):
    B, n, m = obj.shape
    mask = mask.to(device=obj.device, dtype=torch.bool)
    if obj.device.type == "cuda":
        if obj.dtype != torch.float32 or w.dtype != torch.float32:
            raise NotImplementedError("ops.tdea.theta_rank: batched runs on a device need float32 objectives and directions")
        check_small_caps(n, w.shape[-2], m, "ops.tdea.theta_rank")
        t_rank, cls, val = _ext.ops().tdea_small_theta_rank(obj.contiguous(), w.contiguous(), theta_of(w).contiguous(), mask.contiguous())
        return (t_rank, cls.to(torch.int64), val) if return_parts else t_rank
    if return_parts:
        raise ValueError("return_parts is the kernels' only")
    return torch.stack([_theta_rank_torch(obj[r], w if w.dim() == 2 else w[r], mask[r]) for r in range(B)])


@torch.library.custom_op("evoxmi_py::tdea_theta_rank_run", mutates_args=())
def _theta_rank_run(obj: torch.Tensor, w: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The dense torch expression on obj (n, m), or run by run on (B, n, m): it writes in place into an unbatched tensor, so ``vmap``
    cannot trace through it; this op is what a vmapped CPU call reaches."""
    if obj.dim() == 3:
        return _theta_rank_runs(obj, w, mask, False)
    return _theta_rank_torch(obj, w, mask)


@_theta_rank_run.register_fake
def _(obj, w, mask):
    return obj.new_empty(obj.shape[:-1], dtype=torch.float32)


@torch.library.register_vmap("evoxmi_py::tdea_theta_rank_run")
def _(info, in_dims, obj, w, mask):
    B = info.batch_size
    ob, mb = (t.unsqueeze(0).expand((B,) + tuple(t.shape)) if d is None else t.movedim(d, 0) for t, d in ((obj, in_dims[0]), (mask, in_dims[2])))
    return _theta_rank_run(ob, w if in_dims[1] is None else w.movedim(in_dims[1], 0), mb), 0


def theta_rank(obj: torch.Tensor, w: torch.Tensor, mask: torch.Tensor, return_parts: bool = False):
    """``t_rank`` (n,) float32: the rank of every masked row of ``obj`` (n, m) inside its direction of ``w`` (nw, m) by
    d1 + θ·d2, +inf outside the mask.  On a HIP device within the caps the kernels (``return_parts`` adds ``cls``, int64,
    and ``val``, float64); elsewhere the dense float32 expression of ``algorithms.mo.tdea``.

    ``obj`` (B, n, m) with ``mask`` (B, n) ranks B independent runs: ``w`` is (B, nw, m) or one (nw, m) for all runs, and every
    result gains a leading run axis.  On a HIP device that is ONE launch of ``tdea_small.hip``, a workgroup per run, whose words
    are those of the 2-D call on each run; runs above its caps (``ops.rvea.small_ok``) raise ``NotImplementedError``.  On the CPU
    the 2-D path runs run by run, also for a run under ``vmap``."""
    if obj.dim() == 3:
        return _theta_rank_runs(obj, w, mask, return_parts)
    if _kernel_path(obj, w):
        mask = mask.to(device=obj.device, dtype=torch.bool).contiguous()
        t_rank, cls, val = _ext.ops().tdea_theta_rank(obj.contiguous(), w.contiguous(), theta_of(w).contiguous(), mask)
        return (t_rank, cls.to(torch.int64), val) if return_parts else t_rank
    if return_parts:
        raise ValueError("return_parts is the kernels' only")
    if not obj.is_cuda and _in_vmap(obj):
        return _theta_rank_run(obj, w, mask)
    return _theta_rank_torch(obj, w, mask)
