"""SPEA2's fitness and environmental selection: strength, raw fitness and second-nearest-neighbour
density, and the one-by-one truncation of the non-dominated set (``spea2_select.hip`` on a HIP
device, the torch expressions on the CPU).

The kernels' contract, where it is sharper than the torch path's: ``d2`` is the float32 squared
distance summed with ``fmaf`` over the objectives in ascending order (a NaN counts as +inf);
``D = 1 / (sqrt(second smallest d2) + 2)``; ``R`` is the exact integer sum of the dominators'
strengths, rounded once; a truncation step removes the live masked row of least
``(nearest-neighbour d2, index)`` — the lowest index of the exactly tied closest pair — and the
lowest-index live masked row where every such distance is +inf.

``fitness``, ``truncate`` and ``select`` take ``obj`` (B, n, m) as B independent runs: row b of every
output is the 2-D call on ``obj[b]``, bit for bit.  On a HIP device that is the same launches with
the run on the grid (a workgroup per run in the removal kernel, each run counting its own
removals).  On the CPU the torch path has data-dependent control flow (the size of the
non-dominated set, the length of the removal loop) and ``torch.cdist`` changes its form with the
row count, so 3-D input and calls under ``vmap`` (``BatchedRuns``) go through Python-registered ops
that apply the 2-D torch path run by run.  Under ``vmap`` on a device a per-run shape above the
caps raises ``NotImplementedError`` instead of running the dense torch path for every run."""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _ext
from .nds import _in_vmap
from ..utils.common import dominate_relation

N_CAP = 8192  # spea2_select.hip, truncation: one workgroup, n ≤ 8192 rows
FIT_N_CAP = 32768  # spea2_select.hip, fitness: the raw-fitness accumulator is 32 bits
M_CAP = 16  # spea2_select.hip, every kernel: m ≤ 16 objectives


def on_device(n: int, m: int, device) -> bool:
    """Whether a merged population of n rows and m objectives on ``device`` runs the kernels."""
    return torch.device(device).type == "cuda" and 2 <= n <= N_CAP and 1 <= m <= M_CAP


def _fitness_on_device(obj) -> bool:
    return obj.is_cuda and obj.dim() == 2 and 2 <= obj.shape[0] <= FIT_N_CAP and 1 <= obj.shape[1] <= M_CAP


def check_batched_caps(n: int, m: int, what: str, n_cap: int = N_CAP) -> None:
    """The per-run caps of the kernels; above them there is no batched form, and the dense torch
    path for every run would hide that."""
    if n < 2 or n > n_cap or m < 1 or m > M_CAP:
        raise NotImplementedError(f"{what}: batched runs need 2 <= n <= {n_cap} rows and 1 <= m <= {M_CAP} objectives per run, "
                                  f"got n = {n}, m = {m}")


# ---------------------------------------------------------------- the torch path and the kernels' oracle
def cal_fitness(obj):
    n = obj.shape[0]
    dom = dominate_relation(obj, obj)  # dom[i, j]: i dominates j
    S = dom.sum(1).to(torch.float32)
    R = (dom.to(torch.float32) * S[:, None]).sum(0)
    dis = torch.cdist(obj, obj)
    dis = dis.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), float("inf"))
    k = int(math.floor(math.sqrt(6))) - 1
    D = 1 / (torch.sort(dis, dim=1).values[:, k] + 2)
    return D + R


def truncation(obj, k, mask):
    """Remove ``k`` of the masked points, each time the one whose nearest neighbour is closest."""
    n = obj.shape[0]
    dis = torch.cdist(obj, obj)
    dis = dis.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), float("inf"))
    dis = torch.where(mask[:, None] & mask[None, :], dis, torch.full_like(dis, float("inf")))
    keep = torch.ones(n, dtype=torch.bool, device=obj.device)
    for _ in range(k):
        idx = torch.argmin(dis.min(1).values)
        keep[idx] = False
        dis[idx, :] = float("inf")
        dis[:, idx] = float("inf")
    return keep & mask


def truncation_predicated(obj, k, mask, max_k: int):
    """``truncation`` with a device-resident removal count ``k`` (≤ ``max_k``)."""
    n = obj.shape[0]
    inf = float("inf")
    dis = torch.cdist(obj, obj)
    dis = dis.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), inf)
    dis = torch.where(mask[:, None] & mask[None, :], dis, torch.full_like(dis, inf))
    keep = torch.ones(n, dtype=torch.bool, device=obj.device)
    col = torch.arange(n, device=obj.device)
    for step in range(max_k):
        act = k > step
        idx = torch.argmin(dis.min(1).values)
        hit = (col == idx) & act
        keep = keep & ~hit
        dis = dis.masked_fill(hit[:, None] | hit[None, :], inf)
    return keep & mask


def _parts(obj):
    """``cal_fitness`` with its parts: ``(sig, S, R, D, nd)``."""
    n = obj.shape[0]
    dom = dominate_relation(obj, obj)
    S = dom.sum(1).to(torch.float32)
    R = (dom.to(torch.float32) * S[:, None]).sum(0)
    dis = torch.cdist(obj, obj)
    dis = dis.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), float("inf"))
    k = int(math.floor(math.sqrt(6))) - 1
    D = 1 / (torch.sort(dis, dim=1).values[:, k] + 2)
    return D + R, S.to(torch.int32), R, D, ~dom.any(0)


def _truncation_order(obj, k, mask):
    """``truncation`` that also records the removed rows."""
    n = obj.shape[0]
    dis = torch.cdist(obj, obj)
    dis = dis.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), float("inf"))
    dis = torch.where(mask[:, None] & mask[None, :], dis, torch.full_like(dis, float("inf")))
    keep = torch.ones(n, dtype=torch.bool, device=obj.device)
    xs = []
    for _ in range(k):
        idx = torch.argmin(dis.min(1).values)
        xs.append(idx)
        keep[idx] = False
        dis[idx, :] = float("inf")
        dis[:, idx] = float("inf")
    return keep & mask, xs


# ---------------------------------------------------------------- the torch path, one run and run by run
def _truncate_torch(obj, mask, n_keep: int, return_order: bool):
    n, dev = obj.shape[0], obj.device
    k = max(0, int(mask.sum()) - n_keep)
    if not return_order:
        return truncation(obj, k, mask)
    keep, xs = _truncation_order(obj, k, mask)
    order = torch.full((max(n - n_keep, 0),), -1, dtype=torch.int64, device=dev)
    if xs:
        order[: len(xs)] = torch.stack(xs)
    return keep, order, torch.zeros((), dtype=torch.int32, device=dev)


def _select_torch(obj, n_keep: int):
    sig = cal_fitness(obj)
    mask = sig < 1
    if obj.is_cuda and torch.cuda.is_current_stream_capturing():
        # capturable form: the removal count stays on the device; a fixed n_keep-step loop with
        # predicated updates replaces the data-dependent one, and the branch becomes a select
        num_valid = mask.sum()
        keep = truncation_predicated(obj, num_valid - n_keep, mask, n_keep)
        key = torch.where(num_valid <= n_keep, sig, (~keep).to(sig.dtype))
        order = torch.argsort(key, stable=True)
    else:
        num_valid = int(mask.sum())
        if num_valid <= n_keep:
            order = torch.argsort(sig, stable=True)
        else:
            keep = truncation(obj, num_valid - n_keep, mask)
            order = torch.argsort((~keep).to(torch.int64), stable=True)
    return order[:n_keep]


def _stacked(outs):
    return tuple(torch.stack(t) for t in zip(*outs))


# What a vmapped or 3-D call reaches where the torch path is due (the CPU): ``vmap`` cannot trace through the 2-D functions
# above, so ``*_run`` is one run as an op and its rule is ``*_runs``, the same function run by run: by construction the
# sequential result, and the oracle the batched device kernels are held to.
@torch.library.custom_op("evoxmi_py::spea2_fitness_runs", mutates_args=())
def _fitness_runs(obj: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _stacked([_parts(o) for o in obj])


@_fitness_runs.register_fake
def _(obj):
    e = lambda dt: obj.new_empty(obj.shape[:2], dtype=dt)
    return e(obj.dtype), e(torch.int32), e(torch.float32), e(obj.dtype), e(torch.bool)


@torch.library.custom_op("evoxmi_py::spea2_fitness_run", mutates_args=())
def _fitness_run(obj: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return _parts(obj)


@_fitness_run.register_fake
def _(obj):
    e = lambda dt: obj.new_empty(obj.shape[:1], dtype=dt)
    return e(obj.dtype), e(torch.int32), e(torch.float32), e(obj.dtype), e(torch.bool)


@torch.library.register_vmap("evoxmi_py::spea2_fitness_run")
def _(info, in_dims, obj):
    return _fitness_runs(obj.movedim(in_dims[0], 0)), (0,) * 5


@torch.library.custom_op("evoxmi_py::spea2_truncate_runs", mutates_args=())
def _truncate_runs(obj: torch.Tensor, mask: torch.Tensor, n_keep: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _stacked([_truncate_torch(o, k, n_keep, True) for o, k in zip(obj, mask)])


@_truncate_runs.register_fake
def _(obj, mask, n_keep):
    B, n = obj.shape[:2]
    return (obj.new_empty((B, n), dtype=torch.bool), obj.new_empty((B, max(n - n_keep, 0)), dtype=torch.int64),
            obj.new_empty((B,), dtype=torch.int32))


@torch.library.custom_op("evoxmi_py::spea2_truncate_run", mutates_args=())
def _truncate_run(obj: torch.Tensor, mask: torch.Tensor, n_keep: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return _truncate_torch(obj, mask, n_keep, True)


@_truncate_run.register_fake
def _(obj, mask, n_keep):
    n = obj.shape[0]
    return (obj.new_empty((n,), dtype=torch.bool), obj.new_empty((max(n - n_keep, 0),), dtype=torch.int64),
            obj.new_empty((), dtype=torch.int32))


def _run_axis_first(x, bdim, B):
    return x.unsqueeze(0).expand((B,) + tuple(x.shape)) if bdim is None else x.movedim(bdim, 0)


@torch.library.register_vmap("evoxmi_py::spea2_truncate_run")
def _(info, in_dims, obj, mask, n_keep):
    B = info.batch_size
    return _truncate_runs(_run_axis_first(obj, in_dims[0], B), _run_axis_first(mask, in_dims[1], B), n_keep), (0, 0, 0)


@torch.library.custom_op("evoxmi_py::spea2_select_runs", mutates_args=())
def _select_runs(obj: torch.Tensor, n_keep: int) -> torch.Tensor:
    return torch.stack([_select_torch(o, n_keep) for o in obj])


@_select_runs.register_fake
def _(obj, n_keep):
    return obj.new_empty((obj.shape[0], min(n_keep, obj.shape[1])), dtype=torch.int64)


@torch.library.custom_op("evoxmi_py::spea2_select_run", mutates_args=())
def _select_run(obj: torch.Tensor, n_keep: int) -> torch.Tensor:
    return _select_torch(obj, n_keep)


@_select_run.register_fake
def _(obj, n_keep):
    return obj.new_empty((min(n_keep, obj.shape[0]),), dtype=torch.int64)


@torch.library.register_vmap("evoxmi_py::spea2_select_run")
def _(info, in_dims, obj, n_keep):
    return _select_runs(obj.movedim(in_dims[0], 0), n_keep), 0


# ---------------------------------------------------------------- public entries
def fitness(obj: torch.Tensor, return_parts: bool = False):
    """SPEA2's fitness ``sig = D + R`` of the rows of ``obj`` (n, m); with ``return_parts`` also
    the strength ``S`` (int32), the raw fitness ``R``, the density ``D`` and ``nd``, whether no row
    dominates the row.  On a HIP device with 2 ≤ n ≤ 32768 and m ≤ 16 two launches of
    ``spea2_select.hip`` without an (n, n) or (n, n, m) temporary; elsewhere ``cal_fitness``.
    ``obj`` (B, n, m): B runs, every output (B, n)."""
    if obj.dim() == 3 or _in_vmap(obj):
        if obj.is_cuda:
            check_batched_caps(obj.shape[-2], obj.shape[-1], "spea2.fitness", FIT_N_CAP)
            parts = _ext.ops().spea2_fitness(obj.to(torch.float32).contiguous())[:5]
        else:
            parts = _fitness_runs(obj) if obj.dim() == 3 else _fitness_run(obj)
        return tuple(parts) if return_parts else parts[0]
    if _fitness_on_device(obj):
        sig, S, R, D, nd = _ext.ops().spea2_fitness(obj.to(torch.float32).contiguous())[:5]
        return (sig, S, R, D, nd) if return_parts else sig
    return _parts(obj) if return_parts else cal_fitness(obj)


def truncate(obj: torch.Tensor, mask: torch.Tensor, n_keep: int, return_order: bool = False):
    """The bool mask of the rows of ``mask`` that SPEA2's truncation keeps: ``max(0, #mask − n_keep)``
    times the masked row whose nearest masked neighbour is closest is removed.  With
    ``return_order`` also the removed rows in the order of their removal, padded with −1 to
    ``max(n − n_keep, 0)`` entries, and the number of neighbour rescans (int32; 0 on the torch
    path).  On a HIP device within the caps the removal count stays on the device: the masked
    nearest-neighbour pass and the one-workgroup removal kernel; elsewhere ``truncation``.
    ``obj`` (B, n, m) with ``mask`` (B, n): B runs, each removing its own count; keep (B, n), the
    order (B, max(n − n_keep, 0)) and the rescans (B,)."""
    n = obj.shape[-2]
    n_keep = int(n_keep)
    if obj.dim() == 3 or _in_vmap(obj) or _in_vmap(mask):
        if obj.is_cuda:
            check_batched_caps(n, obj.shape[-1], "spea2.truncate")
            if n_keep < 1:
                raise NotImplementedError("spea2.truncate: batched runs need n_keep >= 1")
            keep, order, stats = _ext.ops().spea2_truncate(obj.to(torch.float32).contiguous(), mask.contiguous(), n_keep, None, None)
            rescans = stats[..., 0]
        elif obj.dim() == 3 and not return_order:  # plain tensors: the 2-D call's cheaper path, run by run
            return torch.stack([_truncate_torch(o, k, n_keep, False) for o, k in zip(obj, mask)])
        else:
            keep, order, rescans = (_truncate_runs if obj.dim() == 3 else _truncate_run)(obj, mask, n_keep)
        return (keep, order, rescans) if return_order else keep
    if obj.dim() == 2 and on_device(n, obj.shape[1], obj.device) and n_keep >= 1:
        keep, order, stats = _ext.ops().spea2_truncate(obj.to(torch.float32).contiguous(), mask.contiguous(), n_keep, None, None)
        return (keep, order, stats[0]) if return_order else keep
    return _truncate_torch(obj, mask, n_keep, return_order)


def select(obj: torch.Tensor, n_keep: int):
    """SPEA2's environmental selection of ``n_keep`` of the rows of ``obj`` (n, m), int64 indices:
    with ``mask = sig < 1`` the non-dominated set, the best ``n_keep`` by ``sig`` where it has at
    most ``n_keep`` rows and its truncation otherwise.  On a HIP device within the caps the
    fitness launches, the removal kernel and a stable argsort of ``where(count ≤ n_keep, sig,
    ~keep)``: nothing is read on the host, eager and captured runs launch the same kernels.
    Elsewhere the torch path (the predicated loop while a stream is capturing).
    ``obj`` (B, n, m): B runs, indices (B, n_keep); a run whose non-dominated set is small fills by
    ``sig`` next to a run that truncates."""
    n = obj.shape[-2]
    n_keep = int(n_keep)
    batched = obj.dim() == 3 or _in_vmap(obj)
    if batched and obj.is_cuda:
        check_batched_caps(n, obj.shape[-1], "spea2.select")
        if n_keep < 1:
            raise NotImplementedError("spea2.select: batched runs need n_keep >= 1")
    elif batched:
        return _select_runs(obj, n_keep) if obj.dim() == 3 else _select_run(obj, n_keep)
    if batched or (obj.dim() == 2 and on_device(n, obj.shape[1], obj.device) and n_keep >= 1):
        o = obj.to(torch.float32).contiguous()
        out = _ext.ops().spea2_fitness(o)
        sig, mask = out[0], out[5]  # mask is sig < 1: a row no row dominates, without a NaN objective
        keep = _ext.ops().spea2_truncate(o, mask, n_keep, out[6], out[7])[0]
        key = torch.where(mask.sum(-1, keepdim=True) <= n_keep, sig, (~keep).to(sig.dtype))
        return torch.argsort(key, dim=-1, stable=True)[..., :n_keep]
    return _select_torch(obj, n_keep)
