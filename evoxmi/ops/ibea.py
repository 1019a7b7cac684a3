"""IBEA's environmental selection: the I_ε+ fitness and the one-by-one truncation with its
fitness correction (``ibea_select.hip`` on a HIP device, the torch expressions on the CPU).

``fitness`` and ``select`` take ``obj`` (B, n, m) as B independent runs: row b of every output is
the 2-D call on ``obj[b]``, bit for bit.  On a HIP device that is the same two launches with the run
on the grid (a workgroup per run in the removal kernel); on the CPU the runs are done one by one.
Under ``vmap`` (``BatchedRuns``) the device calls reach the same batched launches through the rules
of ``ops/batching.py``; a per-run shape above the caps then raises ``NotImplementedError`` instead
of running the dense torch path for every run."""
from __future__ import annotations

import torch

from . import _ext
from .nds import _in_vmap
from ..utils.common import cal_max

N_CAP = 8192  # ibea_select.hip, truncation: one workgroup, n ≤ 8192 rows
M_CAP = 16  # ibea_select.hip, both kernels: m ≤ 16 objectives


def on_device(n: int, m: int, device) -> bool:
    """Whether a merged population of n rows and m objectives on ``device`` runs both kernels."""
    return torch.device(device).type == "cuda" and 1 <= n <= N_CAP and 1 <= m <= M_CAP


def check_batched_caps(n: int, m: int, what: str, need_rows: bool = True) -> None:
    """The per-run caps of the kernels; above them there is no batched form, and the dense torch
    path for every run would hide that."""
    if m < 1 or m > M_CAP or (need_rows and (n < 1 or n > N_CAP)):
        raise NotImplementedError(f"{what}: batched runs need 1 <= n <= {N_CAP} rows (the truncation) and 1 <= m <= {M_CAP} "
                                  f"objectives per run, got n = {n}, m = {m}")


def normalise(pop_obj):
    # the reference normalises by the scalar min/max over *all* objectives (ibea.py:23-26); (B, n, m): per run
    if pop_obj.dim() == 3:
        mn, mx = pop_obj.amin((1, 2), keepdim=True), pop_obj.amax((1, 2), keepdim=True)
    else:
        mn, mx = pop_obj.min(), pop_obj.max()
    return (pop_obj - mn) / (mx - mn)


def cal_fitness(pop_obj, kappa):
    """The dense torch path (CPU, above the caps, and the oracle of the kernels):
    ``(fitness, I, C)`` with the full (n, n) indicator matrix ``I``."""
    obj = normalise(pop_obj)
    I = cal_max(obj, obj)
    C = torch.abs(I).max(0).values
    fitness = (-torch.exp(-I / C[None, :] / kappa)).sum(0) + 1
    return fitness, I, C


def _truncate(fitness, I, C, kappa, n_remove):
    f = fitness.clone()
    removed = torch.zeros_like(f, dtype=torch.bool)
    xs = []
    for _ in range(n_remove):
        x = torch.argmin(f)
        row = I.index_select(0, x.reshape(1))[0]
        cx = C.index_select(0, x.reshape(1))[0]
        f = f + torch.exp(-row / cx / kappa)
        f = f.scatter(0, x.reshape(1), f.max().reshape(1))
        removed = removed.scatter(0, x.reshape(1), torch.ones(1, dtype=torch.bool, device=f.device))
        xs.append(x)
    return ~removed, xs


def ibea_truncate(fitness, I, C, kappa, n_remove):
    """Remove ``n_remove`` individuals one by one; returns the survivor mask."""
    return _truncate(fitness, I, C, kappa, n_remove)[0]


def fitness(obj: torch.Tensor, kappa):
    """``(f, C)`` of the rows of ``obj`` (n, m): with o the objectives normalised by their scalar
    min and max and ``I[i, j] = max_k(o_ik − o_jk)``, ``C[j] = max_i |I[i, j]|`` and
    ``f[j] = 1 − Σ_i exp(−I[i, j] / C[j] / κ)``.  On a HIP device with m ≤ 16 one launch of
    ``ibea_select.hip`` without an (n, n) or (n, n, m) temporary; on the CPU and above the cap the
    dense torch expressions.  ``obj`` (B, n, m): B runs, ``f`` and ``C`` (B, n)."""
    if obj.dim() == 3:
        if not obj.is_cuda:
            f, C = zip(*(fitness(o, kappa) for o in obj))
            return torch.stack(f), torch.stack(C)
        check_batched_caps(obj.shape[1], obj.shape[2], "ibea.fitness", need_rows=False)
        f, C = _ext.ops().ibea_fitness(normalise(obj).to(torch.float32).contiguous(), float(kappa))
        return f, C
    if obj.is_cuda and _in_vmap(obj):
        check_batched_caps(obj.shape[0], obj.shape[1], "ibea.fitness", need_rows=False)
    if obj.is_cuda and obj.dim() == 2 and obj.shape[0] >= 1 and 1 <= obj.shape[1] <= M_CAP:
        f, C = _ext.ops().ibea_fitness(normalise(obj).to(torch.float32).contiguous(), float(kappa))
        return f, C
    f, _, C = cal_fitness(obj, kappa)
    return f, C


def select(obj: torch.Tensor, kappa, n_keep: int, return_order: bool = False):
    """The rows (int64, ascending) that IBEA's truncation of ``obj`` (n, m) keeps: ``n − n_keep``
    times the row of least fitness is removed and every fitness corrected by its indicator
    against that row.  With ``return_order`` also the removed rows in the order of their removal.
    On a HIP device with n ≤ 8192 and m ≤ 16 it is the normalisation and two launches of
    ``ibea_select.hip``; on the CPU and above the caps ``cal_fitness``, ``ibea_truncate`` and a
    stable argsort of the survivor mask.  Nothing is read on the host on either path.
    ``obj`` (B, n, m): B runs, the rows (B, n_keep) and the order (B, n − n_keep)."""
    n = obj.shape[-2]
    n_keep = int(n_keep)
    dev = obj.device
    if obj.dim() == 3:
        B = obj.shape[0]
        if n == 0 or n_keep >= n:
            idx = torch.arange(n, device=dev)[:n_keep].expand(B, -1).contiguous()
            return (idx, torch.zeros((B, 0), dtype=torch.int64, device=dev)) if return_order else idx
        if not obj.is_cuda:
            idx, order = zip(*(select(o, kappa, n_keep, return_order=True) for o in obj))
            return (torch.stack(idx), torch.stack(order)) if return_order else torch.stack(idx)
        check_batched_caps(n, obj.shape[2], "ibea.select")
        o = normalise(obj).to(torch.float32).contiguous()
        f, C = _ext.ops().ibea_fitness(o, float(kappa))
        idx, order = _ext.ops().ibea_truncate(o, f, C, float(kappa), n - n_keep, n_keep)
        return (idx, order) if return_order else idx
    if n == 0 or n_keep >= n:
        idx = torch.arange(n, device=dev)[:n_keep]
        return (idx, torch.zeros(0, dtype=torch.int64, device=dev)) if return_order else idx
    if obj.is_cuda and _in_vmap(obj):
        check_batched_caps(n, obj.shape[1], "ibea.select")
    if obj.dim() == 2 and on_device(n, obj.shape[1], dev):
        o = normalise(obj).to(torch.float32).contiguous()
        f, C = _ext.ops().ibea_fitness(o, float(kappa))
        idx, order = _ext.ops().ibea_truncate(o, f, C, float(kappa), n - n_keep, n_keep)
        return (idx, order) if return_order else idx
    f, I, C = cal_fitness(obj, kappa)
    keep, xs = _truncate(f, I, C, kappa, n - n_keep)
    idx = torch.argsort((~keep).to(torch.int64), stable=True)[:n_keep]
    return (idx, torch.stack(xs)) if return_order else idx
