"""BCE-IBEA's PC selection and exploration: the niche radius of the non-dominated set, its one-by-one
truncation by niche score, and the under-populated PC members (``bce_select.hip`` on a HIP device, the
torch expressions on the CPU).

The kernels' contract, where it is sharper than the torch path's: the mask is the rows no row dominates;
``span_k = max(f_max_k − f_min_k, 1e-12)`` over the masked rows; ``d2`` is the float32 sum, with ``fmaf``
over the objectives in ascending order, of the squares of ``δ_k = (f_ik − f_jk) / span_k`` — the difference
first, normalising first cancels for close neighbours — and a NaN counts as +inf; ``t_i`` is the square
root of the third smallest ``d2`` to the other masked rows and ``r`` their mean, summed in the fixed order
stated in the kernel file; ``R(i, j) = min(sqrt(d2) / r, 1)`` and ``P_j`` their product over the live masked
rows in a fixed order; ``max(0, n_nd − n_keep)`` times the live masked row of greatest ``(1 − P_j, lowest
index)`` leaves, a NaN score counting as greatest (``torch.argmax``'s rule) — compared as the least ``P_j``, so
that products below 2⁻²⁵ are still told apart."""
from __future__ import annotations

import torch

from . import _ext

N_CAP = 8192  # bce_select.hip, removal: one workgroup, n ≤ 8192 rows
M_CAP = 16  # bce_select.hip, every kernel: m ≤ 16 objectives


def on_device(n: int, m: int, device) -> bool:
    """Whether n rows of m objectives on ``device`` run the kernels."""
    return torch.device(device).type == "cuda" and 3 <= n <= N_CAP and 1 <= m <= M_CAP


# ---------------------------------------------------------------- the torch path and the kernels' oracle
def exploration(pc_obj, npc_obj, n_nd, n):
    f_max, f_min = pc_obj.max(0).values, pc_obj.min(0).values
    span = (f_max - f_min).clamp(min=1e-12)
    npc_n = (npc_obj - f_min) / span
    pc_n = (pc_obj - f_min) / span
    d = torch.cdist(pc_n, pc_n).masked_fill(torch.eye(pc_n.shape[0], dtype=torch.bool, device=pc_obj.device), float("inf"))
    d = torch.nan_to_num(d, nan=float("inf"))
    sd = torch.sort(d, 1).values
    r0 = sd[:, min(2, sd.shape[1] - 1)].mean()
    r = n_nd / n * r0
    return (torch.cdist(pc_n, npc_n) <= r).sum(1) <= 1


def _niche(f):
    """The pairwise distances of the normalised rows of ``f`` (+inf on the diagonal) and their sort."""
    n = f.shape[0]
    f_max, f_min = f.max(0).values, f.min(0).values
    norm = (f - f_min) / (f_max - f_min).clamp(min=1e-12)
    d = torch.cdist(norm, norm).masked_fill(torch.eye(n, dtype=torch.bool, device=f.device), float("inf"))
    return d, torch.sort(d, 1).values


def pc_selection_indices(pc_obj, n, order=None):
    """``(idx, n_nd)`` of the reference PC selection: the non-dominated rows of ``pc_obj``, truncated one by
    one to ``n`` by niche score, or padded with the first of them (``order`` collects the removed rows)."""
    from ..operators.selection.non_dominate import non_dominated_sort

    rank = non_dominated_sort(pc_obj)
    mask = rank == 0
    n_nd = int(mask.sum())
    if n_nd > n:
        d, sd = _niche(pc_obj[mask])
        r = sd[:, min(2, n_nd - 1)].sum() / n_nd
        R = torch.clamp(d / r, max=1)
        keep = torch.ones(n_nd, dtype=torch.bool, device=pc_obj.device)
        rows = torch.nonzero(mask).flatten()
        for _ in range(n_nd - n):
            score = torch.where(keep, 1 - torch.prod(R, 0), torch.full((n_nd,), -1.0, device=R.device))
            i = int(torch.argmax(score))
            if order is not None:
                order.append(int(rows[i]))
            keep[i] = False
            R[i, :] = 1
            R[:, i] = 1
        idx = rows[keep]
    else:
        idx = torch.nonzero(mask).flatten()
        idx = torch.cat([idx, idx[:1].expand(n - idx.shape[0])])  # pad with the first member
    return idx, n_nd


# ---------------------------------------------------------------- public entries
def niche_radius(obj: torch.Tensor, mask: torch.Tensor = None):
    """``(r, t)``: ``t_i`` the distance of masked row ``i`` of ``obj`` (n, m) to its third nearest masked
    neighbour on the objectives normalised by the masked rows' spans (0 outside the mask), and ``r`` their
    mean over the mask (every row without a mask).  On a HIP device within the caps three launches of
    ``bce_select.hip``; elsewhere the torch expressions."""
    n = obj.shape[0]
    if obj.dim() == 2 and on_device(n, obj.shape[1], obj.device):
        t, ws, _ = _ext.ops().bce_niche(obj.to(torch.float32).contiguous(), None if mask is None else mask.contiguous())
        return ws[-1], t
    rows = torch.arange(n, device=obj.device) if mask is None else torch.nonzero(mask).flatten()
    _, sd = _niche(obj[rows])
    tm = sd[:, min(2, rows.shape[0] - 1)]
    t = torch.zeros(n, dtype=tm.dtype, device=obj.device)
    t[rows] = tm
    return tm.sum() / rows.shape[0], t


def pc_select(obj: torch.Tensor, n_keep: int, return_order: bool = False, mask: torch.Tensor = None):
    """BCE's PC selection over the rows of ``obj`` (n, m): ``(idx, n_nd)`` with ``n_nd`` (0-d int64) the
    number of rows no row dominates and ``idx`` (int64, (n_keep,)) those rows in ascending order after
    ``max(0, n_nd − n_keep)`` removals by niche score, padded with the first of them where ``n_nd ≤ n_keep``.
    With ``return_order`` also the removed rows in the order of their removal, padded with −1 to
    ``n − n_keep`` entries, and the number of rescanned rows (int32; 0 on the torch path).  ``mask`` replaces
    the non-dominated set (device path only).  On a HIP device with 3 ≤ n ≤ 8192, m ≤ 16 and n_keep ≥ 2 the
    kernels of ``bce_select.hip`` and a stable argsort: nothing is read on the host, eager and captured runs
    launch the same kernels.  Elsewhere ``pc_selection_indices``."""
    n = obj.shape[0]
    n_keep = int(n_keep)
    dev = obj.device
    if obj.dim() == 2 and on_device(n, obj.shape[1], dev) and n_keep >= 2:
        keep, order, stats, n_nd = _ext.ops().bce_pc_select(obj.to(torch.float32).contiguous(), n_keep,
                                                            None if mask is None else mask.contiguous())[:4]
        by_keep = torch.argsort((~keep).to(torch.int8), stable=True)  # the kept rows, ascending, come first
        if n_keep > n:
            by_keep = torch.cat([by_keep, by_keep[:1].expand(n_keep - n)])
        kept = torch.clamp(n_nd, max=n_keep)
        idx = torch.where(torch.arange(n_keep, device=dev) < kept, by_keep[:n_keep], by_keep[0])
        return (idx, n_nd, order, stats[0]) if return_order else (idx, n_nd)
    if mask is not None:
        raise ValueError("pc_select: a caller's mask needs the device path")
    xs = []
    idx, n_nd = pc_selection_indices(obj, n_keep, xs)
    n_nd = torch.tensor(n_nd, dtype=torch.int64, device=dev)
    if not return_order:
        return idx, n_nd
    order = torch.full((max(n - n_keep, 0),), -1, dtype=torch.int64, device=dev)
    if xs:
        order[: len(xs)] = torch.tensor(xs, dtype=torch.int64, device=dev)
    return idx, n_nd, order, torch.zeros((), dtype=torch.int32, device=dev)


def explore(pc_obj: torch.Tensor, npc_obj: torch.Tensor, n_nd, n: int):
    """Bool (N,): the rows of ``pc_obj`` with at most one row of ``npc_obj`` within ``n_nd / n`` times the
    mean niche radius of ``pc_obj``, on ``pc_obj``'s normalisation.  On a HIP device within the caps four
    launches of ``bce_select.hip`` with ``n_nd`` read from device memory (``n`` is the row count of
    ``pc_obj``); elsewhere ``exploration``."""
    N = pc_obj.shape[0]
    if (pc_obj.dim() == 2 and on_device(N, pc_obj.shape[1], pc_obj.device) and int(n) == N and npc_obj.dim() == 2
            and 1 <= npc_obj.shape[0] <= N_CAP and npc_obj.shape[1] == pc_obj.shape[1]):
        if not isinstance(n_nd, torch.Tensor):
            n_nd = torch.tensor(int(n_nd), dtype=torch.int64, device=pc_obj.device)
        return _ext.ops().bce_explore(pc_obj.to(torch.float32).contiguous(), npc_obj.to(torch.float32).contiguous(),
                                      n_nd.to(torch.int64).reshape(1))
    return exploration(pc_obj, npc_obj, n_nd, n)
