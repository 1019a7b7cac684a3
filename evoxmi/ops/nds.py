"""Device non-dominated sort (``nds.hip``) and crowding distance."""
from __future__ import annotations

import torch

from . import _ext
from .. import config


def non_dominated_sort(f: torch.Tensor, until: int = 0) -> torch.Tensor:
    """Pareto ranks; with ``until`` > 0 fronts are peeled only until ≥ ``until`` rows are
    ranked and the remaining rows get rank ``n`` (larger than every real rank)."""
    f = f.to(torch.float32).contiguous()
    if f.shape[0] <= 65536 and f.shape[1] <= 8:
        try:
            rank = _ext.ops().nds(f, int(until), _ext.error_flag(f.device))
        except RuntimeError as e:
            if "co-resident" not in str(e):
                raise
        else:
            if config.get("debug") and not torch.cuda.is_current_stream_capturing():
                _ext.check_kernel_errors()
            return rank
    from ..operators.selection.non_dominate import _peel
    from ..utils.common import dominate_relation

    dom = dominate_relation(f, f)
    return _peel(dom, dom.sum(0).to(torch.int32))


def crowding_distance(costs: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Vectorised over objectives: one batched sort of the (m, n) masked keys."""
    n, m = costs.shape
    inf = torch.full((), float("inf"), device=costs.device, dtype=costs.dtype)  # fill kernel, not an H2D copy (capturable)
    nvalid = mask.sum()
    key = torch.where(mask[:, None], costs, inf).T  # (m, n)
    order = torch.argsort(key, dim=1, stable=True)
    sc = torch.gather(costs.T, 1, order)
    last = (nvalid - 1).clamp_min(0)
    rng = sc.gather(1, last.expand(m, 1)) - sc[:, :1]
    d = torch.empty((m, n), dtype=costs.dtype, device=costs.device)
    if n > 2:
        d.scatter_(1, order[:, 1:-1], (sc[:, 2:] - sc[:, :-2]) / rng)
    d.scatter_(1, order[:, :1], inf.expand(m, 1))
    d.scatter_(1, order.gather(1, last.expand(m, 1)), inf.expand(m, 1))
    dist = d.sum(0)
    return torch.where(mask, dist, -inf)


def nsga2_survivors(f: torch.Tensor, N: int, mask_pos: int, until: int = 0) -> torch.Tensor:
    """Indices of the N survivors of NSGA-II environmental selection (rank, then crowding
    distance on the front ``rank == sorted(rank)[mask_pos]``, lexsort order) — the fused
    ``nsga_select.hip`` kernel after the device non-dominated sort (n ≤ 8192).

    Identical to the torch path (``crowding_distance`` + lexsort) for finite objectives.  The
    kernel computes the crowding distance on the cut front alone; the torch path sorts all
    rows with the masked-out ones keyed ``+inf``, so the two differ when a cut-front row
    holds ``+inf`` (or NaN) while other rows are masked out."""
    f = f.to(torch.float32).contiguous()
    rank = non_dominated_sort(f, until)
    return _ext.ops().nsga_select(rank, f, int(N), int(mask_pos))


NICHE_SELECT_CAP = 8192  # nsga3_select.hip: one workgroup, n ≤ 8192 rows and R ≤ 8192 niches


def _lexsort(primary, secondary):
    """Order by (primary, secondary) ascending, stable."""
    o = torch.argsort(secondary, stable=True)
    return o[torch.argsort(primary[o], stable=True)]


def _nsga3_survivors_torch(rank, last_rank, group, group_dist, key, N: int, R: int) -> torch.Tensor:
    """``nsga3_survivors`` in fixed-shape torch: no host read, no data-dependent shape (the CPU
    oracle of the kernel and the capturable device path above its caps)."""
    from . import random as rnd

    n, dev = rank.shape[0], rank.device
    front = rank < last_rank
    last = rank == last_rank
    K = N - front.sum()
    g = group.clamp(0, R - 1)
    rho = torch.zeros(R, dtype=torch.int64, device=dev).scatter_add_(0, g, front.to(torch.int64))
    ordinal = (torch.cumsum(last, 0) - 1).clamp_min(0)  # position among the candidates
    u = rnd.uniform(key, (n,)).to(dev)[ordinal]  # the stream is prefix-stable: == uniform(key, (c,))
    inf = torch.full((), float("inf"), device=dev)
    # the closest member of an empty niche goes first
    big = torch.full((R,), float("inf"), device=dev).scatter_reduce(0, g, torch.where(last, group_dist, inf), "amin")
    first = last & (rho[g] == 0) & (group_dist == big[g])
    key_in = torch.where(first, torch.full_like(u, -1.0), u)
    gs = torch.where(last, g, torch.full_like(g, R))  # the other rows sort behind every niche
    o = _lexsort(gs, key_in)  # candidates ordered by (niche, key), then the rest
    g_o = gs[o]
    starts = torch.searchsorted(g_o, g_o, right=False)
    k = torch.arange(n, device=dev) - starts
    is_cand = g_o < R
    level = torch.where(is_cand, rho[g_o.clamp_max(R - 1)] + k, torch.full_like(k, n))
    pick = _lexsort(level, g_o)  # (level, niche) is unique per candidate
    chosen = torch.zeros(n, dtype=torch.bool, device=dev).scatter_(0, o[pick], (torch.arange(n, device=dev) < K) & is_cand[pick])
    keep = front | chosen
    return torch.argsort(~keep, stable=True)[:N]  # the kept rows, ascending


def nsga3_survivors(rank: torch.Tensor, last_rank: torch.Tensor, group: torch.Tensor, group_dist: torch.Tensor, key: torch.Tensor,
                    N: int, R: int) -> torch.Tensor:
    """Indices (ascending) of the N survivors of NSGA-III's niche-preserving selection.

    Rows with ``rank < last_rank`` survive; of the last front ``rank == last_rank`` the
    ``K = N − #front`` smallest ``(ρ_j + k, j)`` are kept, with ρ_j the number of surviving rows
    in niche ``j = group`` and ``k`` the position of a candidate inside its niche: the closest
    one (``group_dist``) first when the niche is empty, the rest in the random order of
    ``uniform(key)`` over the candidates.  ``last_rank`` is a 0-d tensor on the device of
    ``rank``: nothing is read on the host, so the call is capturable.  On a HIP device with
    n ≤ 8192 and R ≤ 8192 it is one launch of ``nsga3_select.hip``; otherwise fixed-shape torch.
    """
    N, R = int(N), int(R)
    n = rank.shape[0]
    group_dist = group_dist.to(torch.float32)
    if rank.is_cuda and n <= NICHE_SELECT_CAP and R <= NICHE_SELECT_CAP:
        return _ext.ops().nsga3_niche_select(rank.to(torch.int32).contiguous(), last_rank.to(torch.int32), group.to(torch.int64).contiguous(),
                                             group_dist.contiguous(), key.to(rank.device).contiguous(), N, R)
    return _nsga3_survivors_torch(rank, last_rank, group.to(torch.int64), group_dist, key, N, R)
