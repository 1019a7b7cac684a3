"""Device non-dominated sort (``nds.hip``) and crowding distance."""
from __future__ import annotations

import torch

from . import _ext
from .. import config


BATCHED_NDS_CAP = 8192  # nds_batched.hip: one workgroup per run, n ≤ 8192 rows
NDS_MAX_M = 8  # the nds op's objective cap, single-run and batched


def _in_vmap(t: torch.Tensor) -> bool:
    return torch._C._functorch.is_batchedtensor(t)


def check_batched_caps(n: int, m: int, what: str = "non_dominated_sort") -> None:
    """The per-run caps of the batched device sort and selection; above them there is no batched
    kernel, and a run-by-run fallback would hide that."""
    if n > BATCHED_NDS_CAP or m > NDS_MAX_M:
        raise NotImplementedError(f"{what}: batched runs need n <= {BATCHED_NDS_CAP} rows and m <= {NDS_MAX_M} objectives per run, "
                                  f"got n = {n}, m = {m}")


def non_dominated_sort(f: torch.Tensor, until: int = 0) -> torch.Tensor:
    """Pareto ranks; with ``until`` > 0 fronts are peeled only until ≥ ``until`` rows are
    ranked and the remaining rows get rank ``n`` (larger than every real rank).

    ``f`` of shape (B, n, m) is B independent runs: ranks (B, n), row b being the 2-D call on
    ``f[b]`` (the stop is per run).  On a HIP device that is one launch of ``nds_batched.hip``,
    one workgroup per run (n ≤ 8192, m ≤ 8 per run); on the CPU the runs are ranked one by one."""
    if f.dim() == 3:
        if not f.is_cuda:
            from ..operators.selection.non_dominate import non_dominated_sort as nds_torch

            return nds_torch(f, until=until)
        check_batched_caps(f.shape[1], f.shape[2])
        return _ext.ops().nds(f.to(torch.float32).contiguous(), int(until), None)
    if f.is_cuda and _in_vmap(f):  # a run of a batch: the rule of ops/batching.py, which has no form above the caps
        check_batched_caps(f.shape[0], f.shape[1])
    f = f.to(torch.float32).contiguous()
    if f.shape[0] <= 65536 and f.shape[1] <= 8:
        try:
            rank = _ext.ops().nds(f, int(until), _ext.error_flag(f.device))
        except RuntimeError as e:
            if "co-resident" not in str(e):
                raise
        else:
            # the host check reads the error word: not under capture, and not under vmap (the batched kernel has no error path)
            if config.get("debug") and not torch.cuda.is_current_stream_capturing() and not _in_vmap(rank):
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
    holds ``+inf`` (or NaN) while other rows are masked out.

    ``f`` of shape (B, n, m) is B independent runs: survivors (B, N), row b being the 2-D call
    on ``f[b]``; two launches for all runs, one workgroup per run in each."""
    f = f.to(torch.float32).contiguous()
    if f.dim() == 3:
        check_batched_caps(f.shape[1], f.shape[2], "nsga2_survivors")
    rank = non_dominated_sort(f, until)
    return _ext.ops().nsga_select(rank, f, int(N), int(mask_pos))


def _survivors_torch(f: torch.Tensor, N: int, mask_pos: int, until: int) -> torch.Tensor:
    """The torch path of ``nsga2_survivors`` for one run: the CPU oracle, and the device path above
    the kernels' caps.  ``worst`` is read as a 0-d view (no host sync: capturable on a device)."""
    from ..operators.selection.non_dominate import crowding_distance as cd_any, lexsort, non_dominated_sort as nds_any

    rank = nds_any(f, until=until)
    worst = torch.sort(rank).values[mask_pos]
    cd = cd_any(f, rank == worst)
    return lexsort([-cd, rank.to(cd.dtype)])[:N]


@torch.library.custom_op("evoxmi_py::nsga2_survivors_runs", mutates_args=())
def _survivors_runs(f: torch.Tensor, N: int, mask_pos: int, until: int) -> torch.Tensor:
    """``_survivors_torch`` run by run on f (B, n, m) → (B, N): the torch path has data-dependent
    control flow on the CPU (the peel loop, the size of the cut front), so ``vmap`` cannot trace
    through it; this op is what a vmapped call reaches."""
    return torch.stack([_survivors_torch(fb, N, mask_pos, until) for fb in f])


@_survivors_runs.register_fake
def _(f, N, mask_pos, until):
    return f.new_empty((f.shape[0], N), dtype=torch.int64)


@torch.library.custom_op("evoxmi_py::nsga2_survivors_run", mutates_args=())
def _survivors_run(f: torch.Tensor, N: int, mask_pos: int, until: int) -> torch.Tensor:
    return _survivors_torch(f, N, mask_pos, until)


@_survivors_run.register_fake
def _(f, N, mask_pos, until):
    return f.new_empty((N,), dtype=torch.int64)


@torch.library.register_vmap("evoxmi_py::nsga2_survivors_run")
def _(info, in_dims, f, N, mask_pos, until):
    # sequential by construction: the oracle of the batched device kernels
    return _survivors_runs(f.movedim(in_dims[0], 0), N, mask_pos, until), 0


def nsga2_survivors_torch(f: torch.Tensor, N: int, mask_pos: int, until: int = 0) -> torch.Tensor:
    """``nsga2_survivors`` through the torch path (``crowding_distance`` + lexsort): the CPU
    implementation.  (B, n, m) input, or a call under ``vmap``, applies it run by run."""
    if f.dim() == 3:
        return _survivors_runs(f, int(N), int(mask_pos), int(until))
    if _in_vmap(f):
        if f.is_cuda:  # above the kernels' caps there is no batched device form
            check_batched_caps(f.shape[0], f.shape[1], "nsga2_survivors")
        return _survivors_run(f, int(N), int(mask_pos), int(until))
    return _survivors_torch(f, N, mask_pos, until)


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
