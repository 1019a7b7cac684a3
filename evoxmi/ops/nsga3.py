"""NSGA-III's normalisation and association: the steps of ``NSGA3.tell`` between the non-dominated sort and the
niche-preserving selection (``ops.nds.nsga3_survivors``).

``associate(f, rank, ref, N)`` returns ``(last_rank, group, group_dist, scale)`` for the merged objectives ``f`` (n, m),
their Pareto ranks and the reference points ``ref`` (K, m), N < n being the number of survivors:

1. ``last_rank``: the rank at sorted position N, i.e. the smallest r with #{rank ≤ r} > N; ``valid = rank ≤ last_rank``;
2. ``ideal``: the column minimum over the valid rows;
3. for every axis j the first valid row that minimises ``max_k (f_k − ideal_k) / (δ_jk + 1e-6)``;
4. ``worst``: the column maximum of ``f − ideal`` over the valid rows;
5. ``E·x = 1`` over the m extreme rows (minus ideal), ``intercept = 1 / x``; ``nadir = intercept`` when the system was
   not singular and every intercept is finite and > 1e-6, else ``nadir = worst``; ``scale = (ideal, nadir)`` (2, m);
6. with ``x = (f − ideal) / nadir`` and ŵ the reference points scaled to unit length, ``group`` is the reference
   point of the smallest perpendicular distance ``|x|·sqrt(1 − cos²)`` (the lowest position on equal distances) and
   ``group_dist`` that distance.  A row with ``|x| = 0`` or a non-finite entry gets ``(0, NaN)``.

On a HIP device with n ≤ 8192, m ≤ 16 and K ≤ 8192 these are the three launches of ``nsga3_assoc.hip``: float64
arithmetic on the float32 inputs without contraction, Gaussian elimination with partial pivoting for step 5, and
``d² = max(|x|² − (x·ŵ)², 0)`` with one square root per row for step 6 (``|x|²`` and ``x·ŵ`` summed in objective order);
no (n, K) array exists.  Elsewhere (the CPU, a device above the caps) the float32 torch expressions that ``NSGA3.tell``
always used are evaluated; the two agree to float32 rounding, and can associate a row differently only where two
reference lines are nearly equidistant from it.

``f`` (B, n, m) with ``rank`` (B, n) is B independent runs that share ``ref``: every output gains the run axis, and
row b is the 2-D call on run b bit for bit (the same launches, one workgroup or one grid row per run).  Under ``vmap``
(``BatchedRuns``) device calls reach those launches through the rules of ``ops/batching.py``; a per-run shape above a
cap then raises ``NotImplementedError``.  On the CPU the torch path has data-dependent control flow (the peel loop of
the sort), so under ``vmap`` the whole selection of a tell goes run by run through ``survivors_run``."""
from __future__ import annotations

import torch

from . import _ext
from .nds import _in_vmap
from ..utils.common import cos_dist

N_CAP = 8192  # nsga3_assoc.hip: one workgroup normalises a run, n ≤ 8192 rows
K_CAP = 8192  # reference points (nsga3_select.hip keeps a word per niche in LDS)
M_CAP = 16  # objectives


def on_device(n: int, m: int, K: int, N: int, device) -> bool:
    """Whether (n, m) objectives against K reference points on ``device`` run the kernels."""
    return torch.device(device).type == "cuda" and 1 <= n <= N_CAP and 1 <= m <= M_CAP and 1 <= K <= K_CAP and 0 <= N < n


def check_batched_caps(n: int, m: int, K: int, what: str) -> None:
    """The per-run caps of the kernels; above them there is no batched form, and the torch path for every run would
    hide that."""
    if n < 1 or n > N_CAP or m < 1 or m > M_CAP or K < 1 or K > K_CAP:
        raise NotImplementedError(f"{what}: batched runs need 1 <= n <= {N_CAP} rows, 1 <= m <= {M_CAP} objectives and "
                                  f"1 <= K <= {K_CAP} reference points per run, got n = {n}, m = {m}, K = {K}")


def _associate_torch(f, rank, ref, N: int):
    """The torch path for one run: the expressions of ``NSGA3.tell`` (no host read: capturable on a device)."""
    m = f.shape[1]
    last_rank = torch.sort(rank).values[N]  # 0-d view: no host sync (capturable)
    valid = rank <= last_rank
    inf = torch.full_like(f, float("inf"))
    ideal = torch.where(valid[:, None], f, inf).min(0).values
    Fn = f - ideal
    weight = torch.eye(m, device=Fn.device) + 1e-6
    asf = (Fn[None, :, :] / weight[:, None, :]).amax(-1)  # (m, n)
    asf = torch.where(valid[None, :], asf, torch.full_like(asf, float("inf")))
    extreme = Fn[torch.argmin(asf, 1)]
    sol, info = torch.linalg.solve_ex(extreme, torch.ones(m, 1, device=Fn.device))
    intercept = 1.0 / sol[:, 0]
    worst = torch.where(valid[:, None], Fn, -inf).max(0).values
    ok = (info == 0) & torch.isfinite(intercept).all() & (intercept > 1e-6).all()
    nadir = torch.where(ok, intercept, worst)
    Fn = Fn / nadir
    cosine = cos_dist(Fn, ref).clamp(-1, 1)
    dist = torch.linalg.norm(Fn, dim=-1, keepdim=True) * torch.sqrt(torch.clamp(1 - cosine**2, min=0))
    group_dist, group = dist.min(1)
    return last_rank, group, group_dist, torch.stack([ideal, nadir]).to(torch.float64)


def associate(f: torch.Tensor, rank: torch.Tensor, ref: torch.Tensor, N: int):
    """``(last_rank, group, group_dist, scale)``: see the module docstring.  ``last_rank`` is a 0-d tensor on the device
    of ``f`` (int32 from the kernels, the dtype of ``rank`` from the torch path), ``group`` int64, ``group_dist``
    float32, ``scale`` float64 (2, m); with ``f`` (B, n, m) each has the leading run axis."""
    N = int(N)
    K = ref.shape[0]
    if f.dim() == 3:
        if not f.is_cuda:
            out = [_associate_torch(fb, rb, ref, N) for fb, rb in zip(f, rank)]
            return tuple(torch.stack(o) for o in zip(*out))
        check_batched_caps(f.shape[1], f.shape[2], K, "nsga3.associate")
    elif f.is_cuda and _in_vmap(f):
        check_batched_caps(f.shape[0], f.shape[1], K, "nsga3.associate")
    if on_device(f.shape[-2], f.shape[-1], K, N, f.device):
        return tuple(_ext.ops().nsga3_associate(f.to(torch.float32).contiguous(), rank.to(torch.int32).contiguous(),
                                                ref.to(torch.float32).contiguous(), N))
    return _associate_torch(f, rank, ref, N)


def _survivors_torch(f, key, ref, N: int) -> torch.Tensor:
    """Sort, association and niche selection of one run in torch: what ``NSGA3.tell`` computes on the CPU."""
    from ..operators.selection.non_dominate import non_dominated_sort
    from .nds import _nsga3_survivors_torch

    rank = non_dominated_sort(f, until=N + 1)
    last_rank, group, group_dist, _ = _associate_torch(f, rank, ref, N)
    return _nsga3_survivors_torch(rank, last_rank, group, group_dist.to(torch.float32), key, N, ref.shape[0])


@torch.library.custom_op("evoxmi_py::nsga3_survivors_runs", mutates_args=())
def _survivors_runs(f: torch.Tensor, key: torch.Tensor, ref: torch.Tensor, N: int) -> torch.Tensor:
    """``_survivors_torch`` run by run on f (B, n, m), key (B, 2) → (B, N): what a vmapped CPU tell reaches (``vmap``
    cannot trace the peel loop of the sort)."""
    return torch.stack([_survivors_torch(fb, kb, ref, N) for fb, kb in zip(f, key)])


@_survivors_runs.register_fake
def _(f, key, ref, N):
    return f.new_empty((f.shape[0], N), dtype=torch.int64)


@torch.library.custom_op("evoxmi_py::nsga3_survivors_run", mutates_args=())
def survivors_run(f: torch.Tensor, key: torch.Tensor, ref: torch.Tensor, N: int) -> torch.Tensor:
    return _survivors_torch(f, key, ref, N)


@survivors_run.register_fake
def _(f, key, ref, N):
    return f.new_empty((N,), dtype=torch.int64)


@torch.library.register_vmap("evoxmi_py::nsga3_survivors_run")
def _(info, in_dims, f, key, ref, N):
    # sequential by construction: the oracle of the batched device kernels
    if in_dims[2] is not None:
        raise NotImplementedError("nsga3_survivors_run vmap rule: the reference points must be shared by all runs")
    B = info.batch_size
    fb = f.movedim(in_dims[0], 0) if in_dims[0] is not None else f.unsqueeze(0).expand((B,) + tuple(f.shape))
    kb = key.movedim(in_dims[1], 0) if in_dims[1] is not None else key.unsqueeze(0).expand(B, -1)
    return _survivors_runs(fb.contiguous(), kb.contiguous(), ref, N), 0
