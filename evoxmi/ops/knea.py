"""KnEA's environmental selection: the knee points of every front up to the critical one and the cut of that front
(``knea_select.hip`` on a HIP device, the host loop ``knee_select_host`` elsewhere).

The kernel's contract.  All arithmetic is float64 on the float32 objectives, without FMA contraction.  With
``last = rank[N]``, for every front ``i = 0 … last``, its rows taken in position order:

1. extremes: ``mx_j``, ``mn_j`` the column max and min, ``e_j`` the *first* position that holds the column-j maximum;
2. plane: if the ``e_j`` are not m distinct positions, ``plane_j = 1 / max(E_jj, 1e-6)`` with ``E`` the matrix of the
   extreme rows; otherwise ``E·plane = 1`` by Gaussian elimination with partial pivoting (the first row on equal
   magnitudes), and the same fallback when a pivot is exactly 0 or a component of the result is not finite;
3. key: ``key = (float)(Σ_j obj_j·plane_j)``, summed in objective order in float64 and then rounded to float32.  The scan
   order is ascending ``(key, position)``, so the extremes (distance 1 ± rounding) tie at ``1.0f`` and scan in position
   order;
4. radius: ``r ← r·exp(−(1 − t / knee_rate) / m)``, ``R_j = (mx_j − mn_j)·r``;
5. scan: a row still marked when the scan reaches it is a knee; it unmarks every *other* row of the front with
   ``|obj_j − own_j| < R_j`` for all j;
6. ratio: ``t ← knees / front size``.

The cut: ``selected = rank < last | knee``, ``dif = |selected| − N``; ``dif > 0`` unselects ``dif`` knees of the last
front by descending key (the lower position first on equal keys), ``dif < 0`` selects the ``−dif`` non-knees of the last
front by ascending ``(key, position)``.  ``idx`` lists the N rows that remain, ascending.  NaN and infinite objectives
do not hang the kernel and leave ``idx`` N distinct positions in range; nothing more is promised for them.

The host path differs from that only in precision and in the order of exact key ties: it solves the plane with a
float32 LAPACK ``solve_ex``, takes a float32 ``exp``, and sorts the raw float32 dot product (so the m extremes of a
front, all at distance 1 ± rounding, are ordered by that rounding)."""
from __future__ import annotations

import torch

from . import _ext

N_CAP = 8192  # knea_select.hip: one workgroup, 8 rows per thread: n ≤ 8192 rows
M_CAP = 16  # knea_select.hip: m ≤ 16 objectives


def on_device(n: int, m: int, device) -> bool:
    """Whether n rows of m objectives on ``device`` run the kernel."""
    return torch.device(device).type == "cuda" and 2 <= n <= N_CAP and 1 <= m <= M_CAP


def _plane(points, m):
    sol, info = torch.linalg.solve_ex(points, torch.ones(m, 1, device=points.device))
    if int(info) == 0 and bool(torch.isfinite(sol).all()):
        return sol[:, 0]
    return 1.0 / torch.clamp(torch.diagonal(points), min=1e-6)


def knee_select_host(obj, rank, N, r, t, knee_rate):
    """The host loop (eager only): ``(idx, knee, r, t)`` with r and t Python floats."""
    m = obj.shape[1]
    last = int(rank[N])
    n = obj.shape[0]
    knee = torch.zeros(n, dtype=torch.bool, device=obj.device)
    r, t = float(r), float(t)
    plane = torch.ones(m, device=obj.device)
    for i in range(last + 1):
        idx = torch.nonzero(rank == i).flatten()
        f = obj[idx]
        mx, mn = f.max(0).values, f.min(0).values
        plane = _plane(f[torch.argmax(f, 0)], m)
        dist_order = idx[torch.argsort(f @ plane, stable=True)]
        r = r * float(torch.exp(torch.tensor(-(1 - t / knee_rate) / m)))
        R = (mx - mn) * r
        cand = torch.ones(n, dtype=torch.bool, device=obj.device)
        cand[idx] = True
        front_knee = torch.zeros(n, dtype=torch.bool, device=obj.device)
        front_knee[idx] = True
        for p in dist_order.tolist():
            if bool(front_knee[p]):
                nb = (torch.abs(obj[idx] - obj[p]) < R).all(1)
                nb_idx = idx[nb]
                front_knee[nb_idx] = False
                front_knee[p] = True
        knee |= front_knee
        t = float((front_knee[idx]).sum()) / idx.shape[0]
    knee &= rank <= last
    selected = (rank < last) | knee
    dif = int(selected.sum()) - N
    last_mask = rank == last
    if dif > 0:
        cand = torch.nonzero(knee & last_mask).flatten()
        far = cand[torch.argsort(-(obj[cand] @ plane), stable=True)][:dif]
        selected[far] = False
    elif dif < 0:
        cand = torch.nonzero(~knee & last_mask).flatten()
        near = cand[torch.argsort(obj[cand] @ plane, stable=True)][:-dif]
        selected[near] = True
    idx = torch.nonzero(selected).flatten()[:N]
    return idx, knee, r, t


def select(obj: torch.Tensor, rank: torch.Tensor, N: int, r, t, knee_rate: float):
    """``(idx, knee, r_out, t_out)``: ``idx`` (N,) int64 the ascending positions of the survivors among the rows of
    ``obj`` (n, m) float32, whose ``rank`` (n,) int32 or int64 is already sorted non-decreasing (``1 ≤ N < n``); ``knee``
    (n,) bool, False beyond the last front; ``r``, ``t`` the running radius factor and the knee ratio of the previous
    front, Python floats on the CPU, 0-dim float64 tensors on a device (new tensors are returned, the inputs are left
    as they are).  On a HIP device with n ≤ 8192 and m ≤ 16 one launch of ``knea_select.hip`` that reads nothing on the
    host; elsewhere ``knee_select_host``, a host loop."""
    N = int(N)
    dev = obj.device
    if obj.dim() == 2 and on_device(obj.shape[0], obj.shape[1], dev):
        as_word = lambda v: (v if isinstance(v, torch.Tensor) else torch.tensor(float(v))).to(device=dev, dtype=torch.float64)
        idx, knee, r_out, t_out = _ext.ops().knea_select(obj.to(torch.float32).contiguous(), rank.contiguous(), N, as_word(r), as_word(t),
                                                         float(knee_rate))
        return idx, knee, r_out, t_out
    idx, knee, r_out, t_out = knee_select_host(obj, rank, N, r, t, knee_rate)
    if dev.type != "cpu":
        r_out, t_out = (torch.tensor(v, dtype=torch.float64, device=dev) for v in (r_out, t_out))
    return idx, knee, r_out, t_out
