"""MOEA/D-M2M's association: every one of K regions keeps S of the rows assigned to it, chosen by an NSGA-II
selection among them (``m2m_select.hip`` on a HIP device, the torch loop of
``algorithms.mo.moeadm2m.association_indices`` elsewhere).

The kernel's contract: region ``k`` with ``c`` members and ``c < S`` gives the member rows ascending, then
``rad[c:S]``; with ``c ≥ S`` the fronts of its members are peeled until ``S`` of them are ranked, the members of the
ranks before the last (``worst``) come first in (rank, row) order, the rest are the last front's members by
(−crowding distance, row), the distance taken on that front alone in float32: per objective a stable sort, the
extremes +inf, an interior row ``(next − prev) / (last − first)``, the terms added in objective order.  For finite
objectives that is index for index what the CPU torch path returns."""
from __future__ import annotations

import torch

from . import _ext

N_CAP = 8192  # m2m_select.hip: one workgroup per region, a region may hold every row: n ≤ 8192 rows
M_CAP = 16  # m2m_select.hip: m ≤ 16 objectives
K_CAP = 1024  # m2m_select.hip: K ≤ 1024 regions


def on_device(n: int, m: int, K: int, device) -> bool:
    """Whether n rows of m objectives in K regions on ``device`` run the kernel."""
    return torch.device(device).type == "cuda" and 1 <= n <= N_CAP and 1 <= m <= M_CAP and 1 <= K <= K_CAP


def _info(obj, region, K, S):
    """``(counts, worst)`` of the torch path: the region sizes and the rank of the front that holds a region's
    S-th member (−1 where the region has fewer than S)."""
    from ..utils.common import dominate_relation

    counts = torch.bincount(region, minlength=K)[:K]
    worst = torch.full((K,), -1, dtype=torch.int32, device=obj.device)
    for k in range(K):
        if int(counts[k]) < S:
            continue
        o = obj[region == k]
        dom = dominate_relation(o, o)
        left = torch.ones(o.shape[0], dtype=torch.bool, device=obj.device)
        r = -1
        while int(left.sum()) > o.shape[0] - S:  # peel until S members are ranked
            left &= (dom & left[:, None]).sum(0) != 0
            r += 1
        worst[k] = r
    return counts.to(torch.int32), worst


def select(obj: torch.Tensor, region: torch.Tensor, rad: torch.Tensor, K: int, S: int, return_info: bool = False):
    """``part`` (K·S,) int64, region-major: ``part[k·S + j]`` is the j-th chosen row of region k among the rows of
    ``obj`` (n, m) whose ``region`` (n,) is k; ``rad`` (S,) int64 are the rows that pad a region of fewer than S
    members.  With ``return_info`` also ``counts`` (K,) int32, the region sizes, and ``worst`` (K,) int32, the rank of
    the cut front (−1 where the region was padded).  On a HIP device with n ≤ 8192, m ≤ 16 and K ≤ 1024 one launch
    of ``m2m_select.hip`` that reads nothing on the host; elsewhere ``association_indices``, a host loop."""
    K, S = int(K), int(S)
    if obj.dim() == 2 and on_device(obj.shape[0], obj.shape[1], K, obj.device):
        part, counts, worst = _ext.ops().m2m_select(obj.to(torch.float32).contiguous(), region.contiguous(), rad.contiguous(), K, S)
        return (part, counts, worst) if return_info else part
    from ..algorithms.mo.moeadm2m import association_indices

    part = association_indices(obj, region, rad, K, S)
    return (part, *_info(obj, region, K, S)) if return_info else part
