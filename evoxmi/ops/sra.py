"""SRA's environmental selection: the two indicators and their stochastic ranking
(``sra_select.hip`` on a HIP device, the host op and the torch expressions on the CPU)."""
from __future__ import annotations

import torch

from . import _ext
from ..utils.common import cal_max

RANK_CAP = 8192  # sra_select.hip, ranking: one workgroup, n ≤ 8192 rows
INDICATOR_M_CAP = 16  # sra_select.hip, indicators: m ≤ 16 objectives


def on_device(n: int, m: int, device) -> bool:
    """Whether a merged population of n rows and m objectives on ``device`` runs both kernels,
    so that nothing of its selection is read on the host."""
    return torch.device(device).type == "cuda" and n <= RANK_CAP and m <= INDICATOR_M_CAP


def sde_distance(obj):
    n = obj.shape[0]
    d = torch.sqrt((torch.clamp(obj[None, :, :] - obj[:, None, :], min=0) ** 2).sum(-1))  # d[i, j] = ‖max(o_j − o_i, 0)‖
    return d.masked_fill(torch.eye(n, dtype=torch.bool, device=obj.device), float("inf")).min(1).values


def indicators_dense(obj):
    I = cal_max(obj, obj)
    I1 = (-torch.exp(-I / 0.05)).sum(0) + 1
    I2 = sde_distance(obj)
    return I1, I2


def indicators(obj: torch.Tensor):
    """``(I1, I2)`` of the rows of ``obj`` (n, m): the I_ε+ fitness
    ``I1[p] = 1 − Σ_q exp(−max_k(o_qk − o_pk) / 0.05)`` and the shift-based density
    ``I2[p] = min_{q≠p} ‖max(o_q − o_p, 0)‖``.  On a HIP device with m ≤ 16 one launch of
    ``sra_select.hip`` forms both in a single pass without an (n, n, m) temporary; on the CPU and
    above the cap the dense torch expressions."""
    if obj.is_cuda and obj.dim() == 2 and obj.shape[1] <= INDICATOR_M_CAP:
        I1, I2 = _ext.ops().sra_indicators(obj.to(torch.float32).contiguous())
        return I1, I2
    return indicators_dense(obj)


def _stochastic_rank_host(I1, I2, u, pc):
    pc = float(pc)
    if _ext.available():
        return _ext.ops().stochastic_ranking(I1, I2, u, pc).to(I1.device)
    n = I1.shape[0]
    a, b, uu = I1.tolist(), I2.tolist(), u.tolist()
    r = list(range(n))
    for _ in range((n + 1) // 2):
        swapped = False
        for j in range(n - 1):
            k = a if uu[j] < pc else b
            if k[r[j]] < k[r[j + 1]]:
                r[j], r[j + 1] = r[j + 1], r[j]
                swapped = True
        if not swapped:
            break
    return torch.tensor(r, device=I1.device)


def stochastic_rank(I1: torch.Tensor, I2: torch.Tensor, u: torch.Tensor, pc) -> torch.Tensor:
    """The permutation (int64, best first) of stochastic ranking (Runarsson & Yao 2000): ⌈n/2⌉
    bubble sweeps in which position j compares by ``I1`` when ``u[j] < pc`` and by ``I2``
    otherwise, the larger value first.  ``pc`` is a Python float or a 0-d tensor.  On a HIP device
    with n ≤ 8192 it is one launch of ``sra_select.hip`` and ``pc`` stays a device word: nothing
    is read on the host, so the call is capturable.  CPU tensors, and HIP tensors above the cap,
    go through the host op ``evoxmi::stochastic_ranking`` (a host read)."""
    n = I1.shape[0]
    if I1.is_cuda and n <= RANK_CAP:
        dev = I1.device
        if isinstance(pc, torch.Tensor):
            pc = pc.to(device=dev, dtype=torch.float32)
        else:
            pc = torch.full((), float(pc), dtype=torch.float32, device=dev)  # a fill kernel, not an H2D copy
        return _ext.ops().sra_rank(I1.to(torch.float32).contiguous(), I2.to(dev, torch.float32).contiguous(),
                                   u.to(dev, torch.float32).contiguous(), pc)
    return _stochastic_rank_host(I1, I2, u, pc)
