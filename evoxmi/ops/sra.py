"""SRA's environmental selection: the two indicators and their stochastic ranking
(``sra_select.hip`` on a HIP device, the host op and the torch expressions on the CPU).

``select`` does both.  On ``obj`` (B, n, m), and as ``sra_select`` under ``vmap`` (``evoxmi/ops/batching.py``), it selects for B
independent runs in ONE launch of ``sra_small.hip``: a workgroup per run stages the run's rows in LDS, forms I1 and I2 in the
summation order of the solo kernel (``csrc/include/evoxmi_sra.h`` holds the arithmetic for both files), and ranks them without
writing them to global memory in between.  Every run gets the words of the 2-D call.  Its caps per run are ``N_SMALL_CAP`` rows at
up to 8 objectives and half that at up to 16; above them it raises, it does not go run by run."""
from __future__ import annotations

import torch

from . import _ext
from ..utils.common import cal_max

RANK_CAP = 8192  # sra_select.hip, ranking: one workgroup, n ≤ 8192 rows
INDICATOR_M_CAP = 16  # sra_select.hip, indicators: m ≤ 16 objectives
N_SMALL_CAP = 2048  # sra_small.hip, a workgroup per run: n ≤ 2048 rows at m ≤ 8, n ≤ 1024 at m ≤ 16


def small_ok(n: int, m: int) -> bool:
    """Whether runs of n rows and m objectives fit the one-workgroup-per-run kernel."""
    return n >= 1 and m >= 1 and ((m <= 8 and n <= N_SMALL_CAP) or (m <= INDICATOR_M_CAP and n <= N_SMALL_CAP // 2))


def check_small_caps(n: int, m: int, what: str):
    if not small_ok(n, m):
        raise NotImplementedError(f"{what}: batched runs need 1 <= n <= {N_SMALL_CAP} rows at m <= 8 objectives or n <= {N_SMALL_CAP // 2} "
                                  f"at m <= {INDICATOR_M_CAP} per run, got n = {n}, m = {m}")


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


def _pc_word(pc, dev):
    if isinstance(pc, torch.Tensor):
        return pc.to(device=dev, dtype=torch.float32)
    return torch.full((), float(pc), dtype=torch.float32, device=dev)  # a fill kernel, not an H2D copy


def _select_runs(obj, u, pc, return_info):
    B, n, m = obj.shape
    if obj.is_cuda:
        check_small_caps(n, m, "ops.sra.select")
        out = _ext.ops().sra_small_select(obj.to(torch.float32).contiguous(), u.to(obj.device, torch.float32).contiguous(),
                                          _pc_word(pc, obj.device).expand(B).contiguous())
    else:
        pcs = pc.expand(B) if isinstance(pc, torch.Tensor) else [pc] * B
        out = [torch.stack(t) for t in zip(*(select(obj[r], u[r], pcs[r], True) for r in range(B)))]
    return tuple(out) if return_info else out[0]


def select(obj: torch.Tensor, u: torch.Tensor, pc, return_info: bool = False):
    """The permutation (n,) int64, best first, of SRA's selection of the rows ``obj`` (n, m): ``indicators`` and then
    ``stochastic_rank`` with the draws ``u`` (n − 1,) and ``pc``, a Python float or a 0-d tensor; ``return_info`` gives
    ``(idx, I1, I2)``.  On a HIP device within the caps of ``on_device`` it is the two launches of ``sra_select.hip`` and reads
    nothing on the host; elsewhere the dense torch expressions and ``stochastic_rank``, on the CPU the host op.

    ``obj`` (B, n, m) selects for B independent runs: ``u`` is (B, n − 1), ``pc`` a float, a 0-d tensor or (B,), and every result
    gains a leading run axis.  On a HIP device that is ONE launch of ``sra_small.hip``, a workgroup per run, whose words are those
    of the 2-D call on each run; runs above its caps (``small_ok``) raise ``NotImplementedError``.  On the CPU the 2-D path runs
    run by run."""
    if obj.dim() == 3:
        return _select_runs(obj, u, pc, return_info)
    n, m = obj.shape
    if on_device(n, m, obj.device):
        dev = obj.device
        idx, I1, I2 = _ext.ops().sra_select(obj.to(torch.float32).contiguous(), u.to(dev, torch.float32).contiguous(), _pc_word(pc, dev))
    else:
        I1, I2 = indicators_dense(obj)
        idx = stochastic_rank(I1, I2, u, pc)
    return (idx, I1, I2) if return_info else idx


@torch.library.custom_op("evoxmi_py::sra_select_runs", mutates_args=())
def _select_draw_runs(obj: torch.Tensor, u: torch.Tensor, draw: torch.Tensor) -> torch.Tensor:
    """The CPU selection of SRA run by run on obj (B, n, m), u (B, n − 1) and the raw draws (B,) that give each run's pc, as the
    solo path forms it: the host ranking loops on data and reads pc as a float, so ``vmap`` cannot trace through it; this op is
    what a vmapped call reaches."""
    return torch.stack([_select_draw(o, uu, d) for o, uu, d in zip(obj, u, draw)])


@_select_draw_runs.register_fake
def _(obj, u, draw):
    return obj.new_empty(obj.shape[:2], dtype=torch.int64)


def _select_draw(obj, u, draw):
    I1, I2 = indicators_dense(obj)
    return _stochastic_rank_host(I1, I2, u, float(draw) * 0.2 + 0.4)


@torch.library.custom_op("evoxmi_py::sra_select_run", mutates_args=())
def select_run(obj: torch.Tensor, u: torch.Tensor, draw: torch.Tensor) -> torch.Tensor:
    """One run of ``sra_select_runs``; under ``vmap`` its rule calls that op."""
    return _select_draw(obj, u, draw)


@select_run.register_fake
def _(obj, u, draw):
    return obj.new_empty(obj.shape[:1], dtype=torch.int64)


@torch.library.register_vmap("evoxmi_py::sra_select_run")
def _(info, in_dims, obj, u, draw):
    B = info.batch_size
    front = [t.unsqueeze(0).expand((B,) + tuple(t.shape)) if d is None else t.movedim(d, 0) for t, d in zip((obj, u, draw), in_dims)]
    return _select_draw_runs(*front), 0
