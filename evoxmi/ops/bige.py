"""BiGE's bi-goal estimate: the proximity and the crowding degree of every masked row (``bige_select.hip`` on a HIP
device, the dense torch expression ``algorithms.mo.bige.estimate`` elsewhere).

The kernels' contract.  All arithmetic is float64 on the float32 inputs, in the operation order written here, without
FMA contraction; a host implementation of the same operations reproduces ``pr`` bit for bit and ``cd`` to the
rounding of a sum of non-negative terms.

``estimate(fit (n, m), mask (n))`` → ``bi (n, 2) float32``:

* ``r = 1 / mask.sum().float() ** (1 / m)`` is computed by torch on the device, a float32 word; the kernels read it as
  ``(double)r``.  (A device ``pow`` is not reproducible on the host, so r is an input of the contract, not part of it.)
* column extremes: ``fmin_k`` and ``fmax_k`` are the float32 extremes over the masked rows (exact);
  ``span_k = max((double)fmax_k − (double)fmin_k, 1e-6)``;
* a masked row i: ``x_ik = ((double)f_ik − (double)fmin_k) / span_k`` and ``pr_i = ((x_i0 + x_i1) + x_i2) + …``;
* the masked rows j ≠ i: ``d2 = ((δ_0² + δ_1²) + …)`` with ``δ_k = x_ik − x_jk``, and ``d = sqrt(d2)``.  If ``d < r``:
  ``w = 1 + (pr_i ≥ pr_j) + (pr_i > pr_j)``, compared in float64, and ``sh = (0.5 · (w · (1 − d / r)))²``; otherwise the
  pair contributes 0;
* ``cd_i = sqrt(Σ_j sh)``.  The order of the sum is part of the contract: partial l of 64 adds the terms of the partners
  ``j ≡ l (mod 64)`` in ascending j (a float64 sum from 0); the pairs at distance 0 (each exactly 1) are counted in an integer
  per partial instead; partials and counts combine by the xor butterfly 32, 16, …, 1 (``s_l ← s_l + s_{l xor k}``); then
  ``cd_i = sqrt(acc + dup)``.  Equal rows, whose other terms are the same words at the same positions, so get bitwise equal
  ``cd``, and a second call gives the same words;
* ``bi_i = (float32(pr_i), float32(cd_i))`` for a masked row and (+inf, +inf) for a row outside the mask, which
  contributes to nothing.  (In the torch path it sits at (m, …, m), farther than r from every masked row.)

That holds for finite objectives.  With an empty mask every output is +inf.  With NaN or ±inf objectives the launches
end and the shapes hold, nothing more.

Three launches, no host read, and no array of n² elements: the scratch is (m + 1)·n float64 words.

``estimate_rank(fit, mask)`` → ``(bi, rank)`` adds the Pareto rank of the bi-goal points, which is what BiGE takes from an
estimate.  On ``fit`` (n, m) that is ``estimate`` and then the non-dominated sort, launch for launch.  On ``fit`` (B, n, m) with
``mask`` (B, n), and for a run under ``vmap`` (``evoxmi/ops/batching.py``), it serves B independent runs: on a HIP device ONE
launch of ``bige_small.hip``, a workgroup per run that keeps the run's x and pr in LDS (no scratch), forms ``cd`` in the sum order
above and ranks the bi-goal pairs there by dominator counts and front peeling (``nds.hip``'s contract), so every run gets the words
of the 2-D call (``csrc/include/evoxmi_bige.h`` holds the operations for both paths).  r stays an input, one word per run.  Its caps
per run are ``small_ok``'s: n ≤ 2048, 1024 or 512 rows at m ≤ 4, 8 or 16; above them it raises, it does not go run by run.  On the
CPU the 2-D path runs run by run."""
from __future__ import annotations

import torch

from . import _ext
from .nds import _in_vmap

M_CAP = 16  # bige_select.hip: a row's x stays in registers
N_CAP = 32768  # not structural: it bounds the scratch and the time of the one-workgroup extremes launch


def tile_rows(m: int) -> int:
    """The rows j of one LDS tile of the crowding launch at ``m`` objectives."""
    return 4096 // (4 if m <= 4 else (8 if m <= 8 else 16))


def on_device(n: int, m: int, device) -> bool:
    """Whether n rows of m objectives on ``device`` run the kernels."""
    return torch.device(device).type == "cuda" and 1 <= n <= N_CAP and 1 <= m <= M_CAP


def estimate(fit: torch.Tensor, mask: torch.Tensor, return_parts: bool = False):
    """``bi`` (n, 2) float32: (proximity, crowding degree) of the masked rows of ``fit`` (n, m), +inf outside the mask.
    On a HIP device within the caps three launches of ``bige_select.hip`` (``return_parts`` adds ``pr`` and ``cd`` in
    float64); elsewhere the dense float32 expression of ``algorithms.mo.bige``."""
    if fit.dim() == 2 and fit.dtype == torch.float32 and on_device(fit.shape[0], fit.shape[1], fit.device):
        mask = mask.to(device=fit.device, dtype=torch.bool).contiguous()
        r = 1 / mask.sum().to(torch.float32) ** (1 / fit.shape[1])
        bi, pr, cd = _ext.ops().bige_estimate(fit.contiguous(), mask, r)
        return (bi, pr, cd) if return_parts else bi
    if return_parts:
        raise ValueError("return_parts is the kernels' only")
    from ..algorithms.mo.bige import estimate as torch_estimate

    return torch_estimate(fit, mask)


def small_ok(n: int, m: int) -> bool:
    """Whether ``bige_small.hip`` takes runs of n rows and m objectives: a run's x, m·n float64 words padded to 4, 8 or 16
    objectives, stays within 64 KiB of LDS."""
    return n >= 1 and 1 <= m <= M_CAP and n * (4 if m <= 4 else (8 if m <= 8 else 16)) <= 8192


def check_small_caps(n: int, m: int, what: str) -> None:
    if not small_ok(n, m):
        raise NotImplementedError(f"{what}: batched runs need n <= 2048 (m <= 4), 1024 (m <= 8) or 512 (m <= 16) rows per run, "
                                  f"got n = {n}, m = {m}")


def _estimate_rank_2d(fit, mask, return_parts=False):
    from ..operators.selection.non_dominate import non_dominated_sort

    if return_parts:
        bi, pr, cd = estimate(fit, mask, True)
        return bi, non_dominated_sort(bi), pr, cd
    bi = estimate(fit, mask)
    return bi, non_dominated_sort(bi)


def _radius(mask, m):
    """r of every run of mask (…, n): one float32 word each, the expression of ``estimate``."""
    return 1 / mask.sum(-1).to(torch.float32) ** (1 / m)


def _estimate_rank_runs(fit, mask, return_parts):
    B, n, m = fit.shape
    mask = mask.to(device=fit.device, dtype=torch.bool)
    if fit.device.type == "cuda":
        if fit.dtype != torch.float32:
            raise NotImplementedError("ops.bige.estimate_rank: batched runs on a device need float32 objectives")
        check_small_caps(n, m, "ops.bige.estimate_rank")
        bi, rank, pr, cd = _ext.ops().bige_small_estimate_rank(fit.contiguous(), mask.contiguous(), _radius(mask, m).contiguous())
        return (bi, rank, pr, cd) if return_parts else (bi, rank)
    if return_parts:
        raise ValueError("return_parts is the kernels' only")
    runs = [_estimate_rank_2d(fit[r], mask[r]) for r in range(B)]
    return torch.stack([bi for bi, _ in runs]), torch.stack([rank for _, rank in runs])


@torch.library.custom_op("evoxmi_py::bige_estimate_rank_run", mutates_args=())
def _estimate_rank_run(fit: torch.Tensor, mask: torch.Tensor) -> list[torch.Tensor]:
    """The torch path on fit (n, m), or run by run on (B, n, m): r is a float32 CPU ``pow``, which rounds an element by its place in
    the tensor (``utils.common.pow_under_vmap``), and ``cdist`` and the peel loop do not batch either; this op is what a vmapped CPU
    call reaches."""
    return list(_estimate_rank_runs(fit, mask, False) if fit.dim() == 3 else _estimate_rank_2d(fit, mask))


@_estimate_rank_run.register_fake
def _(fit, mask):
    return [fit.new_empty(fit.shape[:-1] + (2,)), fit.new_empty(fit.shape[:-1], dtype=torch.int32)]


@torch.library.register_vmap("evoxmi_py::bige_estimate_rank_run")
def _(info, in_dims, fit, mask):
    B = info.batch_size
    fb, mb = (t.unsqueeze(0).expand((B,) + tuple(t.shape)) if d is None else t.movedim(d, 0) for t, d in zip((fit, mask), in_dims))
    return _estimate_rank_run(fb, mb), [0, 0]


def estimate_rank(fit: torch.Tensor, mask: torch.Tensor, return_parts: bool = False):
    """``(bi, rank)``: ``estimate(fit, mask)`` and the Pareto rank (int32, 0 = first front) of its rows, the rows outside the mask,
    at (+inf, +inf), included.  ``return_parts`` adds ``pr`` and ``cd`` in float64, on a device only.

    ``fit`` (n, m) outside ``vmap`` is ``estimate`` followed by the non-dominated sort.  ``fit`` (B, n, m) with ``mask`` (B, n) is B
    independent runs, every result with a leading run axis: on a HIP device ONE launch of ``bige_small.hip``, a workgroup per run,
    whose words are those of the 2-D call on each run; runs above its caps (``small_ok``) raise ``NotImplementedError``.  A run under
    ``vmap`` reaches the same launch through the op's rule (an unbatched operand is broadcast).  On the CPU the 2-D path runs run by
    run, also under ``vmap``."""
    if fit.dim() == 3:
        return _estimate_rank_runs(fit, mask, return_parts)
    if _in_vmap(fit) or _in_vmap(mask):
        if not fit.is_cuda:
            if return_parts:
                raise ValueError("return_parts is the kernels' only")
            return tuple(_estimate_rank_run(fit, mask))
        if fit.dtype != torch.float32:
            raise NotImplementedError("ops.bige.estimate_rank: batched runs on a device need float32 objectives")
        mask = mask.to(device=fit.device, dtype=torch.bool)
        bi, rank, pr, cd = _ext.ops().bige_small_estimate_rank(fit, mask, _radius(mask, fit.shape[1]))  # the rule of ops/batching.py
        return (bi, rank, pr, cd) if return_parts else (bi, rank)
    return _estimate_rank_2d(fit, mask, return_parts)
