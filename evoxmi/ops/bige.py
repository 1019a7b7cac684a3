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
* ``cd_i = sqrt(Σ_j sh)``; the order of the sum is the kernel's own, fixed from call to call, with the pairs at
  distance 0 (each exactly 1) counted in an integer and added last, so equal rows get bitwise equal ``cd``;
* ``bi_i = (float32(pr_i), float32(cd_i))`` for a masked row and (+inf, +inf) for a row outside the mask, which
  contributes to nothing.  (In the torch path it sits at (m, …, m), farther than r from every masked row.)

That holds for finite objectives.  With an empty mask every output is +inf.  With NaN or ±inf objectives the launches
end and the shapes hold, nothing more.

Three launches, no host read, and no array of n² elements: the scratch is (m + 1)·n float64 words."""
from __future__ import annotations

import torch

from . import _ext

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
