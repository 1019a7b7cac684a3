"""Caps of the one-workgroup CMA-ES generation kernels (``csrc/kernels/cma_small.hip``).

``cma_small_ask`` and ``cma_small_tell`` run one workgroup per optimiser run and keep C, B and the
rotated matrix in LDS: d ≤ 64, μ ≤ λ ≤ 1024 (``evx_cma_small_max_d`` / ``evx_cma_small_max_lambda``).
"""
from __future__ import annotations

D_CAP = 64
LAMBDA_CAP = 1024


def caps_ok(d: int, lam: int) -> bool:
    return 1 <= d <= D_CAP and 1 <= lam <= LAMBDA_CAP


def check_batched_caps(d: int, lam: int, what: str) -> None:
    """Batched runs have no run-by-run fallback: a per-run shape above the caps is an error."""
    if not caps_ok(d, lam):
        raise NotImplementedError(f"{what}: batched runs need 1 <= d <= {D_CAP} and 1 <= lambda <= {LAMBDA_CAP} per run")
