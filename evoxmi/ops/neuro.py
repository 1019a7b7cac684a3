"""Launchers of the persistent rollout kernels: Ant + MLP (``neuro.hip``) and the planar
articulated-tree tasks + MLP (``planar_rollout.hip``)."""
from __future__ import annotations

import torch

from . import _ext


def ant_param_count(h1: int, h2: int) -> int:
    return 27 * h1 + h1 + h1 * h2 + h2 + h2 * 8 + 8


def ant_rollout(flat_weights: torch.Tensor, h1: int, h2: int, init_state: torch.Tensor, cap: int):
    """Episode returns (N,) and lengths (N,) of N individuals whose MLP 27-h1-h2-8 (tanh)
    weights are rows of ``flat_weights`` in the layout [W1 (27×h1), b1, W2 (h1×h2), b2,
    W3 (h2×8), b3], all starting from ``init_state`` (29,)."""
    return _ext.ops().ant_rollout(flat_weights.to(torch.float32).contiguous(), int(h1), int(h2),
                                  init_state.to(device=flat_weights.device, dtype=torch.float32).contiguous(), int(cap))


def ant_lds_bytes(h1: int, h2: int, waves: int = 1) -> int:
    """LDS that ``waves`` waves of the LDS-resident Ant kernel (``h1`` or ``h2`` above 64) need.  The launcher
    puts up to 4 waves in a workgroup, as many as stay within ``ant_lds_limit()``; the binding refuses a policy
    whose single wave does not."""
    return _ext.ops().ant_lds_bytes(int(h1), int(h2), int(waves))


def ant_lds_limit() -> int:
    return _ext.ops().ant_lds_limit()


def planar_param_count(obs_dim: int, h1: int, h2: int, act_dim: int) -> int:
    return obs_dim * h1 + h1 + h1 * h2 + h2 + h2 * act_dim + act_dim


PLANAR_LDS_LIMIT = 160 * 1024  # one wave's share of LDS, in bytes


def planar_lds_bytes(obs_dim: int, h1: int, h2: int, act_dim: int) -> int:
    """LDS one wave of ``planar_rollout`` needs: weights, 32 spare words and the activations; the binding
    refuses a policy that needs more than ``PLANAR_LDS_LIMIT``."""
    return (planar_param_count(obs_dim, h1, h2, act_dim) + 32 + h1 + h2 + 8) * 4


def planar_rollout(flat_weights: torch.Tensor, h1: int, h2: int, model: torch.Tensor, init_state: torch.Tensor, cap: int):
    """Episode returns (N,) float32 and lengths (N,) int32 of N individuals on a planar
    articulated-tree model.  ``model`` is the float32 table of ``PlanarChain.model_table()`` (kept
    in host memory: it is passed to the kernel by value, so the launch captures into a hipGraph);
    the MLP obs-h1-h2-act (tanh) weights are rows of ``flat_weights`` in the layout [W1 (obs×h1),
    b1, W2 (h1×h2), b2, W3 (h2×act), b3]; every individual starts from ``init_state`` (2·nd + n_aux,) =
    q ++ u ++ aux (the reach task's target; nothing for the other kinds).  The observation, action and
    auxiliary sizes follow from the table.  Raises for a model or policy outside the kernel's caps (≤ 8
    bodies, ≤ 10 degrees of freedom, ≤ 32 observations, ≤ 8 actions, hidden ≤ 512, ``planar_lds_bytes`` ≤
    ``PLANAR_LDS_LIMIT``) or outside the six instantiated combinations of tree shape, root constraint and task
    kind: chains of 3 or 4 bodies or a root with two chains of 3 with a free root and the run task (every hinge
    driven); chain of 2, x-only root, balance and chain of 3, x-only root, balance_tip (the slider driven, the
    hinges passive); chain of 3, locked root, reach (both hinges driven)."""
    return _ext.ops().planar_rollout(flat_weights.to(torch.float32).contiguous(), int(h1), int(h2),
                                     model.to(device="cpu", dtype=torch.float32).contiguous(),
                                     init_state.to(device=flat_weights.device, dtype=torch.float32).contiguous(), int(cap))
