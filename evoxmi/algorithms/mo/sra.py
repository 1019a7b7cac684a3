"""SRA — stochastic ranking algorithm (Li et al. 2016; reference ``algorithms/mo/sra.py:115-191``).

Two indicators — I_ε+ fitness (I1) and shift-based density (I2) — are balanced by
stochastic ranking (a bubble sort choosing the comparison indicator at random with
probability pc ∈ [0.4, 0.6]).  The reference fills the SDE distance matrix only below the
diagonal (``sra.py:96-106``), so its I2 ignores later individuals; here I2 is the SDE
nearest-neighbour distance over all j ≠ i.

Both steps are ``evoxmi.ops.sra``.  On a HIP device (merged population ≤ 8192 rows, ≤ 16
objectives) the indicators are one fused pass and the bubble sort runs its sweeps pipelined
in one workgroup (``sra_select.hip``); pc stays a device word and nothing is read on the
host, so a whole generation is captured into one hipGraph (``StdWorkflow(..., graph=True)``).
On the CPU, and above those caps, the indicators are the dense torch expressions and the sort
is the sequential host op ``evoxmi::stochastic_ranking``; those sizes stay eager-only.
"""
from __future__ import annotations

import torch

from ...operators import crossover
from ...ops import random as rnd
from ...ops import sra as sra_ops
from ...ops.sra import _stochastic_rank_host as stochastic_ranking  # noqa: F401  (the host path, under its earlier name)
from ...ops.sra import sde_distance  # noqa: F401
from .common import MOAlgorithm


class SRA(MOAlgorithm):
    def __init__(self, lb, ub, n_objs, pop_size, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op if crossover_op is not None else crossover.SimulatedBinary(type=2))

    def ask(self, state):
        key, sel_key, x_key, mut_key = rnd.split(state.key, 4)
        pool = rnd.randint(sel_key, (self.pop_size * 2,), 0, self.pop_size).to(state.population.device)
        off = self.mutation(mut_key, self.crossover(x_key, state.population[pool]))
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_fit = torch.cat([state.fitness, fitness], 0)
        key, k_pc, k_env = rnd.split(state.key, 3)
        n, m = merged_fit.shape
        if sra_ops.on_device(n, m, merged_fit.device):
            # the value the host path hands to the op (a double product, cast to float), as a device word
            pc = (rnd.uniform(k_pc, ()).double() * 0.2 + 0.4).float()
            I1, I2 = sra_ops.indicators(merged_fit)
        else:
            pc = float(rnd.uniform(k_pc, ())) * 0.2 + 0.4
            I1, I2 = sra_ops.indicators_dense(merged_fit)
        u = rnd.uniform(k_env, (n - 1,))
        idx = sra_ops.stochastic_rank(I1, I2, u, pc)[: self.pop_size]
        return state.update(population=merged_pop[idx], fitness=merged_fit[idx], key=key)
