"""SPEA2 (Zitzler et al. 2001; reference ``algorithms/mo/spea2.py:71-158``).

Strength + raw fitness + k-th nearest-neighbour density; environmental selection
keeps the non-dominated set, filled by fitness or truncated by iteratively removing
the individual closest to its nearest neighbour.

Both steps are ``evoxmi.ops.spea2``.  On a HIP device (merged population ≤ 8192 rows, ≤ 16
objectives) the fitness is two launches without an (n, n) temporary and the removal loop runs in
one workgroup with the removal count on the device (``spea2_select.hip``): eager and captured
generations run the same kernels.  On the CPU, and above those caps, ``cal_fitness``,
``truncation`` and ``truncation_predicated`` (importable from here as before) are the dense torch path.
"""
from __future__ import annotations

import torch

from ...operators import selection
from ...ops import random as rnd
from ...ops import spea2 as spea2_ops
from ...ops.spea2 import cal_fitness, truncation, truncation_predicated  # noqa: F401  (the torch path and the kernels' oracle, under their earlier names)
from .common import MOAlgorithm


class SPEA2(MOAlgorithm):
    # decision-axis state sharding (P2): variation per global column, tournament and
    # truncation from the replicated objectives
    column_separable = True

    def __init__(self, lb, ub, n_objs, pop_size, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op)
        self.selection = selection.Tournament(n_round=pop_size)

    def ask(self, state):
        key, sel_key, x_key, mut_key = rnd.split(state.key, 4)
        selected, _ = self.selection(sel_key, state.population, spea2_ops.fitness(state.fitness))
        off = self._variation(x_key, mut_key, selected, clip=False)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_fit = torch.cat([state.fitness, fitness], 0)
        idx = spea2_ops.select(merged_fit, self.pop_size)
        return state.update(population=merged_pop[idx], fitness=merged_fit[idx])
