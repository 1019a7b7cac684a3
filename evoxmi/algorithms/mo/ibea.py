"""IBEA (Zitzler & Künzli 2004; reference ``algorithms/mo/ibea.py:21-132``).

I_ε+ indicator fitness and iterative removal of the worst individual with fitness
correction.  The removal loop has a fixed trip count (N) and no host
synchronisation, so it stays on the device (and inside a hipGraph).

Both steps are ``evoxmi.ops.ibea``.  On a HIP device (merged population ≤ 8192 rows, ≤ 16
objectives) the fitness is one pass that stores no indicator matrix and the whole removal
loop runs in one workgroup (``ibea_select.hip``): two launches per selection.  On the CPU,
and above those caps, ``cal_fitness`` and ``ibea_truncate`` below are the dense torch
expressions and the loop of torch ops; both paths are capturable.
"""
from __future__ import annotations

import torch

from ...core import State
from ...operators import selection
from ...ops import ibea as ibea_ops
from ...ops import random as rnd
from ...ops.ibea import cal_fitness, ibea_truncate  # noqa: F401  (the torch path and the kernels' oracle, under their earlier names)
from .common import MOAlgorithm


class IBEA(MOAlgorithm):
    column_separable = True  # variation per global column, selection by the replicated fitness

    def __init__(self, lb, ub, n_objs, pop_size, kappa=0.05, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op)
        self.kappa = kappa
        self.selection = selection.Tournament(n_round=pop_size)

    def ask(self, state):
        key, sel_key, x_key, mut_key = rnd.split(state.key, 4)
        fit = ibea_ops.fitness(state.fitness, self.kappa)[0]
        selected, _ = self.selection(sel_key, state.population, -fit)
        off = self._variation(x_key, mut_key, selected, clip=False)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_obj = torch.cat([state.fitness, fitness], 0)
        idx = ibea_ops.select(merged_obj, self.kappa, self.pop_size)
        return state.update(population=merged_pop[idx], fitness=merged_obj[idx])
