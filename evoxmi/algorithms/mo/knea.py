"""KnEA — knee-point-driven EA (Zhang, Tian & Jin 2015; reference ``algorithms/mo/knea.py:39-221``).

Mating: binary tournament by (front rank, knee flag, weighted distance DW).
Environmental selection: non-dominated fronts up to the critical one; in every front
the knee points are found by scanning the members in order of their distance to the
extreme hyperplane and suppressing neighbours within the adaptive radius R (a
sequential scan); the last front is completed / trimmed by hyperplane distance.
``ops.knea.select`` does all of it: one launch of ``knea_select.hip`` on a HIP
device (n ≤ 8192, m ≤ 16), which reads nothing on the host, so a generation
captures into a hipGraph; a host loop on the CPU and above the caps.
"""
from __future__ import annotations

import torch

from ...core import State
from ...operators.selection.misc import tournament_multi_fit
from ...operators.selection.non_dominate import non_dominated_sort
from ...ops import knea as knea_ops
from ...ops import random as rnd
from ...ops.knea import _plane  # noqa: F401  (the host path's plane, importable from here as before)
from .common import MOAlgorithm


def calc_DW(fit, k):
    dis = torch.cdist(fit, fit)
    nb = torch.sort(dis, 1).values[:, 1 : k + 1]
    avg = nb.mean(1, keepdim=True)
    r = 1 / torch.abs(nb - avg).clamp(min=1e-12)
    w = r / r.sum(1, keepdim=True)
    return (nb * w).sum(1)


class KnEA(MOAlgorithm):
    def __init__(self, lb, ub, n_objs, pop_size, knee_rate=0.5, k_neighbors=3, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op)
        self.knee_rate, self.k_neighbors = knee_rate, k_neighbors

    def setup(self, key):
        st = super().setup(key)
        dev = st.population.device
        # on a device r and t are 0-dim float64 words that the selection kernel reads and writes there
        r, t = (1.0, 0.0) if dev.type == "cpu" else (torch.tensor(v, dtype=torch.float64, device=dev) for v in (1.0, 0.0))
        return st.update(knee=torch.zeros(self.pop_size, dtype=torch.bool, device=dev), r=r, t=t)

    def ask(self, state):
        k0, k1, k2, k3 = rnd.split(state.key, 4)
        rank = non_dominated_sort(state.fitness).to(torch.float32)
        DW = calc_DW(state.fitness, self.k_neighbors)
        keys = torch.stack([rank, (~state.knee).to(torch.float32), -DW], 1)
        selected, _ = tournament_multi_fit(k1, state.population, keys, self.pop_size)
        off = self._variation(k2, k3, selected)
        return off, state.update(next_generation=off, key=k0)

    def tell(self, state, fitness):
        N = self.pop_size
        pop = torch.cat([state.population, state.next_generation])
        obj = torch.cat([state.fitness, fitness])
        rank = non_dominated_sort(obj)
        order = torch.argsort(rank, stable=True)
        rank, pop, obj = rank[order], pop[order], obj[order]
        idx, knee, r, t = knea_ops.select(obj, rank, N, state.r, state.t, self.knee_rate)
        return state.update(population=pop[idx], fitness=obj[idx], knee=knee[idx], r=r, t=t)
