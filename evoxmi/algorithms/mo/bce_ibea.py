"""BCE-IBEA — bi-criterion evolution with IBEA (Li, Yang & Liu 2016; reference ``algorithms/mo/bce_ibea.py:174-332``).

Two cooperating populations: the Pareto-criterion population PC (non-dominated,
niche-truncated to N) and the IBEA non-Pareto-criterion population NPC.  Generations
alternate: odd ones explore around under-populated PC members, even ones run IBEA
variation on NPC; NPC is always updated by IBEA environmental selection and PC by
the PC selection over everything evaluated.  The reference mixes up the objective
arrays between the two populations in its odd/even tells (e.g. ``fitness=npc_obj``
in ``_tell_odd``); here each population keeps its own objectives.

On a HIP device both selections and the exploration test are HIP kernels
(``ops/ibea.py``, ``ops/bce.py``), ``n_nd`` and ``counter`` are device words and the
odd branch has a fixed shape: ``ask`` and ``tell`` read nothing on the host, and
``StdWorkflow(graph=True)`` captures a generation into a hipGraph, one graph per
parity (``graph_variant``).  ``graph="auto"`` stays eager (``graph_auto``).
"""
from __future__ import annotations

import contextlib

import torch

from ...operators import crossover, selection
from ...ops import bce as bce_ops
from ...ops import ibea as ibea_ops
from ...ops import random as rnd
from .common import MOAlgorithm


exploration = bce_ops.exploration


def pc_selection(pc, pc_obj, n):
    idx, n_nd = bce_ops.pc_selection_indices(pc_obj, n)
    return pc[idx], pc_obj[idx], n_nd


def ibea_selection(pop, obj, n, kappa):
    idx = ibea_ops.select(obj, kappa, n)
    return pop[idx], obj[idx]


class BCEIBEA(MOAlgorithm):
    # graph="auto" keeps the eager generation it has always run for BCE-IBEA: test_bce_ibea_still_falls_back_to_eager
    # (tests/test_ibea_select_gpu.py) asserts it.  The eager generation runs the same kernels and reads nothing on the
    # host; graph=True captures.  Once that test asserts a capture instead, this line and Algorithm.graph_auto can go.
    graph_auto = False

    def __init__(self, lb, ub, n_objs, pop_size, kappa=0.05, selection_op=None, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op)
        self.kappa = kappa
        self.selection = selection.Tournament(n_round=pop_size)
        self.crossover_odd = crossover.SimulatedBinary(type=2)
        self._parity = None  # of the generation being run, inside a graph_variant_context

    def setup(self, key):
        st = super().setup(key)
        dev = st.population.device
        z = torch.zeros((self.pop_size, self.n_objs), device=dev)
        if dev.type == "cuda":  # device words: a captured generation updates them in place
            return st.update(npc=st.population.clone(), npc_obj=z, n_nd=torch.zeros((), dtype=torch.int64, device=dev),
                             counter=torch.ones((), dtype=torch.int64, device=dev))
        return st.update(npc=st.population.clone(), npc_obj=z, n_nd=0, counter=1)

    # ---- the generation's parity is the workflow's: init_ask / init_tell are generation 0 and leave counter = 1,
    # every tell adds one, so counter equals the workflow generation from generation 1 on
    def graph_variant(self, generation: int):
        return "explore" if generation % 2 else "ibea"

    def graph_variant_set(self):
        return ("explore", "ibea")

    @contextlib.contextmanager
    def graph_variant_context(self, variant):
        prev, self._parity = self._parity, 1 if variant == "explore" else 0
        try:
            yield
        finally:
            self._parity = prev

    def _pc_select(self, pop, obj):
        idx, n_nd = bce_ops.pc_select(obj, self.pop_size)
        return pop[idx], obj[idx], n_nd if obj.is_cuda else int(n_nd)

    def init_tell(self, state, fitness):
        pc, pc_obj, n_nd = self._pc_select(state.population, fitness)
        return state.update(population=pc, fitness=pc_obj, npc=state.population, npc_obj=fitness, n_nd=n_nd)

    def ask(self, state):
        key, k1, x_key, mut_key = rnd.split(state.key, 4)
        N = self.pop_size
        parity = self._parity if self._parity is not None else int(state.counter) % 2  # a direct call: one host read
        if parity == 0:  # IBEA variation on NPC
            fit = -ibea_ops.fitness(state.npc_obj, self.kappa)[0]
            selected, _ = self.selection(k1, state.npc, fit)
            off = self.mutation(mut_key, self.crossover(x_key, selected))
        else:  # PC exploration, fixed shape: the candidates first, cycled; no candidate keeps the population
            s = bce_ops.explore(state.fitness, state.npc_obj, state.n_nd, N)
            cnt = s.sum()
            cand = torch.argsort((~s).to(torch.int8), stable=True)
            mate = rnd.randint(k1, (N,), 0, N).to(cand.device)
            first = cand[torch.arange(N, device=cand.device) % torch.clamp(cnt, min=1)]
            parents = torch.cat([state.population[first], state.population[mate]])
            varied = self.mutation(mut_key, self.crossover_odd(x_key, parents))
            off = torch.where(cnt > 0, varied, state.population)
        off = torch.clamp(off, self.lb, self.ub)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        N = self.pop_size
        npc, npc_obj = ibea_selection(torch.cat([state.npc, state.next_generation]), torch.cat([state.npc_obj, fitness]), N, self.kappa)
        pc, pc_obj, n_nd = self._pc_select(torch.cat([state.population, state.next_generation]), torch.cat([state.fitness, fitness]))
        return state.update(population=pc, fitness=pc_obj, npc=npc, npc_obj=npc_obj, n_nd=n_nd, counter=state.counter + 1)
