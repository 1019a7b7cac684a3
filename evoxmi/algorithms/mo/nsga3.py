"""NSGA-III (Deb & Jain 2014; reference ``algorithms/mo/nsga3.py:27-211``).

Normalisation by the ideal point and the hyperplane through the extreme points
(falling back to the worst point when the extremes are degenerate), association with
Das–Dennis reference points by perpendicular distance, and niche-preserving
selection from the last front.

The reference fills the remaining K slots with a sequential ``while_loop`` (pick the
niche with the smallest count, lowest index first; take its closest candidate when
the niche was empty, a random one otherwise; increment).  That greedy order is
exactly the lexicographic order of the pairs (ρ_j + k, j) over niches j and their
k-th last-front member, so the loop is replaced by one sort: each candidate gets its
within-niche position k (closest first for empty niches, random otherwise) and the K
smallest (ρ_j + k, j) are kept.  Same distribution, no data-dependent loop.

That selection is ``ops.nds.nsga3_survivors``: one launch of ``nsga3_select.hip`` on the
device (merged population ≤ 8192 rows, ≤ 8192 reference points), the same steps in
fixed-shape torch on the CPU and above those caps.  The normalisation and the association
before it are ``ops.nsga3.associate``: three launches of ``nsga3_assoc.hip`` on the device
(float64, no (n, K) array; ≤ 16 objectives), the float32 torch expressions on the CPU and above
the caps.  Nothing reads the host, so a whole generation is captured into one hipGraph
(``StdWorkflow(..., graph=True)``), and every kernel takes a run index, so ``BatchedRuns(NSGA3)``
advances R seeds with the launches of one (merged population ≤ 8192 rows and ≤ 8 objectives per
run, the caps of the batched non-dominated sort); run r is bit-identical to the algorithm alone.
"""
from __future__ import annotations

import torch

from ...core import State
from ...operators import selection
from ...operators.sampling import UniformSampling
from ...operators.selection.non_dominate import non_dominated_sort
from ...ops import nsga3 as nsga3_ops
from ...ops import random as rnd
from ...ops.nds import _in_vmap, nsga3_survivors
from .common import MOAlgorithm


class NSGA3(MOAlgorithm):
    column_separable = True  # variation per global column, selection by the replicated fitness

    def __init__(self, lb, ub, n_objs, pop_size, selection_op=None, mutation_op=None, crossover_op=None):
        super().__init__(lb, ub, n_objs, pop_size, mutation_op, crossover_op)
        self.selection = selection_op if selection_op is not None else selection.UniformRand(1)
        self.ref = UniformSampling(pop_size, n_objs)()[0].to(lb.device)

    def ask(self, state):
        key, mut_key, x_key = rnd.split(state.key, 3)
        off = self._variation(x_key, mut_key, state.population)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        N = self.pop_size
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_fit = torch.cat([state.fitness, fitness], 0)
        if not merged_fit.is_cuda and _in_vmap(merged_fit):
            # a run of BatchedRuns on the CPU: vmap cannot trace the peel loop, the selection goes run by run inside one op
            idx = nsga3_ops.survivors_run(merged_fit, state.key, self.ref, N)
        else:
            rank = non_dominated_sort(merged_fit, until=N + 1)
            # normalisation and association: nsga3_assoc.hip on the device, the torch expressions on the CPU
            last_rank, group, group_dist, _ = nsga3_ops.associate(merged_fit, rank, self.ref, N)
            # niche-preserving selection from the last front: nsga3_select.hip on the device
            idx = nsga3_survivors(rank, last_rank, group, group_dist, state.key, N, self.ref.shape[0])
        key, _ = rnd.split(state.key)
        return state.update(population=merged_pop[idx], fitness=merged_fit[idx], key=key)
