"""MOEA/D (reference ``algorithms/mo/moead.py:19-134``).

Semantics kept: Das–Dennis weights with ``pop_size`` overwritten by the number of
weight vectors, T = ⌈N/10⌉ nearest neighbours, two random neighbours → SBX
(type 2) + polynomial mutation, default PBI aggregation (``func_name``).

``tell`` — the reference runs a *sequential* ``lax.scan`` over the N offspring,
each replacing neighbours it improves.  During that scan ``z``, ``z_max`` and the
weights are fixed, so slot ``s`` only ever compares its *own* current occupant
with offspring ``i`` (for every ``i`` whose neighbourhood contains ``s``, in
increasing ``i``) and replaces on strict improvement.  Its final occupant is
therefore the **first minimiser** of the aggregation over
``[original, offspring i ∈ revN(s) in order]`` — an exact, order-preserving
reformulation that evaluates all N·T (slot, offspring) pairs at once and
reduces per slot (a segmented first-argmin over the reverse-neighbour CSR),
then gathers only the winning rows.  At N = 16384, d = 10 000 this replaces
16 384 dependent steps (each moving T rows of 10 000 floats) with one parallel
pass plus one row gather.
"""
from __future__ import annotations

import math

import torch

from ...core import Algorithm, State
from ...operators import crossover, mutation
from ...operators.sampling import UniformSampling
from ...ops import geom
from ...ops import random as rnd
from ...utils.common import AggregationFunction


def nearest_neighbors(w: torch.Tensor, T: int) -> torch.Tensor:
    """T nearest weight vectors of every weight (ties by index, like the reference's stable
    argsort of the distance matrix, moead.py:65-67).  On the GPU one fused kernel keeps
    each row's top-T in registers (``ops.geom.knn``, K17): no N×N matrix at N = 16384."""
    return geom.knn(w, w, T)[1]


def reverse_neighbors(neighbors: torch.Tensor):
    """CSR of {i : s ∈ N(i)} for every slot s, with i ascending inside each row."""
    n, T = neighbors.shape
    slots = neighbors.reshape(-1)
    owners = torch.arange(n, device=neighbors.device).repeat_interleave(T)
    key = slots.to(torch.int64) * n + owners
    order = torch.argsort(key)
    rev_owner = owners[order]
    rev_slot = slots[order]
    counts = torch.bincount(slots, minlength=n)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=neighbors.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, rev_slot, rev_owner


def first_argmin_segments(vals: torch.Tensor, seg: torch.Tensor, n_seg: int):
    """Per segment: (min value, position of its first occurrence) — positions are global."""
    inf = torch.full((n_seg,), float("inf"), device=vals.device, dtype=vals.dtype)
    segmin = inf.scatter_reduce(0, seg, vals, reduce="amin", include_self=True)
    pos = torch.arange(vals.shape[0], device=vals.device)
    big = torch.full((n_seg,), vals.shape[0], device=vals.device, dtype=torch.int64)
    cand = torch.where(vals == segmin[seg], pos, torch.full_like(pos, vals.shape[0]))
    first = big.scatter_reduce(0, seg, cand, reduce="amin", include_self=True)
    return segmin, first


def moead_replace(pop_obj, off_obj, w, z, z_max, agg, rev):
    """Exact parallel form of the reference's sequential replacement scan.

    Returns (winner offspring index per slot or −1, new objective matrix)."""
    rowptr, rev_slot, rev_owner = rev
    n = pop_obj.shape[0]
    f_old = agg(pop_obj, w, z, z_max)
    f_new = agg(off_obj[rev_owner], w[rev_slot], z, z_max)
    # the scan's ``f_old > f_new`` is false for a NaN aggregate on either side: such an offspring never takes a
    # slot (and must not poison the segment minimum for the others), such an occupant stays
    f_new = torch.where(torch.isnan(f_new), torch.full_like(f_new, float("inf")), f_new)
    segmin, first = first_argmin_segments(f_new, rev_slot, n)
    better = segmin < f_old
    has = first < f_new.shape[0]
    win = torch.where(better & has, rev_owner[first.clamp_max(f_new.shape[0] - 1)], torch.full_like(first, -1))
    new_obj = torch.where((win >= 0)[:, None], off_obj[win.clamp_min(0)], pop_obj)
    return win, new_obj


def locality_order(w: torch.Tensor, leaves: int = 64) -> torch.Tensor:
    """Permutation of the rows of ``w`` (N × M weight vectors) by recursive coordinate bisection
    into ``leaves`` parts: each split sorts its points along the coordinate of largest spread and
    cuts at the median (stable sorts: deterministic)."""
    ids = torch.arange(w.shape[0])
    wc = w.detach().to("cpu", torch.float64)

    def rec(ix, parts):
        if parts <= 1 or ix.numel() <= 1:
            return [ix]
        pts = wc[ix]
        ax = int((pts.max(0).values - pts.min(0).values).argmax())
        o = ix[torch.argsort(pts[:, ax], stable=True)]
        h = parts // 2
        cut = o.numel() * h // parts
        return rec(o[:cut], h) + rec(o[cut:], parts - h)

    return torch.cat(rec(ids, leaves)).to(w.device)


class MOEAD(Algorithm):
    def __init__(self, lb, ub, n_objs, pop_size, func_name="pbi", mutation_op=None, crossover_op=None):
        super().__init__()
        self.lb, self.ub = lb, ub
        self.n_objs = n_objs
        self.dim = lb.shape[0]
        self.pop_size = pop_size
        self.func_name = func_name
        self.n_neighbor = 0
        self.mutation = mutation_op if mutation_op is not None else mutation.Polynomial((lb, ub))
        self.crossover = crossover_op if crossover_op is not None else crossover.SimulatedBinary(type=2)
        self.sample = UniformSampling(self.pop_size, self.n_objs)
        self.aggregate_func = AggregationFunction(self.func_name)
        self._rev = None
        self._rev32 = None

    def setup(self, key):
        key, k1, k2 = rnd.split(key, 3)
        dev = self.lb.device
        w, _ = self.sample(k2)
        # slots in a locality-preserving order (recursive coordinate bisection of the weight
        # vectors): any power-of-two contiguous split of the slot range is a compact region of the
        # simplex, so a rank's T = N/10 neighbourhoods stay mostly inside its own slots.  The
        # weight SET and the neighbourhoods are the reference's (moead.py:53-77); only slot indices
        # are permuted.  Owner-computes halo at rank 0..7 of 8 (pop 16 290, 3 objectives): mean
        # 0.456 → 0.375, worst rank 0.572 → 0.416 of the population; at world 2 the cut through
        # the middle is already optimal (0.707: own half + the boundary band).
        w = w[locality_order(w)]
        w = w.to(dev)
        self.pop_size = w.shape[0]
        self.n_neighbor = int(math.ceil(self.pop_size / 10))
        pop = rnd.uniform(k1, (self.pop_size, self.dim)).to(dev) * (self.ub - self.lb) + self.lb
        neighbors = nearest_neighbors(w, self.n_neighbor)
        return State(
            population=pop,
            fitness=torch.zeros((self.pop_size, self.n_objs), device=dev),
            next_generation=pop,
            weight_vector=w,
            neighbors=neighbors,
            z=torch.zeros(self.n_objs, device=dev),
            key=key,
            # parents (p0, p1) and variation keys of the current offspring, and the last
            # replacement's winner per slot (−1: kept): what the population-sharded tell needs
            # to regenerate winning rows locally instead of moving them between GPUs
            parents=torch.zeros((2, self.pop_size), dtype=torch.int32, device=dev),
            var_keys=torch.zeros((2, 2), dtype=torch.int64, device=dev),
            win=torch.full((self.pop_size,), -1, dtype=torch.int32, device=dev),
        )

    def init_ask(self, state):
        return state.population, state

    def init_tell(self, state, fitness):
        return state.update(fitness=fitness, z=fitness.min(0).values)

    def _parents(self, state, key):
        n, T = state.neighbors.shape
        # independent permutation of every neighbour row; only the first two columns are used
        perm = torch.argsort(rnd.uniform(key, (n, T)).to(state.neighbors.device), dim=1, stable=True)[:, :2]
        return torch.gather(state.neighbors, 1, perm)

    def _fused(self, x):
        """The default SBX(type 2) + PM pipeline runs as the fused moead.hip kernels on a GPU."""
        c, m = self.crossover, self.mutation
        return (x.is_cuda and x.dtype == torch.float32 and self.dim > 0
                and type(c) is crossover.SimulatedBinary and c.type == 2
                and type(m) is mutation.Polynomial and m.boundary[0] is self.lb and m.boundary[1] is self.ub)

    def _parent_pairs(self, state, key, row0=0, rows=0):
        """(2, N) int32: the two parents of every offspring (first two entries of a random
        permutation of its neighbour row); ``rows > 0`` (owner mode on a GPU): only those
        offspring's parents are drawn."""
        if self._fused(state.population):
            from ...ops import mo as mo_ops

            p0, p1 = mo_ops.moead_parents(state.neighbors, key, row0, rows)
            return torch.stack([p0, p1])
        return self._parents(state, key).T.to(torch.int32).contiguous()

    def _offspring_rows(self, state, parents, sel_key, mut_key, row0=0, rows=0, win=None):
        """Offspring of ``parents`` (all, a row slice, or — with ``win`` — the winner of every
        slot with ``population`` where there is none).  Counters are global offspring
        indices, so every variant is bit-identical to the full generation."""
        pop = state.population
        c, m = self.crossover, self.mutation
        if self._fused(pop):
            from ...ops import mo as mo_ops

            return mo_ops.moead_variation(pop, parents[0].contiguous(), parents[1].contiguous(), sel_key, mut_key, self.lb, self.ub,
                                          c.pro_c, c.dis_c, m.pro_m, m.dis_m, row0=row0, rows=rows, win=win)
        p = parents.long()
        off = torch.clamp(self.mutation(mut_key, self.crossover(sel_key, torch.cat([pop[p[0]], pop[p[1]]], 0))), self.lb, self.ub)
        if win is not None:
            return torch.where((win >= 0)[:, None], off[win.long().clamp_min(0)], pop)
        return off[row0 : row0 + rows] if rows else off

    def ask(self, state):
        key, sub, sel_key, mut_key = rnd.split(state.key, 4)
        parents = self._parent_pairs(state, sub)
        buf = state.next_generation
        if (state.population.is_cuda and torch.cuda.is_current_stream_capturing() and self._fused(state.population) and buf is not None
                and buf.shape == state.population.shape and buf.is_contiguous() and buf.data_ptr() != state.population.data_ptr()):
            # hipGraph: generate straight into the captured offspring buffer (no state write-back copy)
            from ...ops import mo as mo_ops

            c, m = self.crossover, self.mutation
            off = mo_ops.moead_variation(state.population, parents[0].contiguous(), parents[1].contiguous(), sel_key, mut_key, self.lb,
                                         self.ub, c.pro_c, c.dis_c, m.pro_m, m.dis_m, out=buf)
        else:
            off = self._offspring_rows(state, parents, sel_key, mut_key)
        return off, state.update(next_generation=off, key=key, parents=parents, var_keys=torch.stack([sel_key, mut_key]))

    def _reverse(self, state):
        if self._rev is None or self._rev[0].device != state.neighbors.device or self._rev[1].shape[0] != state.neighbors.numel():
            self._rev = reverse_neighbors(state.neighbors)
        return self._rev

    def _replace(self, state, fitness):
        z = torch.minimum(state.z, fitness.min(0).values)
        z_max = state.fitness.max(0).values
        if fitness.is_cuda and state.population.dtype == torch.float32:
            from ...ops import mo as mo_ops

            rowptr, _, owner = self._reverse(state)
            if self._rev32 is None or self._rev32[0].data_ptr() != rowptr.data_ptr():
                self._rev32 = (rowptr, rowptr.to(torch.int32), owner.to(torch.int32))
            win, new_obj = mo_ops.moead_replace(state.fitness, fitness, state.weight_vector, z, z_max, self._rev32[1], self._rev32[2], self.func_name)
        else:
            win, new_obj = moead_replace(state.fitness, fitness, state.weight_vector, z, z_max, self.aggregate_func, self._reverse(state))
        return win.to(torch.int32), new_obj, z

    def tell(self, state, fitness):
        win, new_obj, z = self._replace(state, fitness)
        if state.population.is_cuda and state.population.dtype == torch.float32:
            from ...ops import mo as mo_ops

            if torch.cuda.is_current_stream_capturing() and state.population.is_contiguous():
                # hipGraph: the captured population buffer is the one the next replay reads, so
                # only the winning rows are written and the state write-back has nothing to copy
                new_pop = mo_ops.moead_select_rows_(state.population, state.next_generation, win)
            else:
                new_pop = mo_ops.moead_select_rows(state.population, state.next_generation, win)
        else:
            new_pop = torch.where((win >= 0)[:, None], state.next_generation[win.long().clamp_min(0)], state.population)
        return state.update(population=new_pop, fitness=new_obj, z=z, win=win)

    # ------------------------------------------------------------------ population-sharded SPMD
    # Slots (weight vectors, Das–Dennis order = contiguous regions of the simplex) are split in
    # balanced contiguous ranges; the population stays replicated.  A rank generates and
    # evaluates only its own slots' offspring; the (N, m) objectives are all-gathered (196 KB
    # at N = 16 290); the exact parallel replacement runs redundantly on every rank; each rank
    # then REGENERATES the winning offspring rows from its replica (same parents, keys and
    # counters) instead of receiving them — no d-length row crosses xGMI.
    #
    # Owner-computes mode (``shard="owner"``, the default on GPUs): a rank keeps current only
    # its HALO — every slot its own offspring can draw as a parent (the union of its slots'
    # neighbourhoods).  It runs the replacement for the halo slots alone and copies each
    # halo slot's winning offspring row straight out of the memory of the rank that
    # generated it (IPC-mapped peer buffers, parallel/peer.py: one direct xGMI read per row,
    # no collective), instead of regenerating every winner of the whole population.  Rows
    # outside the halo go stale on that rank and are never read by it; the global z_max
    # comes from an all-reduce of the owners' slot maxima.  Per-rank work falls from
    # O(N·d) to O(|halo|·d) row updates + O(N·d / world) variation.
    rank_local_fields = ("next_generation",)
    # owner mode: rows outside a rank's halo go stale there (excluded from replica checks)
    rank_divergent_fields = ("population", "fitness", "win")
    shard = "auto"

    def _owner_mode(self, state, dist):
        if self.shard == "replica":
            return False
        return self.shard == "owner" or dist.world_size > 1 or getattr(dist, "backend", "") == "simulated"

    def _owner(self, state, dist):
        """Halo slots, offspring starts and the peer buffer of this rank (built once)."""
        cache = getattr(self, "_owner_cache", None)
        if cache is not None and cache["ctx"] is dist:
            return cache
        from ...parallel.context import balanced_slices
        from ...parallel.peer import PeerBuffer

        n = self.pop_size
        start, size = dist.slice_of(n)
        dev = state.population.device
        halo = self._halo(state, start, size)
        slices = balanced_slices(n, dist.world_size)
        starts = [a for a, _ in slices] + [n]
        rows = max(z for _, z in slices)
        cache = dict(ctx=dist, start=start, size=size, halo=halo.to(torch.int32).to(dev), halo_long=halo.to(dev),
                     starts=torch.tensor(starts, dtype=torch.int32, device=dev), starts_list=starts,
                     peer=PeerBuffer(dist, rows, self.dim, dev), win_h=torch.full((halo.numel(),), -1, dtype=torch.int32, device=dev),
                     first=torch.empty((self.pop_size,), dtype=torch.int32, device=dev),
                     offsets=torch.tensor([4 * a * self.dim for a in starts[:-1]], dtype=torch.int64, device=dev))
        self._owner_cache = cache
        return cache

    @staticmethod
    def _halo(state, start, size):
        """Sorted slots a rank owning [start, start + size) keeps current: its slots and every
        neighbour of them (the parents its offspring can draw)."""
        own_nb = state.neighbors[start : start + size].reshape(-1).to(torch.int64)
        return torch.unique(torch.cat([own_nb, torch.arange(start, start + size, device=own_nb.device)]))

    def halo_fraction(self, state, rank: int, world: int) -> float:
        """|halo| / N: the share of the population rank ``rank`` of ``world`` keeps current in
        owner mode."""
        from ...parallel.context import balanced_slices

        start, size = balanced_slices(self.pop_size, world)[rank]
        return float(self._halo(state, start, size).numel()) / self.pop_size

    def fresh_slots(self, state, dist):
        """Slots whose population / objective rows are current on this rank (all of them in
        replica mode)."""
        if self._owner_mode(state, dist):
            return self._owner(state, dist)["halo_long"]
        return torch.arange(self.pop_size, device=state.population.device)

    def init_ask_sharded(self, state, dist):
        start, size = dist.slice_of(self.pop_size)
        return state.population[start : start + size], state

    def init_tell_sharded(self, state, fitness, dist):
        return self.init_tell(state, fitness)

    def ask_sharded(self, state, dist):
        key, sub, sel_key, mut_key = rnd.split(state.key, 4)
        start, size = dist.slice_of(self.pop_size)
        owner = self._owner_mode(state, dist)
        # owner mode never regenerates another rank's offspring: its own rows' parents suffice
        parents = self._parent_pairs(state, sub, *((start, size) if owner else (0, 0)))
        if owner:
            ow = self._owner(state, dist)
            buf = ow["peer"].local[:size]  # the peers read this rank's offspring from here
            if self._fused(state.population):
                from ...ops import mo as mo_ops

                c, m = self.crossover, self.mutation
                off = mo_ops.moead_variation(state.population, parents[0].contiguous(), parents[1].contiguous(), sel_key, mut_key,
                                             self.lb, self.ub, c.pro_c, c.dis_c, m.pro_m, m.dis_m, row0=start, rows=size, out=buf)
            else:
                off = buf.copy_(self._offspring_rows(state, parents, sel_key, mut_key, row0=start, rows=size))
            ow["peer"].release()  # the peers read these rows after the next collective (peer.py contract)
        else:
            off = self._offspring_rows(state, parents, sel_key, mut_key, row0=start, rows=size)
        return off, state.update(next_generation=off, key=key, parents=parents, var_keys=torch.stack([sel_key, mut_key]))

    def tell_sharded(self, state, fitness, dist):
        if self._owner_mode(state, dist):
            return self._tell_owner(state, fitness, dist)
        win, new_obj, z = self._replace(state, fitness)
        new_pop = self._offspring_rows(state, state.parents, state.var_keys[0], state.var_keys[1], win=win)
        return state.update(population=new_pop, fitness=new_obj, z=z, win=win)

    def _tell_owner(self, state, fitness, dist):
        ow = self._owner(state, dist)
        start, size = ow["start"], ow["size"]
        z = torch.minimum(state.z, fitness.min(0).values)
        # global z_max from the owners' (always current) slots
        z_max = state.fitness[start : start + size].max(0).values.clone()
        dist.all_reduce_(z_max, op=torch.distributed.ReduceOp.MAX)
        obj = state.fitness.clone()
        pop = state.population  # halo rows are updated in place (a full copy would cost more than the update)
        halo = ow["halo"]
        if fitness.is_cuda and obj.dtype == torch.float32:
            from ...ops import mo as mo_ops

            rowptr, _, owner = self._reverse(state)
            if self._rev32 is None or self._rev32[0].data_ptr() != rowptr.data_ptr():
                self._rev32 = (rowptr, rowptr.to(torch.int32), owner.to(torch.int32))
            win_h = ow["win_h"]
            mo_ops.moead_halo_replace(obj, fitness, state.weight_vector, z, z_max, self._rev32[1], self._rev32[2], halo,
                                      self.func_name, win_h)
            table = ow["peer"].peer_table()
            first = ow["first"]
            if table is None:
                # no device IPC (single-process simulation, gloo): the offspring of every rank
                # as one buffer, then the same gather (pointer table built on the device:
                # capturable)
                full = dist.all_gather_rows(state.next_generation, self.pop_size).contiguous()
                table = torch.full_like(ow["offsets"], full.data_ptr()) + ow["offsets"]
                mo_ops.moead_halo_gather(pop, halo, win_h, table, ow["starts"], first)
                del full
            else:
                mo_ops.moead_halo_gather(pop, halo, win_h, table, ow["starts"], first)
                ow["peer"].fence()
            if getattr(dist, "backend", "") == "simulated":
                # wire accounting of the simulated rank: the distinct offspring generated on another
                # rank that win one of this rank's halo slots are the rows a real rank reads over
                # xGMI (each once: the gather is deduplicated); device-side count, no host sync
                gen_rank = torch.bucketize(win_h.to(torch.int64), ow["starts"][1:].to(torch.int64), right=True)
                h_idx = torch.arange(win_h.numel(), device=win_h.device, dtype=torch.int32)
                is_first = first[win_h.clamp_min(0).long()] == h_idx
                dist.count_peer_rows(((win_h >= 0) & (gen_rank != dist.rank) & is_first).sum(), self.dim * 4)
            win = torch.full((self.pop_size,), -1, dtype=torch.int32, device=obj.device)
            win.index_copy_(0, ow["halo_long"], win_h)
        else:
            win_all, new_obj = moead_replace(state.fitness, fitness, state.weight_vector, z, z_max, self.aggregate_func,
                                                self._reverse(state))
            hl = ow["halo_long"]
            win = torch.full((self.pop_size,), -1, dtype=torch.int32, device=obj.device)
            win[hl] = win_all[hl].to(torch.int32)
            obj[hl] = new_obj[hl]
            full = dist.all_gather_rows(state.next_generation, self.pop_size)
            take = hl[win[hl] >= 0]
            pop = pop.clone()
            pop[take] = full[win[take].long()]
        return state.update(population=pop, fitness=obj, z=z, win=win)


def cross_shard_winner_fraction(win: torch.Tensor, world: int):
    """(winners / N, fraction of winners generated on another rank than the slot's owner):
    the share of d-length rows a row-shipping design would move every generation."""
    from ...parallel.context import balanced_slices

    n = win.shape[0]
    owner = torch.empty(n, dtype=torch.int64)
    for r, (s, z) in enumerate(balanced_slices(n, world)):
        owner[s : s + z] = r
    w = win.cpu().long()
    has = w >= 0
    if not bool(has.any()):
        return 0.0, 0.0
    cross = owner[has] != owner[w[has]]
    return float(has.float().mean()), float(cross.float().mean())


def moead_replace_sequential(pop, pop_obj, off, off_obj, w, z, z_max, neighbors, agg):
    """Literal transcription of the reference scan (test oracle)."""
    pop, pop_obj = pop.clone(), pop_obj.clone()
    for i in range(off.shape[0]):
        idx = neighbors[i]
        f_old = agg(pop_obj[idx], w[idx], z, z_max)
        f_new = agg(off_obj[i][None, :], w[idx], z, z_max)
        upd = f_old > f_new
        pop[idx[upd]] = off[i]
        pop_obj[idx[upd]] = off_obj[i]
    return pop, pop_obj
