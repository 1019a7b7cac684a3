"""``evoxmi.ops.ibea`` on the CPU: the public fitness / select entry points are the dense torch
expressions IBEA and BCE-IBEA used before them, bit for bit, and both algorithms compute what
they computed with ``cal_fitness`` / ``ibea_truncate`` / a stable argsort written out in their
``ask`` and ``tell``."""
import pytest
import torch

import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import bce_ibea as bce_mod
from evoxmi.algorithms.mo.ibea import cal_fitness, ibea_truncate
from evoxmi.ops import ibea as ibea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

KAPPA = 0.05


def _objectives(n, m, kind="uniform"):
    obj = torch.rand(n, m, generator=torch.Generator().manual_seed(100 * n + m))
    if kind == "front":
        obj = obj / obj.sum(1, keepdim=True)
    return obj


def _present_select(obj, kappa, n_keep):
    f, I, C = cal_fitness(obj, kappa)
    keep = ibea_truncate(f, I, C, kappa, obj.shape[0] - n_keep)
    return torch.argsort((~keep).to(torch.int64), stable=True)[:n_keep]


def test_caps():
    assert ibea_ops.N_CAP == 8192 and ibea_ops.M_CAP == 16
    assert not ibea_ops.on_device(100, 3, "cpu")
    assert ibea_ops.on_device(8192, 16, "cuda") and not ibea_ops.on_device(8193, 3, "cuda") and not ibea_ops.on_device(100, 17, "cuda")


@pytest.mark.parametrize("n,m", [(50, 3), (201, 2), (1, 2)])
def test_fitness_is_cal_fitness(n, m):
    obj = _objectives(n, m)
    want = cal_fitness(obj, KAPPA)
    f, C = ibea_ops.fitness(obj, KAPPA)
    assert torch.equal(f, want[0]) or (n == 1 and torch.isnan(f).all() and torch.isnan(want[0]).all())
    assert torch.equal(C, want[2])


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", [(50, 3), (201, 2)])
def test_select_is_the_present_selection(n, m, kind):
    obj = _objectives(n, m, kind)
    want = _present_select(obj, KAPPA, n // 2)
    got = ibea_ops.select(obj, KAPPA, n // 2)
    assert got.dtype == torch.int64 and torch.equal(got, want)


@pytest.mark.parametrize("n,m", [(50, 3), (201, 2)])
def test_return_order_marks_the_complement(n, m):
    obj = _objectives(n, m, "front")
    n_keep = n // 2
    idx, order = ibea_ops.select(obj, KAPPA, n_keep, return_order=True)
    assert order.dtype == torch.int64 and order.shape == (n - n_keep,)
    assert torch.equal(idx, ibea_ops.select(obj, KAPPA, n_keep))
    assert order.unique().numel() == order.numel()  # no row is removed twice on this input
    assert torch.equal(torch.cat([idx, order]).sort().values, torch.arange(n))


def test_edge_cases():
    obj = _objectives(7, 3)
    for n_keep in (7, 9):
        idx, order = ibea_ops.select(obj, KAPPA, n_keep, return_order=True)
        assert torch.equal(idx, torch.arange(7)) and idx.dtype == torch.int64 and order.shape == (0,) and order.dtype == torch.int64
        assert torch.equal(ibea_ops.select(obj, KAPPA, n_keep), torch.arange(7))
    one = _objectives(1, 3)
    assert torch.equal(ibea_ops.select(one, KAPPA, 1), torch.arange(1))
    idx, order = ibea_ops.select(one, KAPPA, 0, return_order=True)  # one step on the only row
    assert idx.shape == (0,) and torch.equal(order, torch.zeros(1, dtype=torch.int64))
    none = torch.zeros(0, 3)
    for n_keep in (0, 4):
        idx, order = ibea_ops.select(none, KAPPA, n_keep, return_order=True)
        assert idx.shape == (0,) and idx.dtype == torch.int64 and order.shape == (0,)


# ---------------------------------------------------------------- the algorithms, as they stood
class _ParentIBEA(A.IBEA):
    def ask(self, state):
        key, sel_key, x_key, mut_key = rnd.split(state.key, 4)
        fit = cal_fitness(state.fitness, self.kappa)[0]
        selected, _ = self.selection(sel_key, state.population, -fit)
        off = self._variation(x_key, mut_key, selected, clip=False)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_obj = torch.cat([state.fitness, fitness], 0)
        f, I, C = cal_fitness(merged_obj, self.kappa)
        keep = ibea_truncate(f, I, C, self.kappa, merged_obj.shape[0] - self.pop_size)
        idx = torch.argsort((~keep).to(torch.int64), stable=True)[: self.pop_size]
        return state.update(population=merged_pop[idx], fitness=merged_obj[idx])


def _parent_ibea_selection(pop, obj, n, kappa):
    f, I, C = cal_fitness(obj, kappa)
    keep = ibea_truncate(f, I, C, kappa, obj.shape[0] - n)
    idx = torch.argsort((~keep).to(torch.int64), stable=True)[:n]
    return pop[idx], obj[idx]


class _ParentBCEIBEA(A.BCEIBEA):
    def ask(self, state):
        key, k1, x_key, mut_key = rnd.split(state.key, 4)
        N = self.pop_size
        if state.counter % 2 == 0:  # IBEA variation on NPC
            fit = -cal_fitness(state.npc_obj, self.kappa)[0]
            selected, _ = self.selection(k1, state.npc, fit)
            off = self.mutation(mut_key, self.crossover(x_key, selected))
        else:  # PC exploration
            s = bce_mod.exploration(state.fitness, state.npc_obj, state.n_nd, N)
            if bool(s.any()):
                cand = torch.nonzero(s).flatten()
                mate = rnd.randint(k1, (N,), 0, N).to(cand.device)
                first = cand[torch.arange(N, device=cand.device) % cand.shape[0]]
                parents = torch.cat([state.population[first], state.population[mate]])
                off = self.mutation(mut_key, self.crossover_odd(x_key, parents))
            else:
                off = state.population.clone()
        off = torch.clamp(off, self.lb, self.ub)
        return off, state.update(next_generation=off, key=key)

    def tell(self, state, fitness):
        N = self.pop_size
        npc, npc_obj = _parent_ibea_selection(torch.cat([state.npc, state.next_generation]), torch.cat([state.npc_obj, fitness]), N,
                                              self.kappa)
        pc, pc_obj, n_nd = bce_mod.pc_selection(torch.cat([state.population, state.next_generation]),
                                                torch.cat([state.fitness, fitness]), N)
        return state.update(population=pc, fitness=pc_obj, npc=npc, npc_obj=npc_obj, n_nd=n_nd, counter=state.counter + 1)


def _generations(cls, gens=5):
    d, m, pop = 6, 3, 20
    wf = StdWorkflow(cls(torch.zeros(d), torch.ones(d), m, pop), DTLZ2(d=d, m=m))
    st = wf.init(rnd.PRNGKey(3))
    for _ in range(gens):
        st = wf.step(st)
    return st.get_child_state("algorithm")


@pytest.mark.parametrize("now,parent", [(A.IBEA, _ParentIBEA), (A.BCEIBEA, _ParentBCEIBEA)])
def test_algorithm_is_unchanged_on_the_cpu(now, parent):
    a, b = _generations(now), _generations(parent)
    assert torch.equal(a.population, b.population)
    assert torch.equal(a.fitness, b.fitness)
    assert torch.equal(a.key, b.key)
    if now is A.BCEIBEA:
        assert torch.equal(a.npc, b.npc) and torch.equal(a.npc_obj, b.npc_obj)
