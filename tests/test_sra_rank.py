"""``evoxmi.ops.sra`` on the CPU: the public functions are the host op and the dense torch
expressions, and ``SRA`` on the CPU computes bit for bit what it computed before the device
kernels (``sra_select.hip``) were added."""
import torch

import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.ops import _ext
from evoxmi.ops import sra as sra_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.utils.common import cal_max
from evoxmi.workflows import StdWorkflow


def _sde_distance(obj):
    n = obj.shape[0]
    d = torch.sqrt((torch.clamp(obj[None, :, :] - obj[:, None, :], min=0) ** 2).sum(-1))
    return d.masked_fill(torch.eye(n, dtype=torch.bool), float("inf")).min(1).values


def test_stochastic_rank_takes_a_tensor_pc():
    gen = torch.Generator().manual_seed(0)
    for n in (1, 2, 5, 64, 201):
        I1, I2, u = torch.rand(n, generator=gen), torch.rand(n, generator=gen), torch.rand(max(n - 1, 0), generator=gen)
        for pc in (0.4, 0.5, 0.6):
            pct = torch.tensor(pc, dtype=torch.float32)
            want = _ext.ops().stochastic_ranking(I1, I2, u, float(pct))
            assert torch.equal(sra_ops.stochastic_rank(I1, I2, u, pct), want)
            assert torch.equal(sra_ops.stochastic_rank(I1, I2, u, float(pct)), want)
            assert sorted(want.tolist()) == list(range(n))


def test_indicators_on_the_cpu_are_the_torch_expressions():
    obj = torch.rand(50, 3, generator=torch.Generator().manual_seed(1))
    I1, I2 = sra_ops.indicators(obj)
    assert torch.equal(I1, (-torch.exp(-cal_max(obj, obj) / 0.05)).sum(0) + 1)
    assert torch.equal(I2, _sde_distance(obj))


class _ParentSRA(A.SRA):
    """``tell`` as it stood before ``evoxmi.ops.sra``: dense indicators, pc read on the host, the host op."""

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_fit = torch.cat([state.fitness, fitness], 0)
        key, k_pc, k_env = rnd.split(state.key, 3)
        pc = float(rnd.uniform(k_pc, ())) * 0.2 + 0.4
        I = cal_max(merged_fit, merged_fit)
        I1 = (-torch.exp(-I / 0.05)).sum(0) + 1
        I2 = _sde_distance(merged_fit)
        u = rnd.uniform(k_env, (merged_fit.shape[0] - 1,))
        idx = _ext.ops().stochastic_ranking(I1, I2, u, float(pc))[: self.pop_size]
        return state.update(population=merged_pop[idx], fitness=merged_fit[idx], key=key)


def test_sra_on_the_cpu_is_unchanged():
    d, m, pop = 6, 3, 20

    def run(cls):
        wf = StdWorkflow(cls(torch.zeros(d), torch.ones(d), m, pop), DTLZ2(d=d, m=m))
        st = wf.init(rnd.PRNGKey(3))
        for _ in range(5):
            st = wf.step(st)
        return st.get_child_state("algorithm")

    a, b = run(A.SRA), run(_ParentSRA)
    assert torch.equal(a.population, b.population)
    assert torch.equal(a.fitness, b.fitness)
    assert torch.equal(a.key, b.key)
