"""BatchedRuns over NSGA-II and GDE3 on the CPU: R independent runs as one vmapped computation
must equal, bit for bit, the algorithm run alone from ``run_keys(key)[r]``.  The environmental
selection has data-dependent control flow on the CPU, so under ``vmap`` it goes through a
Python-registered op whose rule applies the torch path run by run (``evoxmi/ops/nds.py``): by
construction the sequential result, and the oracle the device kernels are held to in
``tests/test_batched_mo_gpu.py``."""
import pytest
import torch

from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.gde3 import GDE3
from evoxmi.algorithms.mo.nsga2 import NSGA2
from evoxmi.operators.selection import non_dominated_sort
from evoxmi.problems.numerical import DTLZ2

D, M, POP, RUNS, GENS = 12, 3, 20, 3, 6
ALGOS = {"NSGA2": NSGA2, "GDE3": GDE3}


def make(name, dev):
    return ALGOS[name](torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)


def run(algo, key, prob, pst, runs=1):
    """GENS generations; a batched algorithm's (runs·pop, d) population is evaluated block by block,
    so every run's rows see exactly the launch shape of a solo run."""
    evaluate = lambda pop: torch.cat([prob.evaluate(pst, blk)[0] for blk in pop.chunk(runs)])
    st = algo.init(key)
    pop, st = algo.init_ask(st)
    st = algo.init_tell(st, evaluate(pop))
    for _ in range(GENS):
        pop, st = algo.ask(st)
        st = algo.tell(st, evaluate(pop))
    return st


def check_runs_equal_solo(name, dev):
    prob = DTLZ2(d=D, m=M)
    pst = prob.init(rnd.PRNGKey(1, device=dev))
    key = rnd.PRNGKey(5, device=dev)
    b = BatchedRuns(make(name, dev), RUNS)
    bst = run(b, key, prob, pst, RUNS)
    assert bst.runs.population.shape == (RUNS, POP, D) and bst.runs.fitness.shape == (RUNS, POP, M)
    for r, k in enumerate(b.run_keys(key)):
        sst = run(make(name, dev), k, prob, pst)
        assert torch.equal(bst.runs.population[r], sst.population), f"{name} run {r}: population differs"
        assert torch.equal(bst.runs.fitness[r], sst.fitness), f"{name} run {r}: fitness differs"
    # the runs are independent: different keys, different populations
    assert not torch.equal(bst.runs.population[0], bst.runs.population[1])
    return bst


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_batched_mo_runs_equal_solo_cpu(name):
    check_runs_equal_solo(name, "cpu")


@pytest.mark.parametrize("until", [0, 7, 30])
def test_non_dominated_sort_3d_cpu(until):
    g = torch.Generator().manual_seed(3)
    f = torch.rand(4, 30, 3, generator=g)
    f[1] = torch.arange(30.0)[:, None].expand(30, 3)  # a chain: 30 fronts
    f[2, 5] = f[2, 6]  # a duplicated row
    f[3, 4] = float("nan")
    f[3, 9] = float("inf")
    out = non_dominated_sort(f, until=until)
    assert out.shape == (4, 30) and out.dtype == torch.int32
    for b in range(4):
        assert torch.equal(out[b], non_dominated_sort(f[b], until=until))
    assert torch.equal(out[1], torch.arange(30, dtype=torch.int32))
