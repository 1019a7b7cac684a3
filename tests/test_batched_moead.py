"""BatchedRuns over MOEA/D on the CPU: every state field of run r equals, bit for bit, ``MOEAD`` alone from ``run_keys(key)[r]``
(``tell`` goes through the Python-registered run-by-run op of ``evoxmi/algorithms/mo/moead.py``)."""
import pytest
import torch

from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.moead import MOEAD
from evoxmi.problems.numerical import DTLZ2

from test_batched_ibea_spea2 import same_bits
from test_batched_mo import run

D, M, POP, RUNS = 12, 3, 91, 3
FUNCS = ["tchebycheff", "pbi", "weighted_sum", "modified_tchebycheff", "tchebycheff_norm"]
FIELDS = ("population", "fitness", "next_generation", "parents", "var_keys", "win", "z", "key", "weight_vector", "neighbors")


def make(func, dev):
    return MOEAD(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP, func_name=func)


def check_moead_runs_equal_solo(func, dev, runs=RUNS):
    prob = DTLZ2(d=D, m=M)
    pst = prob.init(rnd.PRNGKey(1, device=dev))
    key = rnd.PRNGKey(5, device=dev)
    b = BatchedRuns(make(func, dev), runs)
    bst = run(b, key, prob, pst, runs)
    assert bst.runs.population.shape == (runs, POP, D) and bst.runs.win.shape == (runs, POP) and bst.runs.win.dtype == torch.int32
    for r, k in enumerate(b.run_keys(key)):
        sst = run(make(func, dev), k, prob, pst)
        for name in FIELDS:
            assert same_bits(bst.runs[name][r], sst[name]), f"{func} run {r}: {name} differs"
    assert bool((bst.runs.win >= 0).any()) and not torch.equal(bst.runs.population[0], bst.runs.population[1])
    return bst


@pytest.mark.parametrize("func", FUNCS)
def test_batched_moead_runs_equal_solo_cpu(func):
    check_moead_runs_equal_solo(func, "cpu")
