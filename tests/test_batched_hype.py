"""BatchedRuns over HypE: run r of ``BatchedRuns(HypE(pop 20, n_sample 512), 3)`` on DTLZ2 (m 3, d 6) after four generations equals,
bit for bit, the solo workflow whose algorithm starts from ``split(key, 3)[r]`` (the device form: ``tests/test_batched_hype_gpu.py``)."""
import functools

import torch

from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.hype import HypE
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

D, M, POP, N_SAMPLE, RUNS, GENS = 6, 3, 20, 512, 3, 4


def final(dev, algo_key, runs=0, graph=False):
    """(population, fitness) after the initial evaluation and GENS generations of a workflow whose algorithm starts from ``algo_key``."""
    algo = HypE(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP, n_sample=N_SAMPLE)
    algo = BatchedRuns(algo, runs) if runs else algo
    wf = StdWorkflow(algo, DTLZ2(d=D, m=M), graph=graph)
    st = wf.init(rnd.PRNGKey(9, device=dev))
    st = st.update_child("algorithm", algo._recursive_init(algo_key, algo._node_id, algo._module_name, False)[0])
    for _ in range(GENS + 1):
        st = wf.step(st)
    ast = st.get_child_state("algorithm")
    ast = ast.runs if runs else ast
    return ast.population.clone(), ast.fitness.clone()


@functools.lru_cache(maxsize=None)
def solo_runs(dev):
    key = rnd.PRNGKey(5, device=dev)
    return key, [final(dev, k) for k in rnd.split(key, RUNS)]


def check_runs_equal_solo(dev, graph=False):
    key, solo = solo_runs(dev)
    pop, fit = final(dev, key, RUNS, graph)
    assert pop.shape == (RUNS, POP, D) and fit.shape == (RUNS, POP, M) and not torch.equal(pop[0], pop[1])
    for r, (p, f) in enumerate(solo):
        assert torch.equal(pop[r], p) and torch.equal(fit[r], f), f"run {r} differs from the solo run"


def test_batched_hype_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")
