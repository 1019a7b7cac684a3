"""BatchedRuns over SRA: run r of ``BatchedRuns(SRA(pop 20), 3)`` on DTLZ2 (m 3, d 6) after six generations equals the solo workflow
whose algorithm starts from ``split(key, 3)[r]`` bit for bit; and ``ops.sra.select`` on (B, n, m) is the 2-D call run by run (the
device forms: ``tests/test_batched_sra_gpu.py``)."""
import functools

import torch

from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.sra import SRA
from evoxmi.ops import sra as sra_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

D, M, POP, RUNS, GENS = 6, 3, 20, 3, 6


def final(dev, algo_key, runs=0, graph=False):
    """(population, fitness) after the initial evaluation and GENS generations of a workflow whose algorithm starts from ``algo_key``."""
    algo = SRA(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)
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
    assert bool(torch.isfinite(fit).all())
    for r, (p, f) in enumerate(solo):
        assert torch.equal(pop[r], p) and torch.equal(fit[r], f), f"run {r} differs from the solo run"


def test_batched_sra_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")


def test_select_on_runs_is_the_2d_select_run_by_run_cpu():
    gen = torch.Generator().manual_seed(3)
    obj, u, pc = torch.rand(3, 40, 3, generator=gen), torch.rand(3, 39, generator=gen), torch.tensor([0.0, 0.45, 1.0])
    per_run, scalar = sra_ops.select(obj, u, pc, return_info=True), sra_ops.select(obj, u, 0.45)
    assert [tuple(t.shape) for t in per_run] == [(3, 40)] * 3 and per_run[0].dtype == torch.int64 and scalar.shape == (3, 40)
    for r in range(3):
        assert all(torch.equal(x[r], y) for x, y in zip(per_run, sra_ops.select(obj[r], u[r], pc[r], return_info=True)))
        assert torch.equal(scalar[r], sra_ops.select(obj[r], u[r], 0.45))
        assert sorted(per_run[0][r].tolist()) == list(range(40))
