"""BatchedRuns over θ-DEA: run r of ``BatchedRuns(TDEA(pop 21), 3)`` on DTLZ2 (m 3, d 6) after eight generations equals the solo
workflow whose algorithm starts from ``split(key, 3)[r]`` bit for bit; and ``ops.tdea.theta_rank`` on (B, n, m) is the 2-D call run by
run (the device forms: ``tests/test_batched_tdea_gpu.py``)."""
import functools

import torch

import _rvea_reference as rv
import _tdea_reference as ref
from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.tdea import TDEA
from evoxmi.ops import tdea as tdea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

D, M, POP, RUNS, GENS = 6, 3, 21, 3, 8


def final(dev, algo_key, runs=0, graph=False):
    """(population, fitness) after the initial evaluation and GENS generations of a workflow whose algorithm starts from ``algo_key``."""
    algo = TDEA(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)
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
    assert torch.isfinite(fit).all()
    for r, (p, f) in enumerate(solo):
        assert torch.equal(pop[r], p) and torch.equal(fit[r], f), f"run {r} differs from the solo run"


def test_batched_tdea_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")


def test_theta_rank_on_runs_is_the_2d_call_run_by_run_cpu():
    obj = torch.stack([torch.from_numpy(ref.objectives(40, 3, kind, s)) for s, kind in enumerate(("front", "uniform", "front"))])
    w = torch.stack([torch.from_numpy(rv.vectors(20, 3, "rand", s)) for s in range(3)])
    mask = torch.stack([torch.from_numpy(ref.masks(40)[name]) for name in ("all", "every7", "one")])
    per_run, shared = tdea_ops.theta_rank(obj, w, mask), tdea_ops.theta_rank(obj, w[1], mask)
    assert per_run.shape == shared.shape == (3, 40) and per_run.dtype == torch.float32
    for r in range(3):
        assert torch.equal(per_run[r], tdea_ops.theta_rank(obj[r], w[r], mask[r]))
        assert torch.equal(shared[r], tdea_ops.theta_rank(obj[r], w[1], mask[r]))
