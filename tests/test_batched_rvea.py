"""BatchedRuns over RVEA: run r of ``BatchedRuns(RVEA(pop 21), 3)`` on DTLZ2 (m 3, d 6) after twelve generations, which cross the
reference-vector adaptation of generation 10, equals the solo workflow whose algorithm starts from ``split(key, 3)[r]`` bit for bit,
NaN padding included; and ``ops.rvea.select`` on (B, n, m) is the 2-D call run by run (the device forms:
``tests/test_batched_rvea_gpu.py``)."""
import functools

import torch

import _rvea_reference as ref
from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.rvea import RVEA
from evoxmi.ops import rvea as rvea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

D, M, POP, RUNS, GENS = 6, 3, 21, 3, 12


def final(dev, algo_key, runs=0, graph=False):
    """(population, fitness, reference_vector) after the initial evaluation and GENS generations of a workflow whose algorithm starts
    from ``algo_key``."""
    algo = RVEA(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)
    algo = BatchedRuns(algo, runs) if runs else algo
    wf = StdWorkflow(algo, DTLZ2(d=D, m=M), graph=graph)
    st = wf.init(rnd.PRNGKey(9, device=dev))
    st = st.update_child("algorithm", algo._recursive_init(algo_key, algo._node_id, algo._module_name, False)[0])
    for _ in range(GENS + 1):
        st = wf.step(st)
    ast = st.get_child_state("algorithm")
    ast = ast.runs if runs else ast
    assert int(ast.gen.reshape(-1)[0]) == GENS
    return ast.population.clone(), ast.fitness.clone(), ast.reference_vector.clone()


@functools.lru_cache(maxsize=None)
def solo_runs(dev):
    key = rnd.PRNGKey(5, device=dev)
    return key, [final(dev, k) for k in rnd.split(key, RUNS)]


def same_bits(a, b):
    """Equal, a NaN equal to a NaN."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def check_runs_equal_solo(dev, graph=False):
    key, solo = solo_runs(dev)
    pop, fit, vec = final(dev, key, RUNS, graph)
    assert pop.shape == (RUNS, POP, D) and fit.shape == (RUNS, POP, M) and vec.shape == (RUNS, POP, M) and not same_bits(pop[0], pop[1])
    assert not torch.equal(vec[0], vec[1]), "the adaptation did not give the runs their own vectors"
    for r, (p, f, v) in enumerate(solo):
        assert same_bits(pop[r], p) and same_bits(fit[r], f) and same_bits(vec[r], v), f"run {r} differs from the solo run"


def test_batched_rvea_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")


def test_select_on_runs_is_the_2d_select_run_by_run_cpu():
    fs, vs = zip(*(ref.to_torch(ref.objectives(40, 3, 0.25, s), ref.vectors(20, 3, "rand", s)) for s in range(3)))
    f, v, theta = torch.stack(fs), torch.stack(vs), torch.tensor([0.0, 0.3, 1.0])
    per_run, shared, scalar = rvea_ops.select(f, v, theta), rvea_ops.select(f, v[0], theta), rvea_ops.select(f, v, 0.3)
    assert per_run[0].shape == per_run[1].shape == (3, 20) and not per_run[1].all()
    for r in range(3):
        assert all(torch.equal(x[r], y) for x, y in zip(per_run, rvea_ops.select(f[r], v[r], theta[r])))
        assert all(torch.equal(x[r], y) for x, y in zip(shared, rvea_ops.select(f[r], v[0], theta[r])))
        assert all(torch.equal(x[r], y) for x, y in zip(scalar, rvea_ops.select(f[r], v[r], torch.tensor(0.3))))
