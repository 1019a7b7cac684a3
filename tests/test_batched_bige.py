"""BatchedRuns over BiGE: run r of ``BatchedRuns(BiGE(pop 20), 3)`` on DTLZ2 (m 3, d 6) after eight generations equals the solo
workflow whose algorithm starts from ``split(key, 3)[r]`` bit for bit; ``ops.bige.estimate_rank`` on (B, n, m) is the 2-D call run by
run; and no fixture of the device test (``tests/test_batched_bige_gpu.py``, which takes ``SHAPES`` and ``runs_of`` from here) has a
``d < r`` decision at the rounding edge."""
import functools

import numpy as np
import pytest
import torch

import _bige_reference as ref
from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.bige import BiGE
from evoxmi.ops import bige as bige_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

D, M, POP, RUNS, GENS = 6, 3, 20, 3, 8

# (B, n, m), the runs' masks: one row; two rows; past one 64-lane pass; rows no multiple of the 16 waves, with an empty mask; MC = 8;
# MC = 16; two owned rows per thread in the peel; the three caps
SHAPES = [((1, 1, 2), ("all",)), ((2, 2, 2), ("all", "one")), ((2, 65, 3), ("all", "every7")), ((3, 130 + 5, 3), ("none", "every7", "all")),
          ((2, 70, 5), ("every7", "all")), ((2, 40, 16), ("all", "every7")), ((2, 1030, 3), ("every7", "all")),
          ((2, 2048, 3), ("all", "every7")), ((2, 1024, 8), ("every7", "all")), ((2, 512, 16), ("all", "every7"))]


def runs_of(shape, mask_names):
    """fit (B, n, m) float32 and mask (B, n): the runs differ in seed, kind and mask, and the last repeats its first rows in its last."""
    B, n, m = shape
    fit = np.stack([ref.objectives(n, m, ("front", "uniform")[r % 2], 7 * r + n) for r in range(B)])
    k = max(1, min(8, n // 4))
    fit[-1, n - k:] = fit[-1, :k]
    return fit, np.stack([ref.masks(n)[name] for name in mask_names])


def final(dev, algo_key, runs=0, graph=False):
    """(population, fitness) after the initial evaluation and GENS generations of a workflow whose algorithm starts from ``algo_key``."""
    algo = BiGE(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)
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


def test_batched_bige_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")


def test_estimate_rank_on_runs_is_the_2d_call_run_by_run_cpu():
    fit = torch.stack([torch.from_numpy(ref.objectives(40, 3, kind, s)) for s, kind in enumerate(("front", "uniform", "front"))])
    mask = torch.stack([torch.from_numpy(ref.masks(40)[name]) for name in ("all", "every7", "one")])
    bi, rank = bige_ops.estimate_rank(fit, mask)
    assert bi.shape == (3, 40, 2) and bi.dtype == torch.float32 and rank.shape == (3, 40) and rank.dtype == torch.int32
    for r in range(3):
        want_bi, want_rank = bige_ops.estimate_rank(fit[r], mask[r])
        assert torch.equal(bi[r], want_bi) and torch.equal(rank[r], want_rank)


@pytest.mark.parametrize("shape,mask_names", SHAPES)
def test_no_fixture_decides_at_the_rounding_edge(shape, mask_names):
    fit, mask = runs_of(shape, mask_names)
    for r in range(shape[0]):
        gap = ref.estimate(fit[r], mask[r], ref.radius(mask[r], shape[2]))[3]
        assert gap > 1e-9, f"run {r}: thr_gap {gap:.3e}"
