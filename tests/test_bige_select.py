"""``ops.bige.estimate`` on the CPU: the host reference of the kernels' contract (``_bige_reference.py``) against the
dense float32 torch expression, the dispatch, and BiGE's seeded trajectory.

Reference against the torch path, every 7th row outside the mask.  ``pr`` is within 4e-7 relative: the float32 sum of
m ≤ 16 terms bounds it.  For ``cd`` the difference is set by ``cdist``'s float32 matrix-product form, not by the
reference, so the bound of every shape is 4× the largest absolute difference observed on the CPU at that shape.
``thr_gap``, the smallest relative distance of a pair from the radius r, is asserted at ≥ 1e-6: no ``d < r`` decision of
these fixtures hangs on the last bits of a float64 distance.

Observed (CPU, float32 torch path against the float64 reference):

================  =========  ===========  ===========  =========
shape, kind       pr rel     cd absolute  bound (4×)   thr_gap
================  =========  ===========  ===========  =========
(257, 3) uniform  1.06e-7    3.30e-5      2.1e-4       4.03e-4
(257, 3) front    1.22e-7    5.06e-5      2.1e-4       9.97e-5
(1000, 10) unif.  1.87e-7    4.27e-5      1.8e-4       7.69e-4
(1000, 10) front  2.21e-7    1.38e-5      1.8e-4       3.30e-5
(1000, 5) unif.   1.38e-7    2.37e-5      1.0e-4       1.92e-5
(1000, 5) front   1.32e-7    1.39e-5      1.0e-4       2.48e-5
(2049, 3) unif.   1.18e-7    1.73e-4      4.1e-3       1.60e-4
(2049, 3) front   1.13e-7    1.02e-3      4.1e-3       4.60e-6
(2049, 2) unif.   1.09e-7    2.66e-3      6.6e-1       2.23e-5
(2049, 2) front   8.14e-8    1.65e-1      6.6e-1       6.80e-6
================  =========  ===========  ===========  =========

(At (2049, 2) the front is a curve of 1757 points inside a radius of 0.024: the matrix-product form of ``cdist`` loses
the close distances, and a crowding degree of about 30 moves by 0.17.)"""
import numpy as np
import pytest
import torch

import _bige_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import bige as bige_algo
from evoxmi.operators.selection.non_dominate import non_dominated_sort
from evoxmi.ops import bige as bige_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

# shape → the largest |cd_torch − cd_reference| observed over both kinds (the table above)
CD_OBSERVED = {(257, 3): 5.06e-5, (1000, 10): 4.27e-5, (1000, 5): 2.37e-5, (2049, 3): 1.02e-3, (2049, 2): 1.65e-1}


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", list(CD_OBSERVED))
def test_reference_against_the_torch_path(n, m, kind):
    fit = ref.cached_objectives(n, m, kind, 100 * n + m)
    mask = ref.masks(n)["every7"]
    bi, pr, cd, gap = ref.estimate(fit, mask, ref.radius(mask, m))
    got = bige_algo.estimate(torch.tensor(np.array(fit)), torch.tensor(mask)).numpy()
    assert np.isinf(got[~mask]).all() and np.isinf(bi[~mask]).all() and (bi[~mask] > 0).all()
    t = got[mask].astype(np.float64)
    e_pr = float(np.max(np.abs(t[:, 0] - pr[mask]) / np.abs(pr[mask])))
    e_cd = float(np.max(np.abs(t[:, 1] - cd[mask])))
    print(f"[bige cpu] ({n}, {m}) {kind}: pr rel {e_pr:.3e}, cd abs {e_cd:.3e} (bound {4 * CD_OBSERVED[(n, m)]:.3e}), thr_gap {gap:.3e}")
    assert gap >= 1e-6
    assert e_pr <= 4e-7
    assert e_cd <= 4 * CD_OBSERVED[(n, m)]
    assert np.array_equal(bi[mask], np.stack([pr[mask], cd[mask]], 1).astype(np.float32))


def test_reference_edges():
    fit = ref.objectives(65, 2, "uniform", 3)
    m = ref.masks(65)
    bi, pr, cd, gap = ref.estimate(fit, m["none"], ref.radius(m["none"], 2))
    assert np.isinf(bi).all() and np.isinf(pr).all() and np.isinf(cd).all() and gap == float("inf")
    bi, pr, cd, _ = ref.estimate(fit, m["one"], ref.radius(m["one"], 2))
    assert ref.radius(m["one"], 2) == 1.0
    assert pr[32] == 0.0 and cd[32] == 0.0 and np.isinf(np.delete(bi, 32, 0)).all()
    # a block of equal rows: w = 2 and d = 0, every pair contributes exactly 1
    f = ref.objectives(300, 3, "front", 6).copy()
    f[100:150] = f[100]
    mask = np.ones(300, dtype=bool)
    _, _, cd, _ = ref.estimate(f, mask, ref.radius(mask, 3))
    assert (cd[100:150] ** 2 >= 49).all() and np.unique(cd[100:150]).size == 1


def test_dispatch_on_the_cpu_and_outside_the_kernel_types():
    for n, m, dtype in [(200, 3, torch.float32), (50, bige_ops.M_CAP + 1, torch.float32), (200, 3, torch.float64)]:
        fit = torch.tensor(ref.objectives(n, m, "uniform", 1)).to(dtype)
        mask = torch.tensor(ref.masks(n)["every7"])
        assert torch.equal(bige_ops.estimate(fit, mask), bige_algo.estimate(fit, mask))
    assert bige_ops.N_CAP == 32768 and bige_ops.M_CAP == 16
    assert not bige_ops.on_device(100, 3, "cpu") and bige_ops.on_device(bige_ops.N_CAP, bige_ops.M_CAP, "cuda")
    assert not bige_ops.on_device(bige_ops.N_CAP + 1, 3, "cuda") and not bige_ops.on_device(100, bige_ops.M_CAP + 1, "cuda")
    assert not bige_ops.on_device(0, 3, "cuda")
    with pytest.raises(ValueError):
        bige_ops.estimate(torch.rand(10, 3), torch.ones(10, dtype=torch.bool), return_parts=True)


def _frozen_estimate(fit, mask):
    n = mask.sum().to(torch.float32)
    m = fit.shape[1]
    r = 1 / n ** (1 / m)
    big = torch.full_like(fit, float("inf"))
    f_max = torch.where(mask[:, None], fit, -big).max(0).values
    f_min = torch.where(mask[:, None], fit, big).min(0).values
    normed = (fit - f_min) / (f_max - f_min).clamp(min=1e-6)
    normed = torch.where(mask[:, None], normed, torch.full_like(normed, float(m)))
    pr = normed.sum(1)
    dis = torch.cdist(normed, normed)
    ge = (pr[:, None] >= pr[None, :]).to(fit.dtype)
    gt = (pr[:, None] > pr[None, :]).to(fit.dtype)
    sh = ((dis < r).to(fit.dtype) * 0.5 * ((1 + ge + gt) * (1 - dis / r))) ** 2
    cd = torch.sqrt(torch.clamp(sh.sum(1) - sh.diagonal(), min=0))
    bi = torch.stack([pr, cd], 1)
    return torch.where(mask[:, None], bi, torch.full_like(bi, float("inf")))


class _FrozenBiGE(A.BiGE):
    """BiGE with the estimate it called before ``ops.bige`` existed, inlined."""

    def ask(self, state):
        k0, k1, k2, k3 = rnd.split(state.key, 4)
        bi = _frozen_estimate(state.fitness, torch.ones(self.pop_size, dtype=torch.bool, device=state.fitness.device))
        selected, _ = self.selection(k1, state.population, non_dominated_sort(bi).to(torch.float32))
        off = self._variation(k2, k3, selected)
        return off, state.update(next_generation=off, key=k0)

    def tell(self, state, fitness):
        merged_pop = torch.cat([state.population, state.next_generation], 0)
        merged_fit = torch.cat([state.fitness, fitness], 0)
        rank = non_dominated_sort(merged_fit)
        order = torch.argsort(rank, stable=True)
        rank, pop, fit = rank[order], merged_pop[order], merged_fit[order]
        last = rank[self.pop_size]
        bi_rank = non_dominated_sort(_frozen_estimate(fit, rank == last))
        fin = torch.where(rank >= last, bi_rank, torch.full_like(bi_rank, -1))
        idx = torch.argsort(fin, stable=True)[: self.pop_size]
        return state.update(population=pop[idx], fitness=fit[idx])


def _run(cls, gens=5, seed=11):
    lb, ub = torch.zeros(12), torch.ones(12)
    wf = StdWorkflow(cls(lb, ub, 3, 100), DTLZ2(d=12, m=3), graph=False)
    st = wf.init(rnd.PRNGKey(seed))
    for _ in range(gens):
        st = wf.step(st)
    return st.get_child_state("algorithm")


def test_the_cpu_trajectory_has_not_moved():
    a, b = _run(A.BiGE), _run(_FrozenBiGE)
    assert torch.isfinite(a.fitness).all()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
