"""``ops.tdea.theta_rank`` on the CPU: the host reference of the kernels' contract (``_tdea_reference.py``) against the
dense float32 ``theta_nd_sort``, the dispatch, and θ-DEA's seeded trajectory.

Reference against ``theta_nd_sort``, n = 2·nw rows, every 7th row outside the mask.  The two differ where float32
rounds a cosine, ``sqrt(1 − c²)`` or ``val`` another way: a row then joins a neighbouring direction or swaps places
with a neighbour inside its cluster.  The share of rows with equal rank is ≥ 0.99 per case, and within every cluster
both rankings hold the ranks 1 … c.  Observed: 1.0 in every case of the list."""
import numpy as np
import pytest
import torch

import _tdea_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import tdea as tdea_algo
from evoxmi.operators.selection.non_dominate import lexsort, non_dominated_sort
from evoxmi.ops import rvea as rvea_ops
from evoxmi.ops import tdea as tdea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.utils.common import cos_dist
from evoxmi.workflows import StdWorkflow

SHAPES = [(91, 3), (300, 3), (210, 5), (1035, 3), (220, 10)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("N,m", SHAPES)
def test_reference_against_theta_nd_sort(N, m, kind):
    obj, w, cls, val = ref.cached_case(N, m, kind)
    n, nw = obj.shape[0], w.shape[0]
    assert n == 2 * nw
    mask = ref.masks(n)["every7"]
    want = ref.rank(cls, val, mask)
    got = tdea_algo.theta_nd_sort(torch.tensor(np.array(obj)), torch.tensor(np.array(w)), torch.tensor(mask)).numpy()
    share = float(np.mean(got == want))
    print(f"[tdea cpu] ({N}, {m}) {kind}: nw {nw}, n {n}, share of equal ranks {share:.4f}")
    assert np.isinf(got[~mask]).all() and np.isinf(want[~mask]).all()
    assert ref.clusters_are_ranked(cls, want, mask, nw)
    assert share >= 0.99
    # the disagreeing rows: their ranks are permutations within their clusters
    for j in np.unique(cls[got != want]):
        rows = mask & (cls == j)
        assert np.array_equal(np.sort(got[rows]), np.sort(want[rows]))


def test_reference_edges():
    obj, w, cls, val = ref.cached_case(91, 3, "front")
    n = obj.shape[0]
    m = ref.masks(n)
    assert np.isinf(ref.rank(cls, val, m["none"])).all()
    one = ref.rank(cls, val, m["one"])
    assert one[n // 2] == 1.0 and np.isinf(np.delete(one, n // 2)).all()
    # equal values: the position decides; a NaN orders after every number
    c = np.zeros(5, dtype=np.int64)
    v = np.array([2.0, np.nan, 1.0, 2.0, np.nan])
    assert ref.rank(c, v, np.ones(5, dtype=bool)).tolist() == [2.0, 4.0, 1.0, 3.0, 5.0]
    # a zero row and a NaN row
    o = np.array(obj[:20]).copy()
    o[3] = 0.0
    o[7, 1] = np.nan
    t, cl, _ = ref.theta_rank(o, w, np.ones(20, dtype=bool))
    assert ref.clusters_are_ranked(cl, t, np.ones(20, dtype=bool), w.shape[0])
    # θ: 1e6 on the axes
    th = ref.theta_of(w)
    assert int((th == 1e6).sum()) == 3 and set(th.tolist()) == {5.0, 1e6}
    assert np.array_equal(th, tdea_ops.theta_of(torch.tensor(np.array(w))).numpy())


def test_dispatch_on_the_cpu_and_outside_the_kernel_types():
    for N, m, dtype in [(91, 3, torch.float32), (20, tdea_ops.M_CAP + 1, torch.float32), (91, 3, torch.float64)]:
        w = torch.tensor(ref.directions(N, m)).to(dtype)
        n = 2 * w.shape[0]
        obj = torch.tensor(ref.objectives(n, m, "front", 1)).to(dtype)
        mask = torch.tensor(ref.masks(n)["every7"])
        assert torch.equal(tdea_ops.theta_rank(obj, w, mask), tdea_algo.theta_nd_sort(obj, w, mask))
    assert (tdea_ops.N_CAP, tdea_ops.M_CAP) == (rvea_ops.N_CAP, rvea_ops.M_CAP)
    with pytest.raises(ValueError):
        tdea_ops.theta_rank(torch.rand(10, 3), torch.rand(4, 3), torch.ones(10, dtype=torch.bool), return_parts=True)


def _frozen_theta_nd_sort(obj, w, mask):
    n, nw = obj.shape[0], w.shape[0]
    norm = torch.linalg.norm(obj, dim=1, keepdim=True)
    cosine = cos_dist(obj, w).clamp(-1, 1)
    d1 = norm * cosine
    d2 = norm * torch.sqrt(torch.clamp(1 - cosine**2, min=0))
    cls = torch.argmin(d2, 1)
    theta = torch.where((w > 1e-4).sum(1) == 1, torch.full((nw,), 1e6, device=w.device), torch.full((nw,), 5.0, device=w.device))
    val = d1.gather(1, cls[:, None])[:, 0] + theta[cls] * d2.gather(1, cls[:, None])[:, 0]
    big = nw + 1
    c = torch.where(mask, cls, torch.full_like(cls, big))
    o = torch.argsort(val, stable=True)
    o = o[torch.argsort(c[o], stable=True)]
    c_o = c[o]
    pos = torch.arange(n, device=obj.device) - torch.searchsorted(c_o, c_o)
    t_rank = torch.empty(n, dtype=torch.float32, device=obj.device)
    t_rank[o] = (pos + 1).to(torch.float32)
    return torch.where(mask, t_rank, torch.full_like(t_rank, float("inf")))


class _FrozenTDEA(A.TDEA):
    """θ-DEA with the ranking it called before ``ops.tdea`` existed, inlined."""

    def tell(self, state, fitness):
        N, m = self.pop_size, self.n_objs
        pop = torch.cat([state.population, state.next_generation], 0)
        obj = torch.cat([state.fitness, fitness], 0)
        rank = non_dominated_sort(obj, until=N + 1)
        worst = torch.sort(rank).values[N]
        mask = rank <= worst
        z = torch.minimum(state.z, obj.min(0).values)
        w1 = torch.where(torch.eye(m, dtype=torch.bool, device=obj.device), 1.0, 1e-6)
        asf = (torch.abs((obj[None] - z) / (state.z_nad - z)) / w1[:, None, :]).amax(-1)  # (m, n)
        ext = torch.argmin(asf, 1)
        sol, info = torch.linalg.solve_ex(obj[ext] - z, torch.ones((m, 1), device=obj.device))
        a = z + 1 / sol[:, 0]
        bad = (info != 0) | torch.isnan(a).any() | (a <= z).any()
        z_nad = torch.where(bad, obj.max(0).values, a)
        norm = (obj - z) / (z_nad - z)
        t_rank = _frozen_theta_nd_sort(norm, state.w, mask)
        idx = lexsort([t_rank, rank.to(t_rank.dtype)])[:N]
        return state.update(population=pop[idx], fitness=obj[idx], z=z, z_nad=z_nad)


def _run(cls, gens=5, seed=11):
    lb, ub = torch.zeros(12), torch.ones(12)
    wf = StdWorkflow(cls(lb, ub, 3, 100), DTLZ2(d=12, m=3), graph=False)
    st = wf.init(rnd.PRNGKey(seed))
    for _ in range(gens):
        st = wf.step(st)
    return st.get_child_state("algorithm")


def test_the_cpu_trajectory_has_not_moved():
    a, b = _run(A.TDEA), _run(_FrozenTDEA)
    assert torch.isfinite(a.fitness).all()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
