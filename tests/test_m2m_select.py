"""MOEA/D-M2M's association on the CPU: ``association_indices`` (the index computation factored out of ``associate``)
against the loop ``associate`` ran before, kept here verbatim as ``_legacy_associate``, and against the independent
numpy reference of ``_m2m_reference.py``; ``ops.m2m.select`` on CPU tensors returns the same rows with the region sizes
and cut ranks; and the seeded trajectory of the algorithm must not move by a bit.

Every case asserts on the reference that it qualifies: a region with fewer than S members, one with more, and one
whose cut front is larger than what is still needed from it, so that crowding decides."""
import numpy as np
import pytest
import torch

import _m2m_reference as ref
import evoxmi.algorithms as A
import evoxmi.algorithms.mo.moeadm2m as m2m_mod
from evoxmi import random as rnd
from evoxmi.algorithms.mo.moeadm2m import _rank_within, association_indices
from evoxmi.operators.selection.non_dominate import crowding_distance, lexsort
from evoxmi.ops import m2m as m2m_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.utils.common import cos_dist
from evoxmi.workflows import StdWorkflow


def _legacy_associate(key, pop, obj, w, s):
    """``associate`` as it was before the op existed (host reads, a loop over the regions)."""
    k = w.shape[0]
    n = pop.shape[0]
    region = torch.argmax(cos_dist(obj, w), 1)
    rank = _rank_within(obj, region).to(torch.float32)
    cols = []
    rad = rnd.randint(key, (s,), 0, n).to(pop.device)
    for i in range(k):
        mask = region == i
        cnt = int(mask.sum())
        if cnt < s:
            members = torch.nonzero(mask).flatten()
            cols.append(torch.cat([members, rad[cnt:]]))
        else:
            rk = torch.where(mask, rank, torch.full_like(rank, float("inf")))
            order = torch.argsort(rk, stable=True)
            worst = rk[order[s - 1]]
            cd = crowding_distance(obj, rk == worst)
            cols.append(lexsort([-cd, rk])[:s])
    part = torch.stack(cols, 1).T.reshape(-1)  # region-major (Fortran flatten of (s, k))
    return pop[part], obj[part]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


CASES = [(20, 3, 10, 1, "uniform"), (65, 2, 10, 3, "uniform"), (200, 3, 10, 10, "uniform"), (200, 3, 10, 10, "front"),
         (257, 5, 10, 12, "uniform"), (257, 16, 8, 16, "uniform"), (1000, 3, 10, 50, "uniform")]


@pytest.mark.parametrize("n,m,K,S,kind", CASES)
def test_reference_torch_path_and_op_agree(n, m, K, S, kind):
    obj, region, rad = ref.cached_case(n, m, K, S, kind)
    part, counts, worst, info = ref.select(obj, region, rad, K, S)
    below, above, crowded = ref.qualifies(info, S)
    assert below, "the input no longer qualifies: no region with fewer than S members"
    assert above, "the input no longer qualifies: no region with more than S members"
    assert crowded, "the input no longer qualifies: no cut front larger than what is needed from it"
    got = association_indices(_t(obj), _t(region), _t(rad), K, S)
    assert got.dtype == torch.int64 and got.shape == (K * S,)
    assert np.array_equal(got.numpy(), part)
    p, c, w = m2m_ops.select(_t(obj), _t(region), _t(rad), K, S, return_info=True)
    assert torch.equal(p, got) and torch.equal(m2m_ops.select(_t(obj), _t(region), _t(rad), K, S), got)
    assert c.dtype == torch.int32 and w.dtype == torch.int32
    assert np.array_equal(c.numpy(), counts) and np.array_equal(w.numpy(), worst)


@pytest.mark.parametrize("kind", ["uniform", "front"])
def test_the_algorithm_s_own_directions(kind):
    """n = 200, m = 3, K = 10, S = 10 with the regions MOEA/D-M2M itself assigns: ``associate`` gathers exactly what the
    loop before it gathered, and the rows are the reference's."""
    n, m, S = 200, 3, 10
    algo = A.MOEADM2M(torch.zeros(12), torch.ones(12), m, 100)
    K = algo.k
    assert K == 10 and algo.s == S
    obj = _t(ref.objectives(n, m, kind, 200))
    pop = torch.arange(n, dtype=torch.float32)[:, None].expand(n, 2).contiguous()  # a row's number as its genome
    key = rnd.PRNGKey(7)
    want_pop, want_obj = _legacy_associate(key, pop, obj, algo.w, S)
    got_pop, got_obj = m2m_mod.associate(key, pop, obj, algo.w, S)
    assert torch.equal(got_pop, want_pop) and torch.equal(got_obj, want_obj)
    region = torch.argmax(cos_dist(obj, algo.w), 1).numpy()
    rad = rnd.randint(key, (S,), 0, n).numpy()
    part, counts, worst, info = ref.select(obj.numpy(), region, rad, K, S)
    print(f"[m2m] {kind}: region sizes {counts.min()}..{counts.max()}, fronts peeled up to {max(i[1] for i in info)}")
    assert all(ref.qualifies(info, S)), "the input no longer qualifies"
    if kind == "front":
        assert worst.max() == 0  # every member at rank 0
    assert np.array_equal(got_pop[:, 0].numpy().astype(np.int64), part)


def test_equal_rows_and_exact_region_size():
    obj = np.full((40, 3), 0.25, dtype=np.float32)
    region, rad = np.zeros(40, dtype=np.int64), np.zeros(10, dtype=np.int64)
    part = ref.select(obj, region, rad, 1, 10)[0]
    assert part.tolist() == [0, 39] + list(range(1, 9))  # the extremes inf, the interior NaN, NaN last
    assert np.array_equal(association_indices(_t(obj), _t(region), _t(rad), 1, 10).numpy(), part)
    obj = ref.objectives(64, 3, "uniform", 9)
    region = np.where(np.arange(64) < 12, 0, 1).astype(np.int64)
    rad = np.arange(12, dtype=np.int64)
    part, counts, worst, _ = ref.select(obj, region, rad, 2, 12)
    assert counts[0] == 12 and worst[0] >= 0 and part[:12].tolist() != list(range(12))  # c == S: the selection branch
    p, c, w = m2m_ops.select(_t(obj), _t(region), _t(rad), 2, 12, return_info=True)
    assert np.array_equal(p.numpy(), part) and np.array_equal(c.numpy(), counts) and np.array_equal(w.numpy(), worst)


def _trajectory(gens=10):
    d, m, pop = 12, 3, 100
    wf = StdWorkflow(A.MOEADM2M(torch.zeros(d), torch.ones(d), m, pop), DTLZ2(d=d, m=m))
    st = wf.init(rnd.PRNGKey(21))
    for _ in range(gens + 1):  # the first step evaluates the initial population
        st = wf.step(st)
    return st.get_child_state("algorithm")


def test_trajectory_is_unchanged(monkeypatch):
    a = _trajectory()
    monkeypatch.setattr(m2m_mod, "associate", _legacy_associate)
    b = _trajectory()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
    assert torch.equal(a.key, b.key) and int(a.gen) == int(b.gen) == 10
