"""The float64 oracles of ``_moead_reference.py`` against the existing CPU paths (no GPU): on finite inputs they
must reproduce ``MOEAD._parents``, the float32 SBX + PM operators, ``moead_replace_sequential`` / the torch
``moead_replace`` and the CPU ``moead_scan``.  The NaN and +inf cases pin the torch ``moead_replace`` to the
sequential scan, whose ``f_old > f_new`` is false whenever either side is NaN."""
import types

import pytest
import torch

import _moead_reference as ref
from evoxmi.algorithms.mo.moead import MOEAD, moead_replace, moead_replace_sequential, reverse_neighbors
from evoxmi.operators.crossover import SimulatedBinary
from evoxmi.operators.mutation import Polynomial
from evoxmi.ops import mo as mo_ops
from evoxmi.ops import random as rnd
from evoxmi.utils.common import AggregationFunction

FUNCS = ["tchebycheff", "pbi", "weighted_sum", "modified_tchebycheff", "tchebycheff_norm"]


@pytest.mark.parametrize("N,T", [(1, 1), (5, 1), (5, 2), (40, 7), (9, 77)])
def test_parents_ref_equals_algorithm(N, T):
    nb = torch.randint(0, N, (N, T), generator=torch.Generator().manual_seed(N * 100 + T))
    key = rnd.PRNGKey(N + T)
    got = MOEAD._parents(None, types.SimpleNamespace(neighbors=nb), key)
    p0, p1 = ref.parents_ref(nb, key)
    assert torch.equal(p0, got[:, 0]) and torch.equal(p1, got[:, -1])
    if N >= 3:
        q0, q1 = ref.parents_ref(nb, key, 1, 2)
        keep = torch.tensor([1 <= i < 3 for i in range(N)])
        assert torch.equal(q0, p0 * keep) and torch.equal(q1, p1 * keep)


@pytest.mark.parametrize("N,d,pro_c,pro_m", [(101, 64, 1.0, 1.0), (101, 37, 0.6, 18.0), (7, 4, 0.5, 2.0), (1, 5, 1.0, 5.0), (64, 1, 0.9, 1.0)])
def test_variation_ref_matches_float32_operators(N, d, pro_c, pro_m):
    """Bounds ±2: the float32 operators stay within 2 ulp32(2) of the float64 restatement."""
    g = torch.Generator().manual_seed(N * 1000 + d)
    pop = torch.rand(N, d, generator=g) * 4 - 2
    lb, ub = torch.full((d,), -2.0), torch.full((d,), 2.0)
    p0, p1 = torch.randint(0, N, (N,), generator=g), torch.randint(0, N, (N,), generator=g)
    kx, km = rnd.PRNGKey(11), rnd.PRNGKey(12)
    off = SimulatedBinary(pro_c=pro_c, type=2)(kx, torch.cat([pop[p0], pop[p1]], 0))
    t32 = torch.clamp(Polynomial((lb, ub), pro_m=pro_m)(km, off), lb, ub)
    y, counts = ref.variation_ref(pop, p0, p1, kx, km, lb, ub, pro_c, 20.0, pro_m, 20.0)
    assert y.dtype == torch.float64 and y.shape == t32.shape
    err = float((t32.double() - y).abs().max())
    print(f"[variation_ref] N {N} d {d}: worst |float32 operators − ref| {err:.3e}, counts {counts}")
    assert err <= 2 * float(ref.ulp32(torch.tensor([2.0], dtype=torch.float64)))
    if N == 101:
        assert counts["pm_lo"] > 0 and counts["pm_hi"] > 0
        assert (counts["no_x"] > 0) == (pro_c < 1)


def _replace_case(N, T, M, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(N, M, generator=g) + 0.05
    nb = torch.argsort(torch.rand(N, N, generator=g), 1)[:, :T]
    pop_obj, off_obj = torch.rand(N, M, generator=g), torch.rand(N, M, generator=g)
    z, zmax = torch.zeros(M) - 0.01, torch.ones(M) * 1.1
    return w, nb, pop_obj, off_obj, z, zmax


def _three_ways(func, w, nb, pop_obj, off_obj, z, zmax):
    agg = AggregationFunction(func)
    N = pop_obj.shape[0]
    ids = torch.arange(N, dtype=torch.float32)[:, None]  # the decision rows carry the offspring's index
    seq_pop, seq_obj = moead_replace_sequential(-ids - 1, pop_obj, ids, off_obj, w, z, zmax, nb, agg)
    seq_win = torch.where(seq_pop[:, 0] >= 0, seq_pop[:, 0], torch.full((N,), -1.0)).long()
    rev = reverse_neighbors(nb)
    win, new_obj = moead_replace(pop_obj, off_obj, w, z, zmax, agg, rev)
    rwin, rnew, info = ref.replace_ref(pop_obj, off_obj, w, z, zmax, rev[0], rev[2], func)
    return (seq_win, seq_obj), (win, new_obj), (rwin, rnew), info


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("func", FUNCS)
def test_replace_ref_equals_sequential_and_torch(func):
    seq, par, r, info = _three_ways(func, *_replace_case(40, 6, 3, 5))
    assert info["margin"] >= 64 and info["ties_occupant"] == 0, info
    assert 0.2 <= info["replaced"] <= 0.95, info
    assert torch.equal(r[0], seq[0]) and torch.equal(r[1], seq[1])
    assert torch.equal(par[0], seq[0]) and torch.equal(par[1], seq[1])


@pytest.mark.parametrize("case", ["nan_offspring", "nan_occupant", "inf_offspring", "all"])
@pytest.mark.parametrize("func", FUNCS)
def test_replace_nan_and_inf_follow_the_sequential_scan(func, case):
    """One offspring row with one NaN objective, one occupant row with a NaN objective, one all-+inf offspring row
    (``nan_policy="inf"``).  The poisoned offspring is the one that wins the most slots on the clean input."""
    w, nb, pop_obj, off_obj, z, zmax = _replace_case(40, 6, 3, 5)
    clean = ref.replace_ref(pop_obj, off_obj, w, z, zmax, *reverse_neighbors(nb)[::2], func)[0]
    winners = torch.bincount(clean[clean >= 0], minlength=40)
    top = torch.argsort(winners, descending=True)
    assert winners[top[1]] >= 1
    if case in ("nan_offspring", "all"):
        off_obj[top[0], 1] = float("nan")
    if case in ("inf_offspring", "all"):
        off_obj[top[1]] = float("inf")
    if case in ("nan_occupant", "all"):
        pop_obj[int((clean >= 0).nonzero()[0]), 2] = float("nan")
    seq, par, r, info = _three_ways(func, w, nb, pop_obj, off_obj, z, zmax)
    assert info["margin"] >= 64, info
    assert torch.equal(r[0], seq[0]) and _same(r[1], seq[1])
    assert torch.equal(par[0], seq[0]) and _same(par[1], seq[1])
    if case in ("nan_offspring", "all"):
        assert not bool((seq[0] == top[0]).any())
    if case in ("nan_occupant", "all"):
        assert seq[0][int((clean >= 0).nonzero()[0])] == -1


@pytest.mark.parametrize("func", ["tchebycheff", "pbi", "weighted_sum", "modified_tchebycheff"])
@pytest.mark.parametrize("T,nr,update_z", [(1, 1, True), (30, 2, True), (30, 30, False), (64, 64, True)])
def test_scan_ref_equals_cpu_scan(func, T, nr, update_z):
    g = torch.Generator().manual_seed(7 + T)
    N, R, M = 80, 60, 3
    objs, off = torch.rand(N, M, generator=g), torch.rand(R, M, generator=g) * 0.9 - 0.05
    P = torch.stack([torch.randperm(N, generator=g)[:T] for _ in range(R)])
    W = torch.rand(N, M, generator=g) + 0.05
    z = objs.min(0).values - 0.01
    want = mo_ops.moead_scan(objs, off, P, W, z, func, nr=nr, update_z=update_z)
    owner, o, zz, info = ref.scan_ref(objs, off, P, W, z, func, nr=nr, update_z=update_z)
    assert info["margin"] >= 64 and info["ties"] == 0, info
    assert torch.equal(owner, want[0]) and torch.equal(o, want[1]) and torch.equal(zz, want[2])
    assert bool((zz != z).any()) == update_z
