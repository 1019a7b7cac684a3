"""NSGA-III niche-preserving selection as a fixed-shape op (``ops.nds.nsga3_survivors``), CPU.

The op replaces the data-dependent tail of ``NSGA3.tell`` (``bincount`` over a boolean mask,
``int(front.sum())``, two ``nonzero`` calls, a random draw whose length is the size of the
last front).  That tail is kept here verbatim as ``_legacy_tail``; the op must select exactly
the same rows, and the seeded trajectory of the algorithm must not move by a bit.
"""
import pytest
import torch

import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.ops.nds import nsga3_survivors
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow


def _lexsort_pair(primary, secondary):
    o = torch.argsort(secondary, stable=True)
    return o[torch.argsort(primary[o], stable=True)]


def _legacy_tail(rank, last_rank, group, group_dist, key, N, R):
    """The selection tail of ``NSGA3.tell`` before the op existed (host reads, dynamic shapes)."""
    dev = rank.device
    front = rank < last_rank
    last = rank == last_rank
    rho = torch.bincount(group[front], minlength=R)
    K = N - int(front.sum())
    cand = torch.nonzero(last).flatten()
    g = group[cand]
    u = rnd.uniform(key, (cand.shape[0],)).to(dev)
    # the closest member of an empty niche goes first
    gd = group_dist[cand]
    big = torch.full((R,), float("inf"), device=dev).scatter_reduce(0, g, gd, "amin")
    first = (rho[g] == 0) & (gd == big[g])
    key_in = torch.where(first, torch.full_like(u, -1.0), u)
    o = _lexsort_pair(g, key_in)  # candidates ordered by (niche, key)
    g_o = g[o]
    starts = torch.searchsorted(g_o, g_o, right=False)
    k = torch.arange(g_o.shape[0], device=dev) - starts
    level = rho[g_o] + k
    pick = _lexsort_pair(level, g_o.to(torch.float32))[:K]
    chosen = cand[o[pick]]
    keep = front.clone()
    keep[chosen] = True
    return torch.nonzero(keep).flatten()[:N]


def _case(seed, N, R, spread, one_niche=False, quarters=False):
    """A consistent random input: ``last_rank`` is the rank at sorted position N, as in ``tell``."""
    gen = torch.Generator().manual_seed(seed)
    n = 2 * N
    if spread >= n:
        rank = torch.randperm(n, generator=gen).to(torch.int32)
    else:
        rank = torch.randint(0, spread, (n,), generator=gen, dtype=torch.int32)
    last_rank = torch.sort(rank).values[N]
    group = torch.zeros(n, dtype=torch.int64) if one_niche else torch.randint(0, R, (n,), generator=gen)
    gd = torch.rand(n, generator=gen)
    if quarters:
        gd = torch.round(gd * 4) / 4
    return rank, last_rank, group, gd, rnd.PRNGKey(1000 + seed)


def test_fixed_shape_op_matches_the_legacy_tail():
    gen = torch.Generator().manual_seed(0)
    spreads = [1, 2, 4, 9, None]
    saw_k0 = saw_single_front = 0
    for c in range(300):
        N = int(torch.randint(2, 71, (1,), generator=gen))
        R = int(torch.randint(1, N + 3, (1,), generator=gen))
        spread = spreads[c % 5] or 2 * N
        rank, last_rank, group, gd, key = _case(c, N, R, spread, one_niche=c % 7 == 0, quarters=c % 3 == 0)
        K = N - int((rank < last_rank).sum())
        saw_k0 += K == 0
        saw_single_front += int(last_rank) == 0
        want = _legacy_tail(rank, last_rank, group, gd, key, N, R)
        got = nsga3_survivors(rank, last_rank, group, gd, key, N, R)
        assert got.dtype == torch.int64 and got.shape == (N,)
        assert torch.equal(got, want), (c, N, R, spread)
    assert saw_k0 >= 1 and saw_single_front >= 1


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nan_and_inf_distance_in_an_empty_niche(bad):
    """torch's amin propagates NaN: a niche with a NaN candidate has no 'closest first' member;
    an inf distance equals the inf the minimum starts from, so that candidate does go first."""
    N, R = 12, 5
    # ranks: 8 rows in front (niches 0-2), 16 candidates over niches 0-4: niches 3 and 4 have rho = 0
    rank = torch.tensor([0] * 8 + [1] * 16, dtype=torch.int32)
    last_rank = torch.sort(rank).values[N]
    group = torch.tensor([0, 0, 1, 1, 2, 2, 0, 1] + [3, 3, 3, 4, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 3])
    gd = torch.linspace(0.1, 0.9, 24)
    gd[9] = bad  # a candidate of niche 3 (rho = 0)
    assert int(last_rank) == 1 and not bool(((rank < last_rank) & (group == 3)).any())
    for seed in range(8):
        key = rnd.PRNGKey(seed)
        want = _legacy_tail(rank, last_rank, group, gd, key, N, R)
        assert torch.equal(nsga3_survivors(rank, last_rank, group, gd, key, N, R), want)


@pytest.mark.parametrize("c", [1, 63, 64, 65, 4095])
def test_uniform_stream_is_prefix_stable(c):
    """The op draws (n,) uniforms and reads the first c: the shorter draw must be its prefix."""
    key = rnd.PRNGKey(3)
    for n in (c, c + 1, 2 * c + 3, 8192):
        assert torch.equal(rnd.uniform(key, (c,)), rnd.uniform(key, (n,))[:c])


class _LegacyNSGA3(A.NSGA3):
    """NSGA-III whose ``tell`` ends in the legacy tail: the trajectory before the op."""

    def tell(self, state, fitness):
        import evoxmi.algorithms.mo.nsga3 as mod

        orig = mod.nsga3_survivors
        mod.nsga3_survivors = _legacy_tail
        try:
            return super().tell(state, fitness)
        finally:
            mod.nsga3_survivors = orig


def test_trajectory_is_unchanged():
    d, m, pop = 12, 3, 100
    lb, ub = torch.zeros(d), torch.ones(d)
    states = []
    for cls in (A.NSGA3, _LegacyNSGA3):
        wf = StdWorkflow(cls(lb, ub, m, pop), DTLZ2(d=d, m=m))
        st = wf.init(rnd.PRNGKey(11))
        for _ in range(5):
            st = wf.step(st)
        states.append(st.get_child_state("algorithm"))
    assert torch.equal(states[0].population, states[1].population)
    assert torch.equal(states[0].fitness, states[1].fitness)
