"""``nsga3_select.hip`` against the fixed-shape CPU op, and NSGA-III generations captured into
a hipGraph (MI355X, marked gpu).

The kernel's contract is exact: the same rows as ``nsga3_survivors`` on the CPU
(``torch.equal``), at sizes on both sides of every items-per-thread step and at the cap,
and on inputs that exercise each branch of the selection (K = 0, a single front, one niche,
empty niches everywhere, tied distances, NaN / inf distances, the two extreme niches).
"""
import pytest
import torch

import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.ops import _ext
from evoxmi.ops import nds
from evoxmi.ops.nds import nsga3_survivors
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu


def _random_case(n, N, R, seed):
    gen = torch.Generator().manual_seed(seed)
    # ~6 fronts over the merged rows: the cut falls inside one of them
    rank = torch.randint(0, 6, (n,), generator=gen, dtype=torch.int32)
    group = torch.randint(0, R, (n,), generator=gen)
    gd = torch.rand(n, generator=gen)
    return rank, group, gd


def _check(rank, group, gd, N, R, seed=0, expect_k=None):
    last_rank = torch.sort(rank).values[N]
    if expect_k is not None:
        assert N - int((rank < last_rank).sum()) == expect_k
    key = rnd.PRNGKey(seed)
    want = nsga3_survivors(rank, last_rank, group, gd, key, N, R)
    got = nsga3_survivors(rank.cuda(), last_rank.cuda(), group.cuda(), gd.cuda(), key.cuda(), N, R)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (N,)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("n,N,R", [(64, 32, 28), (130, 65, 66), (200, 100, 91), (2050, 1025, 1035), (8192, 4096, 4095)])
def test_kernel_matches_cpu_op(n, N, R):
    rank, group, gd = _random_case(n, N, R, seed=n)
    _check(rank, group, gd, N, R, seed=n)


STRUCTURED = ["k0", "one_front", "one_niche", "rho0", "equal_dist", "nan", "inf", "extreme_niches"]


@pytest.mark.parametrize("n,N,R", [(200, 100, 91), (8192, 4096, 4095)])
@pytest.mark.parametrize("kind", STRUCTURED)
def test_kernel_structured_inputs(kind, n, N, R):
    rank, group, gd = _random_case(n, N, R, seed=7)
    expect_k = None
    if kind == "k0":
        # exactly N rows ahead of the last front: nothing to fill
        rank = torch.cat([torch.zeros(N, dtype=torch.int32), torch.ones(n - N, dtype=torch.int32)])[torch.randperm(n, generator=torch.Generator().manual_seed(1))]
        expect_k = 0
    elif kind == "one_front":
        rank = torch.zeros(n, dtype=torch.int32)  # last_rank 0: every row is a candidate, K = N
        expect_k = N
    elif kind == "one_niche":
        group = torch.full((n,), R // 2, dtype=torch.int64)
    elif kind == "rho0":
        # front rows (ranks below the cut) all sit in niche 0; candidates use niches 1.. only
        last_rank = torch.sort(rank).values[N]
        group = torch.where(rank < last_rank, torch.zeros_like(group), 1 + group % (R - 1))
    elif kind == "equal_dist":
        gd = torch.full((n,), 0.25)
    elif kind in ("nan", "inf"):
        last_rank = torch.sort(rank).values[N]
        cand = torch.nonzero(rank == last_rank).flatten()
        group = torch.where(rank < last_rank, group % (R - 1), group)  # niche R − 1 has rho = 0
        group[cand[:3]] = R - 1
        gd[cand[1]] = float(kind)
    elif kind == "extreme_niches":
        group = (R - 1) * torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(2))
    _check(rank, group, gd, N, R, seed=3, expect_k=expect_k)


def test_over_cap_runs_the_torch_path(monkeypatch):
    n, N, R = 8194, 4097, 300
    rank, group, gd = _random_case(n, N, R, seed=5)
    last_rank = torch.sort(rank).values[N]
    key = rnd.PRNGKey(9)
    want = nsga3_survivors(rank, last_rank, group, gd, key, N, R)
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name != "nsga3_niche_select", "the kernel was called above its cap"
            return getattr(ops, name)

    monkeypatch.setattr(nds._ext, "ops", lambda: NoKernel())
    got = nsga3_survivors(rank.cuda(), last_rank.cuda(), group.cuda(), gd.cuda(), key.cuda(), N, R)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("c", [1, 63, 64, 65, 4095, 4096, 5000])
def test_uniform_stream_is_prefix_stable_on_device(c):
    key = rnd.PRNGKey(3, device="cuda")
    host = rnd.uniform(rnd.PRNGKey(3), (c,))
    # n ≥ 4096 draws through philox_fill, shorter ones through philox_words
    for n in (c, c + 1, 4095, 4096, 8192):
        if n >= c:
            u = rnd.uniform(key, (n,))[:c]
            assert torch.equal(u.cpu(), host)


def _run(pop, graph, gens, seed=11):
    d, m = 12, 3
    lb, ub = torch.zeros(d, device="cuda"), torch.ones(d, device="cuda")
    wf = StdWorkflow(A.NSGA3(lb, ub, m, pop), DTLZ2(d=d, m=m), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


@pytest.mark.parametrize("pop,gens", [(100, 5), (4097, 2)])
def test_generation_is_captured_and_matches_eager(pop, gens):
    """pop 100 runs the kernel; pop 4097 (n = 8194) the fixed-shape torch path above its cap."""
    _, a = _run(pop, False, gens)
    wf, b = _run(pop, True, gens)
    assert wf._graph is not None
    fa, fb = a.fitness, b.fitness
    fin = torch.isfinite(fa)
    assert torch.equal(fin, torch.isfinite(fb))
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)


def test_graph_runs_are_bitwise_reproducible():
    _, a = _run(100, True, 5)
    _, b = _run(100, True, 5)
    assert torch.equal(a.population, b.population)
    assert torch.equal(a.fitness, b.fitness)
