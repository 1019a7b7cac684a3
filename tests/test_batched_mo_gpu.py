"""The batched device forms behind ``BatchedRuns(NSGA2 | GDE3)``: B independent runs in one launch.

* ``nds`` on f (B, n, m) (``nds_batched.hip``, one workgroup per run) against the single-run op run by
  run, exact, for every ``until``, and for ``until = 0`` against ``host_rank_from_domination_matrix``
  on the CPU dominance matrix.  Runs of different structure share a launch (a chain of n fronts next
  to one front next to random rows), which shows that the stop is per run and that no state is shared.
  n covers 1, 2, the wave size ± 1, both sides of the 256/1024-thread switch at 512 and more than one
  owned row per thread (1025).
* ``nsga2_survivors`` on (B, n, m) against the single-run op run by run, exact, and for finite objectives
  against the CPU torch path.  Runs with ±inf / NaN compare only against the single-run kernel
  (``nsga_select.hip``'s header says why the torch path differs there).
* ``sbx`` / ``pm`` on x (B, n, d) with keys (B, 2) against the single-run ops per key, bitwise.
* End to end: the runs of ``BatchedRuns`` on the device equal solo runs bit for bit, a captured batched
  generation equals the eager one, and shapes above the kernels' caps raise under ``vmap``.
"""
import functools

import numpy as np
import pytest
import torch

from test_batched_mo import D, GENS, M, POP, RUNS, check_runs_equal_solo, make

pytestmark = pytest.mark.gpu


@pytest.fixture
def ext():
    from evoxmi.ops import _ext

    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    yield _ext
    torch.cuda.synchronize()
    _ext.check_kernel_errors()


# ---------------------------------------------------------------- inputs
def _random(n, m, rng):
    return rng.random((n, m), dtype=np.float32)


def _duplicated(n, m, rng):
    f = np.round(rng.random((n, m), dtype=np.float32) * 4) / 4  # a coarse grid: many equal rows and ties
    if n > 3:
        f[n // 2] = f[0]
        f[n - 1] = f[1]
    return f.astype(np.float32)


def _chain(n, m, rng):
    return np.repeat(rng.permutation(n)[:, None], m, 1).astype(np.float32)  # n fronts


def _one_front(n, m, rng):
    if m == 1:
        return np.full((n, 1), 0.5, dtype=np.float32)
    f = np.zeros((n, m), dtype=np.float32)
    p = rng.permutation(n)
    f[:, 0], f[:, 1] = p, -p.astype(np.float32)
    return f


def _nonfinite(n, m, rng):
    f = rng.random((n, m), dtype=np.float32)
    f[0, 0] = np.nan  # a NaN row: dominates nothing, dominated by nothing
    if n > 1:
        f[n - 1] = np.inf  # an inf row
    if n > 4:
        f[n // 2, m - 1] = -np.inf
        f[n // 3] = -np.inf
    return f


@functools.lru_cache(maxsize=None)
def runs_of(n, m):
    """Five runs of different structure, (5, n, m), read-only and shared by the tests."""
    rng = np.random.default_rng(100 * n + m)
    kinds = [_chain if n <= 130 else _duplicated, _one_front, _random, _duplicated, _nonfinite]
    f = np.stack([k(n, m, rng) for k in kinds])
    f.setflags(write=False)
    return f


def _batch(n, m, B):
    f = runs_of(n, m)
    return f[{1: [4], 3: [0, 1, 2], 5: [0, 1, 2, 3, 4]}[B]]  # B = 1: the run with NaN and inf


def _host_rank(f):
    from evoxmi.operators.selection.non_dominate import host_rank_from_domination_matrix
    from evoxmi.utils.common import dominate_relation

    t = torch.from_numpy(np.array(f))
    dom = dominate_relation(t, t)
    return host_rank_from_domination_matrix(dom.numpy(), dom.sum(0).to(torch.int32).numpy())


def _untils(n):
    return sorted({0, 1, n // 2, n // 2 + 1, n})


# ---------------------------------------------------------------- ranks
@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 512, 513, 1025])
def test_batched_ranks_equal_single_run_op(ext, n, m):
    dev = torch.device("cuda")
    all_runs = torch.from_numpy(np.array(runs_of(n, m))).to(dev)
    err = ext.error_flag(dev)
    single = {(r, u): ext.ops().nds(all_runs[r].contiguous(), u, err) for r in range(5) for u in _untils(n)}
    host = [_host_rank(runs_of(n, m)[r]) for r in range(5)]
    for r in range(5):
        assert np.array_equal(single[(r, 0)].cpu().numpy(), host[r]), f"single-run op, run {r}"
    if n <= 130:
        assert int(single[(0, 0)].max()) == n - 1  # the chain has n fronts
    assert int(single[(1, 0)].max()) == 0  # one front
    for B in (1, 3, 5):
        ids = {1: [4], 3: [0, 1, 2], 5: [0, 1, 2, 3, 4]}[B]
        f = torch.from_numpy(np.array(_batch(n, m, B))).to(dev)
        for u in _untils(n):
            out = ext.ops().nds(f, u, None)
            assert out.shape == (B, n) and out.dtype == torch.int32
            for b, r in enumerate(ids):
                assert torch.equal(out[b], single[(r, u)]), f"B={B} until={u} run {r}"
            if u == 0:
                for b, r in enumerate(ids):
                    assert np.array_equal(out[b].cpu().numpy(), host[r]), f"B={B} run {r} against the host peel"
            assert torch.equal(ext.ops().nds(f, u, None), out), "a second call differs"


def test_batched_ranks_public_entry_points(ext):
    from evoxmi.operators.selection import non_dominated_sort
    from evoxmi.ops import nds

    f = torch.from_numpy(np.array(runs_of(130, 3))).cuda()
    ref = torch.stack([non_dominated_sort(f[b], until=66) for b in range(5)])
    assert torch.equal(non_dominated_sort(f, until=66), ref)
    assert torch.equal(nds.non_dominated_sort(f, 66), ref)
    assert torch.equal(non_dominated_sort(f).cpu(), non_dominated_sort(f.cpu()))


# ---------------------------------------------------------------- survivors
@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("n", [2, 40, 130, 1025])
def test_batched_survivors_equal_single_run_op(ext, n, m):
    from evoxmi.ops import nds

    f_host = runs_of(n, m)
    f = torch.from_numpy(np.array(f_host)).cuda()
    N = n // 2
    for mask_pos, until in ((N, N + 1), (N - 1, N)):  # NSGA-II's tell; common.nsga2_select
        out = nds.nsga2_survivors(f, N, mask_pos, until=until)
        assert out.shape == (5, N) and out.dtype == torch.int64
        for b in range(5):
            assert torch.equal(out[b], nds.nsga2_survivors(f[b], N, mask_pos, until=until)), f"run {b} mask_pos={mask_pos}"
            assert out[b].unique().numel() == N and int(out[b].min()) >= 0 and int(out[b].max()) < n
        for b in range(4):  # the finite runs: also the CPU torch path
            ref = nds.nsga2_survivors_torch(torch.from_numpy(np.array(f_host[b])), N, mask_pos, until=until)
            assert torch.equal(out[b].cpu(), ref), f"run {b} mask_pos={mask_pos} against the torch path"
        assert torch.equal(nds.nsga2_survivors(f, N, mask_pos, until=until), out), "a second call differs"


def test_batched_nsga_select_takes_any_labels(ext):
    """The selection kernel alone, on labels that are no Pareto ranks (unranked rows carry n)."""
    rng = np.random.default_rng(5)
    B, n, m, N = 3, 257, 3, 100
    f = torch.from_numpy(rng.random((B, n, m), dtype=np.float32)).cuda()
    label = torch.from_numpy(rng.integers(0, 4, (B, n)).astype(np.int32)).cuda()
    label[1, label[1] == 3] = n
    for mask_pos in (N - 1, N):
        out = ext.ops().nsga_select(label, f, N, mask_pos)
        for b in range(B):
            assert torch.equal(out[b], ext.ops().nsga_select(label[b].contiguous(), f[b].contiguous(), N, mask_pos))


# ---------------------------------------------------------------- variation
VARIATION_SHAPES = [(d, 0, 0) for d in (1, 3, 4, 12)] + [(4, 4, 12)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [5, 6])
@pytest.mark.parametrize("d,col0,dtot", VARIATION_SHAPES)
def test_batched_sbx_pm_equal_single_run_ops(ext, d, col0, dtot, n, B):
    from evoxmi import random as rnd
    from evoxmi.ops import evo

    dev = torch.device("cuda")
    keys = rnd.split(rnd.PRNGKey(31 * d + n, device=dev), B)
    x = rnd.uniform(rnd.PRNGKey(3, device=dev), (B, n, d)).to(dev) * 2 - 0.5  # some genes outside [0, 1]: pm clips them
    lb, ub = torch.zeros(d, device=dev), torch.linspace(1, 2, d, device=dev)
    cols = (col0, dtot) if dtot else None
    for typ in (1, 2):
        out = evo.sbx(keys, x, 0.9, 20.0, typ, cols)
        assert out.shape == (B, n if typ == 1 else n // 2, d)
        for b in range(B):
            assert torch.equal(out[b], evo.sbx(keys[b], x[b], 0.9, 20.0, typ, cols)), f"sbx type {typ} run {b}"
    if n % 2:
        assert torch.equal(evo.sbx(keys, x, 0.9, 20.0, 1, cols)[:, -1], x[:, -1])  # the odd last parent passes through
    out = evo.polynomial(keys, x, lb, ub, 1.0 * max(dtot, d), 20.0, cols)  # every gene a mutation site
    assert out.shape == x.shape
    for b in range(B):
        assert torch.equal(out[b], evo.polynomial(keys[b], x[b], lb, ub, 1.0 * max(dtot, d), 20.0, cols)), f"pm run {b}"
    if n % 2:
        assert torch.equal(out[:, -1], x[:, -1])  # rows past nm pass through
    if B > 1:
        assert not torch.equal(out[0], out[1])


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["GDE3", "NSGA2"])
def test_batched_mo_runs_equal_solo_gpu(ext, name):
    check_runs_equal_solo(name, "cuda")


def test_batched_nsga2_captured_equals_eager(ext):
    from evoxmi import random as rnd
    from evoxmi.algorithms.containers.batched import BatchedRuns
    from evoxmi.problems.numerical import DTLZ2
    from evoxmi.workflows import StdWorkflow

    def final(graph):
        wf = StdWorkflow(BatchedRuns(make("NSGA2", "cuda"), RUNS), DTLZ2(d=D, m=M), graph=graph)
        st = wf.init(rnd.PRNGKey(9, device="cuda"))
        for _ in range(GENS + 1):  # the initial evaluation, then GENS generations
            st = wf.step(st)
        runs = st.get_child_state("algorithm").runs
        return runs.population.clone(), runs.fitness.clone()

    (p0, f0), (p1, f1) = final(False), final(True)
    assert p0.shape == (RUNS, POP, D)
    assert torch.equal(p0, p1) and torch.equal(f0, f1)


def test_above_cap_shapes_raise_under_vmap(ext):
    from torch.func import vmap

    from evoxmi.algorithms.mo.common import nsga2_select
    from evoxmi.operators.selection import non_dominated_sort
    from evoxmi.ops import batching, nds

    batching.register()
    wide = torch.rand(2, 16, 9, device="cuda")  # m = 9 > 8
    tall = torch.zeros(2, 8193, 2, device="cuda")  # n = 8193 > 8192
    for f in (wide, tall):
        with pytest.raises(NotImplementedError, match="8192"):
            vmap(lambda x: non_dominated_sort(x))(f)
        with pytest.raises(NotImplementedError, match="8192"):
            vmap(lambda x: nsga2_select(x, 8))(f)
        with pytest.raises(NotImplementedError, match="8192"):
            nds.non_dominated_sort(f)
    # the ops' own rules (a call that reaches them is never run sample by sample)
    with pytest.raises(NotImplementedError, match="nds vmap rule.*8192"):
        vmap(lambda x: torch.ops.evoxmi.nds(x, 0, None))(tall)
    with pytest.raises(NotImplementedError, match="nsga_select vmap rule.*8192"):
        vmap(lambda x: torch.ops.evoxmi.nsga_select(torch.zeros(8193, dtype=torch.int32, device="cuda"), x, 8, 8))(tall)
    with pytest.raises(NotImplementedError, match="shared"):
        vmap(lambda x, lo: torch.ops.evoxmi.pm(x, lo, lo + 1, torch.zeros(2, 2, dtype=torch.int64, device="cuda"), 1.0, 20.0, 4))(
            torch.rand(2, 4, 3, device="cuda"), torch.zeros(2, 3, device="cuda"))
