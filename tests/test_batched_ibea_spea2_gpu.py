"""The batched device forms behind ``BatchedRuns(IBEA | SPEA2)``: B independent runs in one launch of every kernel of
``ibea_select.hip`` and ``spea2_select.hip`` (MI355X, marked gpu).

* Every batched output against the single-run op run by run, bitwise (floats through ``.view(torch.int32)``, so NaNs
  count), and against a second call.  Runs of different structure share every launch: ``front`` (every row
  non-dominated: SPEA2 removes n − n_keep rows), ``uniform`` (at m = 3 few rows are non-dominated: SPEA2 removes nothing
  and ``select`` fills by ``sig``), ``equal`` (all rows equal), ``coarse`` (a coarse grid with duplicated rows) and
  ``nonfinite`` (a NaN row, an inf row, a −inf entry).  B = 1 is the non-finite run alone, B = 3 and B = 5 the first three
  and all five; IBEA's shapes from n = 1025 on run B = 2 (``nonfinite``, ``front``), so that every thread count meets a
  non-zero run offset.  The odd n make every per-run offset unaligned.
* The single-run kernels changed with them and are held to host references by ``tests/test_ibea_select_gpu.py`` and
  ``tests/test_spea2_select_gpu.py``.  In addition one batched launch per algorithm, B = 3 at (257, 3), is checked
  directly against those references on inputs they qualify as exact: SPEA2's S, nd, R against the int64 reference
  and its removal order against the float64 one (exactly two rows at the minimum and a relative gap of at least 1e-5
  at every step), IBEA's removal order against the float64 replay (a relative margin of at least 5e-5 at every
  step).  The qualification is asserted, so an input that stops qualifying fails.
* End to end: the runs of ``BatchedRuns`` on the device equal solo runs bit for bit, a captured batched generation
  equals the eager one, and per-run shapes above the kernels' caps raise under ``vmap`` while a solo call above them
  still takes the torch path.
"""
import functools

import numpy as np
import pytest
import torch

import _spea2_reference as ref
from test_batched_ibea_spea2 import KAPPA, check_runs_equal_solo, make, same_bits
from test_batched_mo import D, GENS, M, POP, RUNS
from test_ibea_select_gpu import _reference64

pytestmark = pytest.mark.gpu

KINDS = ["front", "uniform", "equal", "coarse", "nonfinite"]


@pytest.fixture
def ext():
    from evoxmi.ops import _ext

    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    yield _ext
    torch.cuda.synchronize()
    _ext.check_kernel_errors()


# ---------------------------------------------------------------- inputs
def _coarse(n, m, rng):
    f = np.round(rng.random((n, m), dtype=np.float32) * 4) / 4
    if n > 3:
        f[n // 2] = f[0]
        f[n - 1] = f[1]
    return f.astype(np.float32)


def _nonfinite(n, m, rng):
    f = rng.random((n, m), dtype=np.float32)
    f[0, 0] = np.nan
    f[n - 1] = np.inf
    if n > 4:
        f[n // 2, m - 1] = -np.inf
    return f


@functools.lru_cache(maxsize=None)
def runs_of(n, m):
    """The five runs of KINDS, (5, n, m) float32, read-only and shared by the tests."""
    rng = np.random.default_rng(100 * n + m)
    f = np.stack([ref.objectives(n, m, "front", 100 * n + m), ref.objectives(n, m, "uniform", 100 * n + m),
                  np.full((n, m), 0.5, dtype=np.float32), _coarse(n, m, rng), _nonfinite(n, m, rng)])
    f.setflags(write=False)
    return f


RUN_IDS = {1: [4], 2: [4, 0], 3: [0, 1, 2], 5: [0, 1, 2, 3, 4]}


def _batch(n, m, B):
    return torch.from_numpy(runs_of(n, m)[RUN_IDS[B]]).cuda()  # fancy indexing copies: the shared array stays read-only


def _all_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"{what}: output {k} differs (or its shape or dtype: {tuple(g.shape)} {g.dtype} / {tuple(w.shape)} {w.dtype})"


# ---------------------------------------------------------------- IBEA
IBEA_SHAPES = [(2, 2), (65, 2), (65, 3), (200, 3), (257, 5), (513, 3), (1025, 2), (2049, 5), (4097, 3)]


@functools.lru_cache(maxsize=None)
def _ibea_single(n, m):
    """(f, C, idx, order) of the single-run ops on each of the five runs."""
    from evoxmi.ops import ibea as ibea_ops

    out = []
    for o in torch.from_numpy(np.array(runs_of(n, m))).cuda():
        out.append(tuple(ibea_ops.fitness(o, KAPPA)) + tuple(ibea_ops.select(o, KAPPA, n // 2, return_order=True)))
    return out


@pytest.mark.parametrize("n,m", IBEA_SHAPES)
def test_ibea_batched_equals_single_run_op(ext, n, m):
    from evoxmi.ops import ibea as ibea_ops

    single = _ibea_single(n, m)
    n_keep = n // 2
    for B in ((1, 3, 5) if n < 1025 else (2,)):
        obj = _batch(n, m, B)
        f, C = ibea_ops.fitness(obj, KAPPA)
        idx, order = ibea_ops.select(obj, KAPPA, n_keep, return_order=True)
        assert f.shape == (B, n) and C.shape == (B, n) and f.dtype == torch.float32
        assert idx.shape == (B, n_keep) and order.shape == (B, n - n_keep) and idx.dtype == torch.int64 and order.dtype == torch.int64
        for b, r in enumerate(RUN_IDS[B]):
            _all_same((f[b], C[b], idx[b], order[b]), single[r], f"({n}, {m}) B={B} run {KINDS[r]}")
        again = tuple(ibea_ops.fitness(obj, KAPPA)) + tuple(ibea_ops.select(obj, KAPPA, n_keep, return_order=True))
        _all_same(again, (f, C, idx, order), f"({n}, {m}) B={B}: a second call")
    if n > 2:  # the finite runs remove different rows: the runs are not copies of one another
        assert not torch.equal(single[0][3], single[1][3])


# ---------------------------------------------------------------- SPEA2
SPEA2_SHAPES = [(2, 2), (65, 3), (200, 3), (257, 4), (257, 5), (513, 16), (1025, 2), (2049, 3), (4097, 5)]


@functools.lru_cache(maxsize=None)
def _spea2_single(n, m):
    """Per run: the eight outputs of spea2_fitness, (keep, order, stats) of spea2_truncate on the fitness mask with the
    fitness pass's neighbours, the same with the neighbour-only pass on an all-true mask, and select's idx."""
    from evoxmi.ops import _ext
    from evoxmi.ops import spea2 as spea2_ops

    ops, out = _ext.ops(), []
    for o in torch.from_numpy(np.array(runs_of(n, m))).cuda():
        fit = ops.spea2_fitness(o)
        tr = ops.spea2_truncate(o, fit[5], n // 2, fit[6], fit[7])
        tr_all = ops.spea2_truncate(o, torch.ones(n, dtype=torch.bool, device="cuda"), n // 2, None, None)
        out.append((tuple(fit), tuple(tr), tuple(tr_all), spea2_ops.select(o, n // 2)))
    return out


@pytest.mark.parametrize("n,m", SPEA2_SHAPES)
def test_spea2_batched_equals_single_run_op(ext, n, m):
    from evoxmi.ops import spea2 as spea2_ops

    ops = ext.ops()
    single = _spea2_single(n, m)
    n_keep = n // 2
    for B in (1, 3, 5):
        obj = _batch(n, m, B)
        what = f"({n}, {m}) B={B}"
        fit = ops.spea2_fitness(obj)
        assert len(fit) == 8 and all(t.shape == (B, n) for t in fit)
        tr = ops.spea2_truncate(obj, fit[5], n_keep, fit[6], fit[7])
        assert tr[0].shape == (B, n) and tr[1].shape == (B, n - n_keep) and tr[2].shape == (B, 2)
        ones = torch.ones(B, n, dtype=torch.bool, device="cuda")
        tr_all = ops.spea2_truncate(obj, ones, n_keep, None, None)  # the neighbour-only pass
        idx = spea2_ops.select(obj, n_keep)
        assert idx.shape == (B, n_keep) and idx.dtype == torch.int64
        for b, r in enumerate(RUN_IDS[B]):
            s_fit, s_tr, s_all, s_idx = single[r]
            _all_same([t[b] for t in fit], s_fit, f"{what} run {KINDS[r]}: fitness")
            _all_same([t[b] for t in tr], s_tr, f"{what} run {KINDS[r]}: truncate")
            _all_same([t[b] for t in tr_all], s_all, f"{what} run {KINDS[r]}: truncate, all-true mask")
            assert same_bits(idx[b], s_idx), f"{what} run {KINDS[r]}: select"
        # the public entries are the same launches
        _all_same(spea2_ops.fitness(obj, return_parts=True), fit[:5], f"{what}: ops.spea2.fitness")
        keep, order, rescans = spea2_ops.truncate(obj, ones, n_keep, return_order=True)
        _all_same((keep, order, rescans), (tr_all[0], tr_all[1], tr_all[2][:, 0]), f"{what}: ops.spea2.truncate")
        # a second call
        _all_same(ops.spea2_fitness(obj), fit, f"{what}: fitness, a second call")
        _all_same(ops.spea2_truncate(obj, fit[5], n_keep, fit[6], fit[7]), tr, f"{what}: truncate, a second call")
        if B >= 3:  # front, uniform, equal side by side: each run counts its own removals
            removed = tr[2][:, 1].tolist()
            assert removed[0] == n - n_keep, f"{what}: front removes n - n_keep rows, got {removed}"
            assert tr_all[2][:, 1].tolist() == [n - n_keep] * B
            if m == 3:
                assert removed[1] == 0, f"{what}: uniform removes nothing, got {removed}"
                assert bool((tr[1][1] == -1).all()) and same_bits(tr[0][1], fit[5][1])  # nothing left the mask
                assert torch.equal(idx[1], torch.argsort(fit[0][1], stable=True)[:n_keep])  # select fills by sig


# ---------------------------------------------------------------- against references that are not the code under test
def test_spea2_batched_launch_against_the_host_references(ext):
    n, m, n_keep = 257, 3, 128
    runs = [("front", 2), ("uniform", 0), ("front", 3)]
    objs = [ref.objectives(n, m, kind, seed) for kind, seed in runs]
    obj = torch.from_numpy(np.stack(objs)).cuda()
    ops = ext.ops()
    sig, S, R, D, nd = ops.spea2_fitness(obj)[:5]
    order = ops.spea2_truncate(obj, torch.ones(3, n, dtype=torch.bool, device="cuda"), n_keep, None, None)[1]
    mask = np.ones(n, dtype=bool)
    for b, (kind, seed) in enumerate(runs):
        S64, nd64, R64, _ = ref.fitness_parts(objs[b])
        assert np.array_equal(S[b].cpu().numpy(), S64), f"run {b}: S"
        assert np.array_equal(nd[b].cpu().numpy(), nd64), f"run {b}: nd"
        assert np.array_equal(R[b].cpu().numpy(), R64.astype(np.float32)), f"run {b}: R"
        if kind == "front":
            assert nd64.all()
        want, gap, pairs, _ = ref.incremental_truncation(objs[b], mask, n - n_keep)
        print(f"[exact] run {b} ({kind}, seed {seed}): gap {gap:.3e}")
        assert pairs and gap >= 1e-5, f"run {b}: the input no longer qualifies: pairs {pairs}, gap {gap:.3e}"
        assert np.array_equal(order[b].cpu().numpy(), want), f"run {b}: removal order"


def test_ibea_batched_launch_against_the_float64_order(ext):
    from evoxmi.ops import ibea as ibea_ops

    n, m, n_keep = 257, 3, 128
    objs = []
    for seed in (28, 55, 58):
        o = torch.rand(n, m, generator=torch.Generator().manual_seed(seed))
        objs.append(o / o.sum(1, keepdim=True))  # rows on the simplex, as near a front
    idx, order = ibea_ops.select(torch.stack(objs).cuda(), KAPPA, n_keep, return_order=True)
    for b, o in enumerate(objs):
        want, gap = _reference64(o, n - n_keep)
        print(f"[exact] run {b}: strict gap {gap:.3e}")
        assert gap >= 5e-5, f"run {b}: the input no longer qualifies: strict gap {gap:.3e}"
        assert torch.equal(order[b].cpu(), want), f"run {b}: removal order"
        keep = torch.ones(n, dtype=torch.bool)
        keep[want] = False
        assert torch.equal(idx[b].cpu(), torch.nonzero(keep).flatten())


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["IBEA", "SPEA2"])
def test_batched_runs_equal_solo_gpu(ext, name):
    check_runs_equal_solo(name, "cuda")


@pytest.mark.parametrize("name", ["IBEA", "SPEA2"])
def test_batched_captured_equals_eager(ext, name):
    from evoxmi import random as rnd
    from evoxmi.algorithms.containers.batched import BatchedRuns
    from evoxmi.problems.numerical import DTLZ2
    from evoxmi.workflows import StdWorkflow

    def final(graph):
        wf = StdWorkflow(BatchedRuns(make(name, "cuda"), RUNS), DTLZ2(d=D, m=M), graph=graph)
        st = wf.init(rnd.PRNGKey(9, device="cuda"))
        for _ in range(GENS + 1):  # the initial evaluation, then GENS generations
            st = wf.step(st)
        runs = st.get_child_state("algorithm").runs
        return runs.population.clone(), runs.fitness.clone()

    (p0, f0), (p1, f1) = final(False), final(True)
    assert p0.shape == (RUNS, POP, D)
    assert torch.equal(p0, p1) and torch.equal(f0, f1)


def test_vmapped_calls_are_the_batched_launches(ext):
    from torch.func import vmap

    from evoxmi.ops import batching
    from evoxmi.ops import ibea as ibea_ops
    from evoxmi.ops import spea2 as spea2_ops

    batching.register()
    obj = _batch(200, 3, 5)
    _all_same(vmap(lambda o: ibea_ops.fitness(o, KAPPA))(obj), ibea_ops.fitness(obj, KAPPA), "ibea.fitness")
    _all_same(vmap(lambda o: ibea_ops.select(o, KAPPA, 100, return_order=True))(obj), ibea_ops.select(obj, KAPPA, 100, return_order=True),
              "ibea.select")
    _all_same(vmap(lambda o: spea2_ops.fitness(o, return_parts=True))(obj), spea2_ops.fitness(obj, return_parts=True), "spea2.fitness")
    ones = torch.ones(200, dtype=torch.bool, device="cuda")  # shared by the runs: the rule broadcasts it
    _all_same(vmap(lambda o: spea2_ops.truncate(o, ones, 100, return_order=True))(obj),
              spea2_ops.truncate(obj, ones.expand(5, 200), 100, return_order=True), "spea2.truncate")
    assert same_bits(vmap(lambda o: spea2_ops.select(o, 100))(obj), spea2_ops.select(obj, 100))


# ---------------------------------------------------------------- caps
def test_above_cap_shapes_raise_under_vmap(ext, monkeypatch):
    from torch.func import vmap

    from evoxmi.ops import batching
    from evoxmi.ops import ibea as ibea_ops
    from evoxmi.ops import spea2 as spea2_ops

    batching.register()
    tall = torch.rand(2, 8193, 2, device="cuda")  # n = 8193 > 8192
    wide = torch.rand(2, 16, 17, device="cuda")  # m = 17 > 16
    rows = lambda t, dt: torch.zeros(t.shape[:2], dtype=dt, device="cuda")
    for f, match in ((tall, "got n = 8193"), (wide, "m = 17")):
        with pytest.raises(NotImplementedError, match=match):
            vmap(lambda x: ibea_ops.select(x, KAPPA, 8))(f)
        with pytest.raises(NotImplementedError, match=match):
            vmap(lambda x: spea2_ops.select(x, 8))(f)
        with pytest.raises(NotImplementedError, match=match):
            vmap(lambda x: spea2_ops.truncate(x, torch.ones(x.shape[0], dtype=torch.bool, device="cuda"), 8))(f)
        with pytest.raises(NotImplementedError, match=match):
            ibea_ops.select(f, KAPPA, 8)
        with pytest.raises(NotImplementedError, match=match):
            spea2_ops.select(f, 8)
        # the ops' own rules (a call that reaches them is never run sample by sample)
        with pytest.raises(NotImplementedError, match=f"ibea_truncate vmap rule.*{match}"):
            vmap(lambda x, a, c: torch.ops.evoxmi.ibea_truncate(x, a, c, KAPPA, 8, 8))(f, rows(f, torch.float32), rows(f, torch.float32))
        with pytest.raises(NotImplementedError, match=f"spea2_truncate vmap rule.*{match}"):
            vmap(lambda x, k: torch.ops.evoxmi.spea2_truncate(x, k, 8, None, None))(f, rows(f, torch.bool))
    with pytest.raises(NotImplementedError, match="ibea_fitness vmap rule.*m = 17"):
        vmap(lambda x: torch.ops.evoxmi.ibea_fitness(x, KAPPA))(wide)
    with pytest.raises(NotImplementedError, match="spea2_fitness vmap rule.*m = 17"):
        vmap(lambda x: torch.ops.evoxmi.spea2_fitness(x))(wide)
    with pytest.raises(NotImplementedError, match="m = 17"):
        vmap(lambda x: ibea_ops.fitness(x, KAPPA))(wide)
    with pytest.raises(NotImplementedError, match="m = 17"):
        vmap(lambda x: spea2_ops.fitness(x))(wide)

    # a solo call above the cap still takes the torch path, without raising
    ops = ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in ("ibea_truncate", "spea2_truncate"), "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(ibea_ops._ext, "ops", lambda: NoKernel())
    solo = tall[0]
    idx = ibea_ops.select(solo, KAPPA, 8190)
    assert idx.is_cuda and idx.shape == (8190,)
    idx = spea2_ops.select(solo, 8190)
    assert idx.is_cuda and idx.shape == (8190,)
