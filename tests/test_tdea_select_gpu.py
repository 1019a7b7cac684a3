"""``tdea_select.hip`` (on ``rvea_select.hip``'s best cosine) against the host reference of its contract, and θ-DEA
generations captured into a hipGraph (MI355X, marked gpu).  The reference is numpy float64 on the same float32 inputs
(``_tdea_reference.py``; ``test_tdea_select.py`` pins it to the torch path).

Inputs: ``uniform`` is rand in [0, 1]^m + 0.01, ``front`` is |normal| + 1e-3 normalised to the unit sphere and scaled by
1 + 0.2·rand, so no row is zero; ``w`` is what ``UniformSampling(N, m)`` yields (one direction (1/m, …) for nw = 1) and
n = 2·nw, in one case 3·nw + 1.  Masks: all rows, every 7th row out, one row only, none.  The n = 2070 and n = 8190 rows of
the two largest cases span more than one LDS tile of the counting launch (2048 rows).

Asserted per case: ``cls`` and ``t_rank`` equal the reference exactly and ``val`` bit for bit; within every cluster the
masked ranks are 1 … c; the rows outside the mask are +inf; a second call is bitwise equal.

Observed on an MI355X (gfx950): equal in all 18 cases under the four masks (largest cluster 17 rows, at n = 901 on 300
directions); IGD after 100 captured generations 0.0545 (the CPU run measures .054)."""
import numpy as np
import pytest
import torch

import _tdea_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import tdea as tdea_algo
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import tdea as tdea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu

KERNELS = ("tdea_theta_rank", "rvea_cos_best")


def _dev(a):
    return torch.tensor(np.array(a)).cuda()


def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(tdea_ops._ext, "ops", lambda: NoKernel())


# ---------------------------------------------------------------- 1. the ranking
# (N, m, factor, extra): n = factor·nw + extra
CASES = [(1, 2, 2, 0), (3, 3, 2, 0), (91, 3, 2, 0), (300, 3, 2, 0), (210, 5, 2, 0), (1035, 3, 2, 0), (4095, 3, 2, 0), (300, 3, 3, 1),
         (220, 10, 2, 0)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("N,m,factor,extra", CASES)
def test_theta_rank_against_the_reference(N, m, factor, extra, kind):
    obj, w, cls64, val64 = ref.cached_case(N, m, kind, factor, extra)
    n, nw = obj.shape[0], w.shape[0]
    assert n == factor * nw + extra and (N != 1 or nw == 1)
    d_obj, d_w = _dev(obj), _dev(w)
    for name, mask in ref.masks(n).items():
        want = ref.rank(cls64, val64, mask)
        d_mask = _dev(mask)
        t_rank, cls, val = tdea_ops.theta_rank(d_obj, d_w, d_mask, return_parts=True)
        assert t_rank.is_cuda and t_rank.dtype == torch.float32 and t_rank.shape == (n,)
        assert cls.dtype == torch.int64 and val.dtype == torch.float64 and cls.shape == (n,) and val.shape == (n,)
        t_h, cls_h, val_h = t_rank.cpu().numpy(), cls.cpu().numpy(), val.cpu().numpy()
        what = f"({nw}, {m}) n {n} {kind} {name}"
        assert np.array_equal(cls_h, cls64), f"{what}: cls differs in {int((cls_h != cls64).sum())} rows"
        assert np.array_equal(val_h.view(np.int64), val64.view(np.int64)), f"{what}: val differs"
        assert np.array_equal(t_h, want), f"{what}: t_rank differs in {int((t_h != want).sum())} rows"
        assert np.isposinf(t_h[~mask]).all()
        assert ref.clusters_are_ranked(cls_h, t_h, mask, nw)
        again = tdea_ops.theta_rank(d_obj, d_w, d_mask)
        assert torch.equal(again.view(torch.int32), t_rank.view(torch.int32))
    print(f"[tdea] ({nw}, {m}) n {n} {kind}: cls, val and t_rank equal under 4 masks; largest cluster "
          f"{int(np.bincount(cls64, minlength=nw).max())} rows")


def test_equal_values_rank_by_position():
    obj, w, _, _ = ref.cached_case(91, 3, "front")
    o = np.array(obj).copy()
    o[10:40] = o[10]  # 30 equal rows in one cluster
    mask = np.ones(o.shape[0], dtype=bool)
    want, cls64, val64 = ref.theta_rank(o, w, mask)
    t_rank, cls, val = tdea_ops.theta_rank(_dev(o), _dev(w), _dev(mask), return_parts=True)
    assert np.array_equal(cls.cpu().numpy(), cls64) and np.array_equal(val.cpu().numpy(), val64)
    t_h = t_rank.cpu().numpy()
    assert np.array_equal(t_h, want) and (np.diff(t_h[10:40]) == 1).all()


@pytest.mark.parametrize("mask_name", ["all", "every7"])
def test_a_zero_row_and_a_nan_row(mask_name):
    obj, w, _, _ = ref.cached_case(300, 3, "uniform")
    o = np.array(obj).copy()
    o[3] = 0.0
    o[8, 1] = np.nan
    o[11] = np.nan
    n, nw = o.shape[0], w.shape[0]
    mask = ref.masks(n)[mask_name]
    t_rank, cls, val = tdea_ops.theta_rank(_dev(o), _dev(w), _dev(mask), return_parts=True)
    torch.cuda.synchronize()
    assert t_rank.shape == (n,) and cls.shape == (n,) and val.shape == (n,)
    assert ref.clusters_are_ranked(cls.cpu().numpy(), t_rank.cpu().numpy(), mask, nw)


# ---------------------------------------------------------------- 2. caps
def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    w = _dev(ref.directions(91, 3))
    n = tdea_ops.N_CAP + 1
    obj = _dev(ref.objectives(n, 3, "front", 1))
    mask = _dev(ref.masks(n)["every7"])
    want = tdea_algo.theta_nd_sort(obj, w, mask)
    _no_kernel(monkeypatch, *KERNELS)
    got = tdea_ops.theta_rank(obj, w, mask)
    assert got.is_cuda and torch.equal(got, want)


def test_over_the_objective_cap_and_float64_run_the_torch_path(monkeypatch):
    for m, dtype in [(tdea_ops.M_CAP + 1, torch.float32), (3, torch.float64)]:
        w = _dev(ref.directions(20, m)).to(dtype)
        n = 2 * w.shape[0]
        obj = _dev(ref.objectives(n, m, "front", 1)).to(dtype)
        mask = _dev(ref.masks(n)["every7"])
        want = tdea_algo.theta_nd_sort(obj, w, mask)
        with monkeypatch.context() as mp:
            _no_kernel(mp, *KERNELS)
            assert torch.equal(tdea_ops.theta_rank(obj, w, mask), want)


# ---------------------------------------------------------------- 3. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=5, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.TDEA(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


@pytest.fixture
def kernel_calls(monkeypatch):
    ops, calls = _ext.ops(), {"tdea_theta_rank": 0}

    class Counting:
        def __getattr__(self, name):
            if name in calls:
                calls[name] += 1
            return getattr(ops, name)

    monkeypatch.setattr(tdea_ops._ext, "ops", lambda: Counting())
    return calls


def test_generation_is_captured_and_is_bitwise_the_eager_one(kernel_calls):
    _, a = _run(False)
    assert kernel_calls["tdea_theta_rank"] >= 4  # every tell after the initial one
    before = dict(kernel_calls)
    wf, b = _run(True)
    assert wf._graph is not None
    assert kernel_calls["tdea_theta_rank"] > before["tdea_theta_rank"]
    assert torch.isfinite(a.fitness).all()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
    _, c = _run(True)
    assert torch.equal(b.population, c.population) and torch.equal(b.fitness, c.fitness)


def test_tell_calls_the_kernel_and_ask_and_tell_read_nothing_on_the_host(monkeypatch, kernel_calls):
    """θ-DEA's ``ask`` is a random mating pool and the variation: the θ-ranking, and so the kernel, is ``tell``'s."""
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.TDEA(lb, ub, M_, POP)
    wf = StdWorkflow(algo, DTLZ2(d=D_, m=M_), graph=False)
    st = wf.init(rnd.PRNGKey(3, device="cuda"))
    for _ in range(2):
        st = wf.step(st)
    a = st.get_child_state("algorithm")
    fit = torch.rand(algo.pop_size, M_, device="cuda")
    torch.cuda.synchronize()

    def forbidden(*args, **kwargs):
        raise AssertionError("host read on the generation path")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        for name in ("item", "tolist", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            mp.setattr(torch.Tensor, name, forbidden)
        _, a = algo.ask(a)
        n1 = kernel_calls["tdea_theta_rank"]
        a = algo.tell(a, fit)
        n2 = kernel_calls["tdea_theta_rank"]
    torch.cuda.synchronize()
    assert n2 == n1 + 1
    assert a.fitness.shape == (algo.pop_size, M_) and torch.isfinite(a.fitness).all()


def test_tdea_converges_on_dtlz2_on_the_device():
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] θ-DEA, DTLZ2 d 12 m 3, N 100, 100 generations: {igd:.4f}")
    assert igd < 0.1
