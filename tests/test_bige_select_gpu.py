"""``bige_select.hip`` against the host reference of its contract, and BiGE generations captured into a hipGraph
(MI355X, marked gpu).  The reference is numpy float64 on the same float32 objectives (``_bige_reference.py``;
``test_bige_select.py`` pins it to the torch path).  The radius r is the device's own float32 word, computed by the torch
expression the op uses: it is an input of the contract.

Inputs: ``uniform`` is rand in [0, 1]^m, ``front`` is |normal| + 1e-3 normalised to the unit sphere.  Masks: all rows,
every 7th row out, one row only, none.  The shapes include both sides of the crowding launch's LDS tile at every
instantiation (1024 rows at m ≤ 4, 512 at m ≤ 8, 256 at m ≤ 16).

Asserted per case: ``pr`` equals the reference bit for bit; ``cd`` is within (n + 2)·2⁻⁵³ relative (every term of the sum
is non-negative, so any summation order is within γ_{n−1}; the square root halves that and adds one rounding), and is 0
where the reference's is 0; ``bi`` is exactly ``float32`` of the kernel's own float64 parts; the rows outside the mask
are +inf; a second call is bitwise equal.

Observed on an MI355X (gfx950), worst over the cases of each test:

==============================  ==============================================================
quantity                        worst observed
==============================  ==============================================================
pr                              equal as float64 words in all 30 (shape, kind) cases, 4 masks
cd, relative error              2.79·2⁻⁵³ at (8192, 3) front (bound 8194·2⁻⁵³); 2.74·2⁻⁵³ at
                                (512, 5) front; 1.2–2.0·2⁻⁵³ at n ≤ 65; exactly 0 at n ≤ 3
cd = 0 in the reference         0 in the kernel in every case (549 of 1000 rows at (1000, 10)
                                uniform, all 257 at (257, 16) uniform)
peak memory, (8192, 3)          +459 776 bytes across a call (bound 4 718 592; one (n, n)
                                float32 array is 268 435 456)
IGD after 100 generations       0.0708 (the CPU run measures .071)
==============================  ==============================================================
"""
import functools

import numpy as np
import pytest
import torch

import _bige_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import bige as bige_algo
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import bige as bige_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.tensor(np.array(a)).cuda()


def _radius(mask, m):
    """The device's float32 word, by the expression of ``ops.bige.estimate``."""
    return np.float32((1 / _dev(mask).sum().to(torch.float32) ** (1 / m)).item())


def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(bige_ops._ext, "ops", lambda: NoKernel())


# ---------------------------------------------------------------- 1. the estimate
SHAPES = [(1, 1), (2, 2), (3, 1), (63, 3), (64, 3), (65, 2), (257, 16), (1000, 10), (1025, 3), (2049, 5), (8192, 3)]
TILE_SIDES = [(1024, 3), (512, 5), (513, 5), (256, 16)]  # with (1025, 3) and (257, 16) above


@functools.lru_cache(maxsize=None)
def _reference(n, m, kind, mask_name, r_bits):
    fit = ref.cached_objectives(n, m, kind, 100 * n + m)
    return ref.estimate(fit, ref.masks(n)[mask_name], np.uint32(r_bits).view(np.float32))


def test_the_tile_sides_are_the_kernels():
    assert [bige_ops.tile_rows(m) for m in (1, 3, 4, 5, 8, 9, 16)] == [1024, 1024, 1024, 512, 512, 256, 256]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", SHAPES + TILE_SIDES)
def test_estimate_against_the_reference(n, m, kind):
    fit = ref.cached_objectives(n, m, kind, 100 * n + m)
    d_fit = _dev(fit)
    for name, mask in ref.masks(n).items():
        r = _radius(mask, m)
        _, pr64, cd64, gap = _reference(n, m, kind, name, int(np.float32(r).view(np.uint32)))
        d_mask = _dev(mask)
        bi, pr, cd = bige_ops.estimate(d_fit, d_mask, return_parts=True)
        assert bi.is_cuda and bi.dtype == torch.float32 and bi.shape == (n, 2)
        assert pr.dtype == torch.float64 and cd.dtype == torch.float64 and pr.shape == (n,) and cd.shape == (n,)
        bi_h, pr_h, cd_h = bi.cpu().numpy(), pr.cpu().numpy(), cd.cpu().numpy()
        assert np.isposinf(bi_h[~mask]).all() and np.isposinf(pr_h[~mask]).all() and np.isposinf(cd_h[~mask]).all()
        assert np.array_equal(pr_h.view(np.int64), pr64.view(np.int64)), f"({n}, {m}) {kind} {name}: pr differs"
        want, got = cd64[mask], cd_h[mask]
        err = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0), initial=0.0))
        bound = (n + 2) * 2.0**-53
        print(f"[bige] ({n}, {m}) {kind} {name}: cd rel {err:.3e} = {err * 2.0**53:.2f}·2^-53 (bound {n + 2}·2^-53), thr_gap {gap:.3e}, "
              f"cd = 0 in {int((want == 0).sum())} of {int(mask.sum())} rows")
        assert err <= bound
        assert (got[want == 0] == 0).all()
        assert np.array_equal(bi_h.view(np.int32), np.stack([pr_h, cd_h], 1).astype(np.float32).view(np.int32))
        again = bige_ops.estimate(d_fit, d_mask)
        assert torch.equal(again.view(torch.int32), bi.view(torch.int32))


def test_a_block_of_duplicates_inside_a_front():
    n = 400
    fit = ref.objectives(n, 3, "front", 6).copy()
    fit[100:150] = fit[100]  # 50 equal rows: every pair of them contributes exactly 1 (w = 2, d = 0)
    mask = np.ones(n, dtype=bool)
    _, pr, cd = bige_ops.estimate(_dev(fit), _dev(mask), return_parts=True)
    cd, pr = cd.cpu().numpy(), pr.cpu().numpy()
    assert (cd[100:150] ** 2 >= 49).all()
    assert np.unique(cd[100:150].view(np.int64)).size == 1 and np.unique(pr[100:150].view(np.int64)).size == 1
    _, pr64, cd64, _ = ref.estimate(fit, mask, _radius(mask, 3))
    assert np.array_equal(pr, pr64) and np.max(np.abs(cd - cd64) / cd64) <= (n + 2) * 2.0**-53


def test_no_n_squared_memory():
    n, m = 8192, 3
    fit, mask = _dev(ref.cached_objectives(n, m, "front", 100 * n + m)), torch.ones(n, dtype=torch.bool, device="cuda")
    bige_ops.estimate(fit, mask)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    bi = bige_ops.estimate(fit, mask)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[bige] peak memory of a call at ({n}, {m}): {rise} bytes (one (n, n) float32 array is {4 * n * n})")
    assert bi.shape == (n, 2) and rise <= 4 * n * (bige_ops.M_CAP + 2) * 8


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_objectives_end_and_keep_the_shapes(bad):
    n = 300
    fit = ref.objectives(n, 3, "uniform", 2).copy()
    fit[17, 1] = bad
    mask = ref.masks(n)["every7"]
    bi = bige_ops.estimate(_dev(fit), _dev(mask))
    torch.cuda.synchronize()
    assert bi.shape == (n, 2) and np.isposinf(bi.cpu().numpy()[~mask]).all()


# ---------------------------------------------------------------- 2. caps
def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    n = bige_ops.N_CAP + 1
    fit = _dev(ref.objectives(n, 3, "uniform", 1))
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[::3] = True
    want = bige_algo.estimate(fit, mask)
    _no_kernel(monkeypatch, "bige_estimate")
    got = bige_ops.estimate(fit, mask)
    assert got.is_cuda and torch.equal(got, want)


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    fit = _dev(ref.objectives(100, bige_ops.M_CAP + 1, "uniform", 1))
    mask = _dev(ref.masks(100)["every7"])
    want = bige_algo.estimate(fit, mask)
    _no_kernel(monkeypatch, "bige_estimate")
    assert torch.equal(bige_ops.estimate(fit, mask), want)


def test_float64_input_runs_the_torch_path(monkeypatch):
    fit = _dev(ref.objectives(100, 3, "uniform", 1)).to(torch.float64)
    mask = _dev(ref.masks(100)["every7"])
    want = bige_algo.estimate(fit, mask)
    _no_kernel(monkeypatch, "bige_estimate")
    assert torch.equal(bige_ops.estimate(fit, mask), want)


# ---------------------------------------------------------------- 3. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=5, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.BiGE(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


@pytest.fixture
def kernel_calls(monkeypatch):
    ops, calls = _ext.ops(), {"bige_estimate": 0}

    class Counting:
        def __getattr__(self, name):
            if name in calls:
                calls[name] += 1
            return getattr(ops, name)

    monkeypatch.setattr(bige_ops._ext, "ops", lambda: Counting())
    return calls


def test_generation_is_captured_and_is_bitwise_the_eager_one(kernel_calls):
    _, a = _run(False)
    assert kernel_calls["bige_estimate"] >= 2  # ask and tell
    before = dict(kernel_calls)
    wf, b = _run(True)
    assert wf._graph is not None
    assert kernel_calls["bige_estimate"] >= before["bige_estimate"] + 2
    assert torch.isfinite(a.fitness).all()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
    _, c = _run(True)
    assert torch.equal(b.population, c.population) and torch.equal(b.fitness, c.fitness)


def test_ask_and_tell_call_the_kernel_and_read_nothing_on_the_host(monkeypatch, kernel_calls):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.BiGE(lb, ub, M_, POP)
    wf = StdWorkflow(algo, DTLZ2(d=D_, m=M_), graph=False)
    st = wf.init(rnd.PRNGKey(3, device="cuda"))
    for _ in range(2):
        st = wf.step(st)
    a = st.get_child_state("algorithm")
    fit = torch.rand(POP, M_, device="cuda")
    torch.cuda.synchronize()

    def forbidden(*args, **kwargs):
        raise AssertionError("host read on the generation path")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        for name in ("item", "tolist", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            mp.setattr(torch.Tensor, name, forbidden)
        n0 = kernel_calls["bige_estimate"]
        _, a = algo.ask(a)
        n1 = kernel_calls["bige_estimate"]
        a = algo.tell(a, fit)
        n2 = kernel_calls["bige_estimate"]
    torch.cuda.synchronize()
    assert n1 == n0 + 1 and n2 == n1 + 1
    assert a.fitness.shape == (POP, M_) and torch.isfinite(a.fitness).all()


def test_bige_converges_on_dtlz2_on_the_device():
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] BiGE, DTLZ2 d 12 m 3, N 100, 100 generations: {igd:.4f}")
    assert igd < 0.1
