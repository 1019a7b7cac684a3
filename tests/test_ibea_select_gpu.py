"""``ibea_select.hip`` against its oracles, and IBEA generations captured into a hipGraph (MI355X,
marked gpu).

Fitness kernel: the rule of ``tests/test_cmaes_kernels_gpu.py``.  With ``e_t`` the largest
deviation of the float32 torch evaluation (on the CPU) from a float64 evaluation of the same
float32 objectives and ``e_k`` the kernel's, ``e_k <= 4·e_t + 2·ulp32(max |ref64|)``, for f and
for C.  The kernel sums a column in another order (64 strided partials, then a tree).

Truncation kernel, exact: on inputs whose float64 removal sequence is decided by a relative
margin of at least 5e-5 at every step (``_reference64``; the float32 error of a running fitness,
n initial terms and n_remove updates at 6e-8 of its peak each, stays below 2.3e-5 there), the
kernel removes the same rows in the same order.

Truncation kernel, certificate: every other input.  The kernel's own removal order is replayed
in float64; ``slack_t = f64[x_t] − min f64`` is how far from the float64 minimum the row it
removed at step t was, ``s_k`` the largest slack, ``s_t`` the same for the order of the float32
torch loop on the CPU, and ``s_k <= 4·s_t + 2·ulp32(peak |f64|)``.

Observed on an MI355X (gfx950), worst over the cases of each test:

==========================  ==================================================
quantity                    worst ratio
==========================  ==================================================
f, e_k / e_t                1.20 ((65, 2) uniform; 1.10 at most elsewhere)
C, e_k / e_t                1.00 (the same bits as torch in every case)
order, s_k / s_t            1.59 ((4096, 2) front: s_k 1.46e-3, s_t 9.2e-4)
==========================  ==================================================

s_k and s_t are both 0 (every removed row was the float64 minimum) in all ``uniform`` cases and
in the ``front`` cases up to n = 1000; the other ``front`` ratios are 1.00 (2049, 8192), 0.46
(4097) and 1.27 (8191).  At the sizes where the truncation kernel changes its rows per thread or
its thread count (256 / 257 … 2048 / 2049, ``STEPS``) both are 0 but for (4097, 5): 1.00.  The
exact cases' strict gaps are 3.0e-2, 1.2e-3, 9.1e-5, 1.4e-4,
1.9e-4 and 7.1e-5.
"""
import functools

import pytest
import torch

import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo.ibea import cal_fitness, ibea_truncate
from evoxmi.ops import _ext
from evoxmi.ops import ibea as ibea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu

KAPPA = 0.05


def _ulp32(ref64):
    """Spacing of float32 at |ref| (float64 tensor): 2^(e − 24) for |ref| = m·2^e, m in [0.5, 1)."""
    _, e = torch.frexp(ref64.abs().clamp_min(2.0**-126))
    return (((e.to(torch.int64) - 24).clamp_min(-149) + 1023) << 52).view(torch.float64)


def _rule(what, out, t32, ref64):
    """e_k <= 4·e_t + 2 ulp32(max |ref|), see the module docstring."""
    out, t32, ref64 = out.detach().cpu(), t32.detach().cpu(), ref64.detach().cpu()
    assert out.dtype == torch.float32 and t32.dtype == torch.float32 and ref64.dtype == torch.float64
    assert out.shape == ref64.shape and t32.shape == ref64.shape, (what, out.shape, t32.shape, ref64.shape)
    assert torch.isfinite(out).all(), what
    e_k = float((out.double() - ref64).abs().max())
    e_t = float((t32.double() - ref64).abs().max())
    floor = 2.0 * float(_ulp32(ref64.abs().max().reshape(1)))
    print(f"[rule] {what}: e_k {e_k:.3e} e_t {e_t:.3e} e_k/e_t {e_k / e_t if e_t > 0 else float('inf'):.3f} floor {floor:.3e}")
    assert e_k <= 4.0 * e_t + floor, f"{what}: e_k {e_k:.3e} > 4·e_t + floor = {4.0 * e_t + floor:.3e} (e_t {e_t:.3e})"


def _objectives(n, m, kind):
    obj = torch.rand(n, m, generator=torch.Generator().manual_seed(100 * n + m))
    if kind == "front":
        obj = obj / obj.sum(1, keepdim=True)  # rows on the simplex, as near a front
    return obj


def _present_select(obj, kappa, n_keep):
    """The selection as IBEA's tell wrote it out before ``evoxmi.ops.ibea``."""
    f, I, C = cal_fitness(obj, kappa)
    keep = ibea_truncate(f, I, C, kappa, obj.shape[0] - n_keep)
    return torch.argsort((~keep).to(torch.int64), stable=True)[:n_keep]


def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(ibea_ops._ext, "ops", lambda: NoKernel())


# ---------------------------------------------------------------- float64 references
def _fitness64(obj32, chunk=1024):
    """(f, C, o) in float64 of float32 objectives; I is formed per objective k over row chunks,
    never as an (n, n, m) tensor."""
    o = obj32.double()
    mn, mx = o.min(), o.max()
    o = (o - mn) / (mx - mn)
    n, m = o.shape

    def I_rows(i0):
        I = o[i0:i0 + chunk, 0, None] - o[None, :, 0]
        for k in range(1, m):
            I = torch.maximum(I, o[i0:i0 + chunk, k, None] - o[None, :, k])
        return I

    C = torch.zeros(n, dtype=torch.float64)
    for i0 in range(0, n, chunk):
        C = torch.maximum(C, I_rows(i0).abs().amax(0))
    s = torch.zeros(n, dtype=torch.float64)
    for i0 in range(0, n, chunk):
        s += torch.exp(-I_rows(i0) / C[None, :] / KAPPA).sum(0)
    return 1 - s, C, o


def _correct(f, o, C, x):
    """One step of the loop along row x, in place: the correction and f[x] = max f."""
    f += torch.exp(-(o[x][None, :] - o).amax(1) / C[x] / KAPPA)
    f[x] = f.max()


def _reference64(obj32, n_remove):
    """The removal order of the loop in float64 and its strict gap: over the steps, the least
    (second smallest f − smallest f) / (largest |f_j| seen so far over all j and steps)."""
    f, C, o = _fitness64(obj32)
    peak, gap, order = float(f.abs().max()), float("inf"), []
    for _ in range(n_remove):
        two = torch.sort(f).values[:2]
        if two.numel() == 2:
            gap = min(gap, float(two[1] - two[0]) / peak)
        x = int(torch.argmin(f))
        order.append(x)
        _correct(f, o, C, x)
        peak = max(peak, float(f.abs().max()))
    return torch.tensor(order, dtype=torch.int64), gap


def _replay64(start, order):
    """The largest slack of a removal order replayed in float64 from ``start = _fitness64(obj)``,
    and the peak |f64| of the replay."""
    f, C, o = start[0].clone(), start[1], start[2]
    peak, slack = float(f.abs().max()), 0.0
    for x in order.tolist():
        slack = max(slack, float(f[x] - f.min()))
        _correct(f, o, C, x)
        peak = max(peak, float(f.abs().max()))
    return slack, peak


def _certificate(what, obj, order, n_keep):
    n = obj.shape[0]
    order = order.cpu()
    assert order.shape == (n - n_keep,) and int(order.min()) >= 0 and int(order.max()) < n
    t_order = ibea_ops.select(obj, KAPPA, n_keep, return_order=True)[1]  # the float32 torch loop on the CPU
    start = _fitness64(obj)
    s_k, peak = _replay64(start, order)
    s_t, _ = _replay64(start, t_order)
    floor = 2.0 * float(_ulp32(torch.tensor([peak], dtype=torch.float64)))
    print(f"[certificate] {what}: s_k {s_k:.3e} s_t {s_t:.3e} s_k/s_t {s_k / s_t if s_t > 0 else float('inf'):.3f} floor {floor:.3e}")
    assert s_k <= 4.0 * s_t + floor, f"{what}: s_k {s_k:.3e} > 4·s_t + floor = {4.0 * s_t + floor:.3e} (s_t {s_t:.3e})"


def _sorted_complement(n, order):
    keep = torch.ones(n, dtype=torch.bool)
    keep[order.cpu()] = False
    return torch.nonzero(keep).flatten()


# ---------------------------------------------------------------- 1. fitness kernel
@functools.lru_cache(maxsize=None)
def _fitness_references(n, m, kind):
    """The objectives, the float32 torch evaluation on the CPU and the float64 one of the same inputs."""
    obj = _objectives(n, m, kind)
    f, _, C = cal_fitness(obj, KAPPA)
    f64, C64, _ = _fitness64(obj)
    return obj, (f, C), (f64, C64)


SHAPES = [(1, 2), (2, 2), (65, 2), (200, 3), (1000, 3), (2050, 5), (600, 10), (300, ibea_ops.M_CAP)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_fitness_follows_the_rule(n, m, kind):
    obj, t32, ref64 = _fitness_references(n, m, kind)
    assert ref64[0].dtype == torch.float64
    f, C = ibea_ops.fitness(obj.cuda(), KAPPA)
    assert f.is_cuda and f.dtype == torch.float32 and f.shape == (n,) and C.dtype == torch.float32 and C.shape == (n,)
    if n <= 2:
        for got, want in zip((f, C), t32):
            assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want))
        if n == 1:
            assert torch.equal(C.cpu(), torch.zeros(1)) and bool(torch.isnan(f).all())  # 0 / 0, as torch
    else:
        _rule(f"f ({n}, {m}) {kind}", f, t32[0], ref64[0])
        _rule(f"C ({n}, {m}) {kind}", C, t32[1], ref64[1])
    again = ibea_ops.fitness(obj.cuda(), KAPPA)
    assert torch.equal(again[0].view(torch.int32), f.view(torch.int32)) and torch.equal(again[1].view(torch.int32), C.view(torch.int32))


# ---------------------------------------------------------------- 2. truncation, exact
EXACT = [(3, 2), (8, 2), (64, 2), (65, 3), (130, 3), (257, 5)]


@pytest.mark.parametrize("n,m", EXACT)
def test_truncation_matches_the_float64_order(n, m):
    obj = _objectives(n, m, "front")
    n_keep = n // 2
    want, gap = _reference64(obj, n - n_keep)
    print(f"[exact] ({n}, {m}) strict gap {gap:.3e}")
    assert gap >= 5e-5, f"({n}, {m}): strict gap {gap:.3e}"
    assert torch.equal(ibea_ops.select(obj, KAPPA, n_keep, return_order=True)[1], want)  # float32 torch on the CPU
    idx, order = ibea_ops.select(obj.cuda(), KAPPA, n_keep, return_order=True)
    assert idx.is_cuda and idx.dtype == torch.int64 and order.dtype == torch.int64
    assert torch.equal(order.cpu(), want)
    assert torch.equal(idx.cpu(), _sorted_complement(n, want))


# ---------------------------------------------------------------- 3. truncation, certificate
ALL_SIZES = [(200, 3), (600, 10), (300, 16), (1000, 3), (2049, 3), (4096, 2), (4097, 2), (8191, 3), (8192, 3)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", ALL_SIZES)
def test_truncation_certificate(n, m, kind):
    obj = _objectives(n, m, kind)
    n_keep = n // 2
    idx, order = ibea_ops.select(obj.cuda(), KAPPA, n_keep, return_order=True)
    assert idx.shape == (n_keep,) and order.shape == (n - n_keep,)
    _certificate(f"({n}, {m}) {kind}", obj, order, n_keep)
    idx = idx.cpu()
    assert bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < n
    assert not torch.isin(idx, order.cpu()).any()
    assert torch.equal(idx, _sorted_complement(n, order)[:n_keep])


# both sides of every step in rows per thread and in threads of the truncation kernel that ALL_SIZES leaves out,
# with the objectives in registers (m = 3) and re-read (m = 5)
STEPS = [(256, 3), (257, 5), (512, 3), (513, 3), (1024, 5), (1025, 3), (2048, 3), (2049, 5), (4097, 5)]


@pytest.mark.parametrize("n,m", STEPS)
def test_truncation_certificate_at_the_kernel_steps(n, m):
    obj = _objectives(n, m, "front")
    n_keep = n // 2
    idx, order = ibea_ops.select(obj.cuda(), KAPPA, n_keep, return_order=True)
    _certificate(f"({n}, {m}) front", obj, order, n_keep)
    assert torch.equal(idx.cpu(), _sorted_complement(n, order)[:n_keep])


# ---------------------------------------------------------------- 4. ties
def test_duplicate_rows_leave_in_index_order():
    o = _objectives(100, 3, "front")
    obj = torch.cat([o, o]).cuda()
    _, order = ibea_ops.select(obj, KAPPA, 100, return_order=True)
    step = [10**6] * 200  # the first step at which a row leaves
    for t, x in enumerate(order.tolist()):
        step[x] = min(step[x], t)
    assert all(step[i] <= step[i + 100] for i in range(100)), "a copy left before its original"
    assert torch.equal(ibea_ops.select(obj, KAPPA, 100, return_order=True)[1], order)


# ---------------------------------------------------------------- 5. non-finite
@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "all_equal"])
def test_nonfinite_objectives_select_as_torch_does(bad):
    obj = _objectives(200, 3, "uniform").cuda()
    if bad == "all_equal":
        obj = torch.full_like(obj, 0.5)  # mx == mn: 0 / 0
    else:
        obj[17, 1] = float(bad)
    assert bool(torch.isnan(cal_fitness(obj, KAPPA)[0]).all())  # the scalar normalisation spreads it
    want = _present_select(obj, KAPPA, 100)
    assert torch.equal(want.cpu(), torch.arange(1, 101))  # row 0 is the arg-min of every step
    got = ibea_ops.select(obj, KAPPA, 100)
    assert torch.equal(got, want)


# ---------------------------------------------------------------- 6. other n_keep
def test_one_step_and_all_but_one():
    n, m = 130, 3
    obj = _objectives(n, m, "front")
    want, gap = _reference64(obj, 1)
    assert gap >= 5e-5
    idx, order = ibea_ops.select(obj.cuda(), KAPPA, n - 1, return_order=True)
    assert torch.equal(order.cpu(), want) and torch.equal(idx.cpu(), _sorted_complement(n, want))
    idx, order = ibea_ops.select(obj.cuda(), KAPPA, 1, return_order=True)
    assert idx.shape == (1,)
    _certificate(f"({n}, {m}) front n_keep 1", obj, order, 1)
    assert torch.equal(idx.cpu(), _sorted_complement(n, order)[:1])


def test_keeping_every_row_launches_nothing(monkeypatch):
    obj = _objectives(130, 3, "front").cuda()
    _no_kernel(monkeypatch, "ibea_fitness", "ibea_truncate")
    idx = ibea_ops.select(obj, KAPPA, 130)
    assert idx.is_cuda and torch.equal(idx.cpu(), torch.arange(130))


# ---------------------------------------------------------------- 7. caps
def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    n = ibea_ops.N_CAP + 2
    obj = _objectives(n, 3, "uniform").cuda()
    want = _present_select(obj, KAPPA, n // 2)
    _no_kernel(monkeypatch, "ibea_truncate")
    got = ibea_ops.select(obj, KAPPA, n // 2)
    assert got.is_cuda and torch.equal(got, want)


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    obj = _objectives(100, ibea_ops.M_CAP + 1, "uniform").cuda()
    f, _, C = cal_fitness(obj, KAPPA)
    want = _present_select(obj, KAPPA, 50)
    _no_kernel(monkeypatch, "ibea_fitness", "ibea_truncate")
    got = ibea_ops.fitness(obj, KAPPA)
    assert torch.equal(got[0], f) and torch.equal(got[1], C)
    assert torch.equal(ibea_ops.select(obj, KAPPA, 50), want)


# ---------------------------------------------------------------- 8. the algorithms
def _run(name, graph, gens=5, seed=11):
    d, m, pop = 12, 3, 100
    lb, ub = torch.zeros(d, device="cuda"), torch.ones(d, device="cuda")
    wf = StdWorkflow(getattr(A, name)(lb, ub, m, pop), DTLZ2(d=d, m=m), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


def _same_fitness(a, b):
    fa, fb = a.fitness, b.fitness
    fin = torch.isfinite(fa)
    assert torch.equal(fin, torch.isfinite(fb))
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)


@pytest.fixture
def kernel_calls(monkeypatch):
    ops, calls = _ext.ops(), {"ibea_fitness": 0, "ibea_truncate": 0}

    class Counting:
        def __getattr__(self, name):
            if name in calls:
                calls[name] += 1
            return getattr(ops, name)

    monkeypatch.setattr(ibea_ops._ext, "ops", lambda: Counting())
    return calls


def test_generation_is_captured_and_matches_eager(kernel_calls):
    _, a = _run("IBEA", False)
    assert kernel_calls["ibea_fitness"] >= 2 and kernel_calls["ibea_truncate"] >= 1  # ask and tell
    before = dict(kernel_calls)
    wf, b = _run("IBEA", True)
    assert wf._graph is not None
    assert kernel_calls["ibea_fitness"] > before["ibea_fitness"] and kernel_calls["ibea_truncate"] > before["ibea_truncate"]
    _same_fitness(a, b)


def test_graph_runs_are_bitwise_reproducible(kernel_calls):
    _, a = _run("IBEA", True)
    assert kernel_calls["ibea_fitness"] > 0 and kernel_calls["ibea_truncate"] > 0
    _, b = _run("IBEA", True)
    assert torch.equal(a.population, b.population)
    assert torch.equal(a.fitness, b.fitness)


def test_bce_ibea_still_falls_back_to_eager():
    import warnings

    _, a = _run("BCEIBEA", False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wf, b = _run("BCEIBEA", "auto")
    assert wf._graph is None
    _same_fitness(a, b)
