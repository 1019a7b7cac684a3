"""``rvea_select.hip`` against the numpy reference of ``_rvea_reference.py``, and RVEA, RVEA* and LMOCSO generations
captured into a hipGraph (MI355X, marked gpu).

The kernels' contract (the docstring of ``evoxmi/ops/rvea.py``) is float64 arithmetic in a stated order without FMA, so
``cos_best`` is compared exactly: ``arg`` equal and ``best`` equal as float64 words, in all four uses (γ, association,
regeneration, truncation).  ``select`` is compared on fixtures that ``qualify`` (a ≥ 1e-12, b ≥ 1e-9: the margins an ulp
of ``acos`` cannot cross): ``next_ind`` and ``empty`` equal, ``apd`` and γ within 1e-12 relative.

Observed on an MI355X (gfx950): every case equal; the fixtures' a from 6.1e-9 at (8192, 4095, 3) to 2.4e-1, b from
4.0e-6 up; peak memory over a select and a truncation ``cos_best`` at (8192, 4095, 3) +0.43 MB; RVEA* keeps 74 of 167
valid rows at the truncating tell; IGD after 100 captured generations RVEA 0.0549, RVEA* 0.0703, LMOCSO 0.0670."""
import warnings

import numpy as np
import pytest
import torch

import _rvea_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import rvea as rvea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu

INF = float("inf")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached fixtures are read-only


def _words(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# (n, nv, m, NaN share): the smallest case, fewer vectors than lanes, NaN rows, m = 5, m at the cap with a lane one vector
# beyond a full stride, many NaN rows, counts just past multiples of 64 and 1024, the bench's size
SHAPES = [(2, 1, 2, 0.0), (20, 10, 2, 0.0), (182, 91, 3, 0.3), (170, 85, 5, 0.0), (130, 65, 16, 0.0), (600, 300, 3, 0.5),
          (2050, 1035, 3, 0.0), (8192, 4096, 3, 0.0)]
CASES = [s + (kind,) for s in SHAPES for kind in ("uniform", "rand")]
THETA = 0.49


def _seed(n, nv, m, share, kind):
    """The first seed whose fixture qualifies (host arithmetic only; cached)."""
    for seed in range(20):
        r = ref.cached_select(n, nv, m, share, kind, seed, THETA)
        if ref.qualifies(r["a"], r["b"]):
            return seed
    raise AssertionError("no qualifying fixture in 20 seeds")


# ---------------------------------------------------------------- 1. cos_best
def _check_cos_best(A, B, want, **kw):
    best, arg = rvea_ops.cos_best(_dev(A), _dev(B), **{k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    assert best.is_cuda and best.dtype == torch.float64 and arg.dtype == torch.int64 and best.shape == arg.shape == (A.shape[0],)
    assert np.array_equal(arg.cpu().numpy(), want[1]), "arg differs from the reference"
    assert np.array_equal(_words(best.cpu().numpy()), _words(want[0])), "best differs from the reference in its float64 words"


@pytest.mark.parametrize("n,nv,m,share,kind", CASES)
def test_cos_best_equals_the_reference_in_all_four_uses(n, nv, m, share, kind):
    f, v = ref.cached_case(n, nv, m, share, kind, _seed(n, nv, m, share, kind))
    cm = ref.colmin(f)
    _check_cos_best(v, v, ref.cos_best(v, v, clamp=True, self_zero=True), clamp=True, self_zero=True)  # γ
    _check_cos_best(f, v, ref.cos_best(f, v, shift=cm, floor=1e-32, clamp=True), shift=cm, floor=1e-32, clamp=True)  # association
    _check_cos_best(f, v, ref.cos_best(f, v, shift=cm), shift=cm)  # regeneration
    _check_cos_best(f, f, ref.cos_best(f, f, self_zero=True), self_zero=True)  # truncation


# ---------------------------------------------------------------- 2. select
def _check_select(f, v, theta, want):
    got = rvea_ops.select(_dev(f), _dev(v), theta, return_info=True)
    next_ind, empty, arg, apd, gamma = (t.cpu().numpy() for t in got)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.bool and next_ind.shape == empty.shape == (v.shape[0],)
    assert np.array_equal(arg, want["arg"])
    assert np.array_equal(empty, want["empty"]) and np.array_equal(next_ind, want["next_ind"])
    assert np.allclose(gamma, want["gamma"], rtol=1e-12, atol=0.0)
    live = arg >= 0
    assert np.allclose(apd[live], want["apd"][live], rtol=1e-12, atol=0.0)
    return next_ind, empty


@pytest.mark.parametrize("n,nv,m,share,kind", CASES)
def test_select_equals_the_reference(n, nv, m, share, kind):
    seed = _seed(n, nv, m, share, kind)
    f, v = ref.cached_case(n, nv, m, share, kind, seed)
    want = ref.cached_select(n, nv, m, share, kind, seed, THETA)
    print(f"[rvea] ({n}, {v.shape[0]}, {m}) {kind} NaN {share} seed {seed}: a {want['a']:.1e} b {want['b']:.1e}, "
          f"{int((~want['empty']).sum())} vectors with a member")
    next_ind, empty = _check_select(f, v, THETA, want)
    again = rvea_ops.select(_dev(f), _dev(v), THETA)  # determinism
    assert np.array_equal(again[0].cpu().numpy(), next_ind) and np.array_equal(again[1].cpu().numpy(), empty)


@pytest.mark.parametrize("theta", [0.0, 0.01, 1.0])
def test_select_at_other_thetas(theta):
    n, nv, m, share, kind = 600, 300, 3, 0.5, "uniform"
    seed = _seed(n, nv, m, share, kind)
    want = ref.cached_select(n, nv, m, share, kind, seed, theta)
    assert ref.qualifies(want["a"], want["b"])
    _check_select(*ref.cached_case(n, nv, m, share, kind, seed), theta, want)


# ---------------------------------------------------------------- 4. hand cases
@pytest.mark.parametrize("name", list(ref.hand_cases()))
def test_hand_cases(name):
    f, v, theta = ref.hand_cases()[name]
    _check_select(f, v, theta, ref.select(f, v, theta))


# ---------------------------------------------------------------- 5. theta
def test_theta_as_a_float_and_as_a_device_word_give_the_same_result():
    f, v = ref.cached_case(182, 91, 3, 0.3, "uniform", _seed(182, 91, 3, 0.3, "uniform"))
    a = rvea_ops.select(_dev(f), _dev(v), 0.3, return_info=True)
    b = rvea_ops.select(_dev(f), _dev(v), torch.tensor(0.3, device="cuda"), return_info=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 6. safety
@pytest.mark.parametrize("bad", ["+inf row", "-inf row", "zero vector"])
def test_inputs_outside_the_promised_range_keep_the_outputs_in_bounds(bad):
    f, v = (a.copy() for a in ref.cached_case(182, 91, 3, 0.3, "uniform", 0))
    row = int(np.flatnonzero(~np.isnan(f).any(1))[5])
    if bad == "+inf row":
        f[row, 1] = np.inf
    elif bad == "-inf row":
        f[row, 1] = -np.inf
    else:
        v[7] = 0.0
    next_ind, empty = rvea_ops.select(_dev(f), _dev(v), THETA)
    next_ind = next_ind.cpu().numpy()  # it returned
    assert ((next_ind >= 0) & (next_ind < f.shape[0])).all()


# ---------------------------------------------------------------- 7. no (n, nv) temporary
def test_select_allocates_no_n_by_nv_array():
    n, nv, m = 8192, 4096, 3
    f, v = (_dev(a) for a in ref.cached_case(n, nv, m, 0.0, "uniform", 0))
    theta = torch.tensor(THETA, device="cuda")
    rvea_ops.select(f, v, theta)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = rvea_ops.select(f, v, theta)
    top = rvea_ops.cos_best(f, f, self_zero=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[rvea] peak memory over select and a truncation cos_best at ({n}, {v.shape[0]}, {m}): +{rise / 1e6:.2f} MB")
    assert rise < 8e6 and out[0].shape == (v.shape[0],) and top[0].shape == (n,)


# ---------------------------------------------------------------- 8. above the caps
def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(rvea_ops._ext, "ops", lambda: NoKernel())


def _torch_path_on_the_device(f, v):
    want = ref.select(f, v, THETA)
    next_ind, empty = rvea_ops.select(_dev(f), _dev(v), THETA)
    assert next_ind.is_cuda and next_ind.dtype == torch.int64 and np.array_equal(empty.cpu().numpy(), want["empty"])
    # the float32 path may settle a near-tie differently from the float64 reference: every kept row is a member of its vector
    kept = next_ind.cpu().numpy()[~want["empty"]]
    assert np.array_equal(want["arg"][kept], np.flatnonzero(~want["empty"]))
    best, arg = rvea_ops.cos_best(_dev(f), _dev(v))
    assert best.dtype == torch.float32 and arg.shape == (f.shape[0],)


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    m = rvea_ops.M_CAP + 1
    f, v = ref.objectives(120, m, 0.2, 3), ref.vectors(40, m, "rand", 3)
    _no_kernel(monkeypatch, "rvea_select", "rvea_cos_best")
    _torch_path_on_the_device(f, v)


def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    f, v = ref.objectives(rvea_ops.N_CAP + 8, 2, 0.2, 4), ref.vectors(10, 2, "uniform", 4)
    _no_kernel(monkeypatch, "rvea_select", "rvea_cos_best")
    _torch_path_on_the_device(f, v)


# ---------------------------------------------------------------- 9. generations
D_, M_, POP = 12, 3, 100
ALGOS = {"RVEA": lambda lb, ub, **kw: A.RVEA(lb, ub, M_, POP, **kw), "RVEAa": lambda lb, ub, **kw: A.RVEAa(lb, ub, M_, POP, **kw),
         "LMOCSO": lambda lb, ub, **kw: A.LMOCSO(M_, lb, ub, POP, **kw)}


def _run(name, graph, gens=6, seed=11, **kw):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(ALGOS[name](lb, ub, **kw), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


def _same(a, b):
    fa, fb = a.fitness, b.fitness
    assert torch.equal(torch.isnan(fa), torch.isnan(fb))
    fin = ~torch.isnan(fa)
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", list(ALGOS))
def test_generation_is_captured_and_matches_eager(name):
    _, a = _run(name, False)
    wf, b = _run(name, True)
    assert wf._graph is not None
    _same(a, b)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        wf, c = _run(name, "auto")
    assert not [w for w in caught if "not capturable" in str(w.message)]
    assert wf._graph is not None and not wf._graph_failed
    _same(a, c)


def test_rveaa_truncation_fires_inside_the_captured_graph():
    _, a = _run("RVEAa", False, gens=42, max_gen=40)
    wf, b = _run("RVEAa", True, gens=42, max_gen=40)
    assert wf._graph is not None and int(a.gen) == int(b.gen) >= 40
    _same(a, b)
    # the state right after the tell that truncates (gen = 39), against a run that never truncates
    _, cut = _run("RVEAa", True, gens=40, max_gen=40)
    _, never = _run("RVEAa", True, gens=40, max_gen=1000)
    assert int(cut.gen) == int(never.gen) == 39
    valid = lambda s: int((~torch.isnan(s.fitness).any(1)).sum())
    print(f"[rvea] RVEA* valid rows after the tell with gen = 39: {valid(cut)} truncated, {valid(never)} with max_gen = 1000")
    assert not torch.equal(torch.isnan(cut.fitness), torch.isnan(never.fitness))


@pytest.mark.parametrize("name", list(ALGOS))
def test_ask_and_tell_read_nothing_on_the_host(name, monkeypatch):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = ALGOS[name](lb, ub)
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
        for attr in ("item", "tolist", "cpu", "numpy", "__int__", "__bool__", "__float__", "__index__"):
            mp.setattr(torch.Tensor, attr, forbidden)
        _, b = algo.ask(a)
        b = algo.tell(b, fit)
    torch.cuda.synchronize()
    assert b.fitness.shape[1] == M_ and int(b.gen) == int(a.gen) + 1 and not torch.isnan(b.fitness).all()


@pytest.mark.parametrize("name", list(ALGOS))
def test_converges_on_dtlz2_on_the_device(name):
    _, a = _run(name, True, gens=100, seed=42)
    fit = a.fitness[~torch.isnan(a.fitness).any(1)]
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] {name}, DTLZ2 d 12 m 3, N 100, 100 captured generations: {igd:.4f} on {fit.shape[0]} rows")
    assert igd < 0.1
