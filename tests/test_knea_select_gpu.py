"""``knea_select.hip`` against the numpy reference of ``_knea_reference.py``, and KnEA generations captured into a
hipGraph (MI355X, marked gpu).  The kernel and the reference perform the same float64 operations in the same order (the
kernel is compiled without FMA contraction), so ``idx``, ``knee`` and ``t`` are compared exactly and ``r``, where the
two ``exp`` may differ by an ulp per front, to 1e-12 relative.  Every fixture is asserted to qualify (a ≥ 1e-12,
b ≥ 1e-9, c ≤ 1e8, see the reference), so that an ulp in r cannot turn a box comparison.

Inputs (``_knea_reference.case``): ``uniform`` is rand in [0, 1]^m, ``front`` is |normal| + 1e-3 normalised to the unit
sphere, both scaled by ``1 + 0.25·rank`` with ``rank`` a sorted random layer index; N = n // 2.  The start values are
(r, t) = (1, 0) and (0.3, 0.6), which leave few knees per front, and (0.02, 0.5), which keeps r at 0.02 in the first
front and makes most rows knees: the long scans.

Observed on an MI355X (gfx950): every case equal (r within 1e-12); 1649 knees in the
one front of (8192, 3, 1) and 2076 + 2034 in the two of (8192, 5, 4) at the start (0.02, 0.5); ten captured generations
equal ten eager ones; IGD after 100 captured generations 0.0612."""
import warnings

import numpy as np
import pytest
import torch

import _knea_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import knea as knea_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu

KNEE_RATE = 0.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _word(v):
    return torch.tensor(float(v), dtype=torch.float64, device="cuda")


def _kernel(obj, rank, N, r, t):
    n = obj.shape[0]
    r_in, t_in = _word(r), _word(t)
    idx, knee, r_out, t_out = knea_ops.select(_dev(obj), _dev(rank), N, r_in, t_in, KNEE_RATE)
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.shape == (N,)
    assert knee.dtype == torch.bool and knee.shape == (n,)
    assert r_out.dtype == torch.float64 and r_out.dim() == 0 and r_out.is_cuda and t_out.dtype == torch.float64 and t_out.dim() == 0
    assert float(r_in) == float(r) and float(t_in) == float(t)  # the inputs are left as they are
    return idx.cpu().numpy(), knee.cpu().numpy(), float(r_out), float(t_out)


def _check(obj, rank, N, r, t, want=None):
    idx, knee, r1, t1, q = ref.select(obj, rank, N, r, t, KNEE_RATE) if want is None else want
    assert ref.qualifies(q), f"the fixture no longer qualifies: a {q['a']:.1e} b {q['b']:.1e} c {q['c']:.1e}"
    got = _kernel(obj, rank, N, r, t)
    assert np.array_equal(got[1], knee), f"knee differs from the reference at {np.flatnonzero(got[1] != knee)[:8]}"
    assert np.array_equal(got[0], idx), f"idx differs from the reference at {np.flatnonzero(got[0] != idx)[:8]}"
    assert got[3] == t1 and abs(got[2] - r1) <= 1e-12 * r1, f"(r, t) = ({got[2]!r}, {got[3]!r}), the reference has ({r1!r}, {t1!r})"
    return got, q


# ---------------------------------------------------------------- 1. sizes
# (n, m, layers, kind, seed); the seeds are those at which the fixture qualifies for all three starts
SIZES = [(2, 2, 1, "uniform", 1), (20, 3, 3, "uniform", 0), (65, 2, 4, "front", 1), (200, 3, 6, "uniform", 0), (257, 5, 3, "front", 0),
         (257, 16, 2, "uniform", 0), (257, 16, 2, "uniform", 1),  # the fallback planes (one row holds two column maxima)
         (2050, 3, 1, "front", 0), (2050, 3, 5, "uniform", 0),  # fronts that cross 1024 and 2048: IT = 1, 2 and 4
         (8192, 3, 1, "front", 1), (8192, 3, 12, "front", 0), (8192, 5, 4, "uniform", 0)]  # the cap: IT = 8, and m > 4
STARTS = [(1.0, 0.0), (0.3, 0.6), (0.02, 0.5)]


@pytest.mark.parametrize("r,t", STARTS)
@pytest.mark.parametrize("n,m,layers,kind,seed", SIZES)
def test_kernel_equals_the_reference(n, m, layers, kind, seed, r, t):
    obj, rank = ref.cached_case(n, m, layers, kind, seed)
    N = max(n // 2, 1)
    got, q = _check(obj, rank, N, r, t, ref.cached_select(n, m, layers, kind, seed, N, r, t, KNEE_RATE))
    print(f"[knea] ({n}, {m}, {layers}) {kind} start ({r}, {t}): a {q['a']:.1e} b {q['b']:.1e} c {q['c']:.1f} dif {q['dif']} "
          f"fallbacks {q['fallbacks']} (front, knees) {q['knees'][:4]}")
    again = _kernel(obj, rank, N, r, t)  # a second call returns identical results
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2:] == got[2:]


def test_the_sizes_meet_fallback_planes_and_both_signs_of_dif():
    quals = [ref.cached_select(n, m, layers, kind, seed, max(n // 2, 1), r, t, KNEE_RATE)[4] for n, m, layers, kind, seed in SIZES[:7]
             for r, t in STARTS]
    assert {q["dif"] for q in quals} >= {-1, 1} and any(q["fallbacks"] for q in quals) and any(q["c"] > 0 for q in quals)


def test_int32_ranks_give_the_same_result():
    n, m, layers, kind, seed = 200, 3, 6, "uniform", 0
    obj, rank = ref.cached_case(n, m, layers, kind, seed)
    _check(obj, rank.astype(np.int32), n // 2, 0.3, 0.6, ref.cached_select(n, m, layers, kind, seed, n // 2, 0.3, 0.6, KNEE_RATE))


# ---------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    obj, rank, N, r, t = ref.hand_cases()[name]
    _check(obj, np.asarray(rank, dtype=np.int64), N, r, t)


def test_a_dominance_chain_has_one_row_per_front():
    N = 50
    n = N + 1  # N + 1 fronts of one row: every one a knee with a fallback plane, the cut front holds position N alone
    obj = np.stack([np.arange(n) + 1.0, np.arange(n) * 2.0 + 1.0, np.arange(n) + 5.0], 1).astype(np.float32)
    rank = np.arange(n, dtype=np.int64)
    (idx, knee, r, t), q = _check(obj, rank, N, 1.0, 0.0)
    assert q["fallbacks"] == n and knee.all() and idx.tolist() == list(range(N)) and t == 1.0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_objectives_are_safe(bad):
    n, m, layers = 300, 3, 3
    obj, rank = ref.case(n, m, layers, "uniform", 3)
    obj = obj.copy()
    obj[5, 1] = bad
    obj[150] = bad
    obj[290, 0] = bad
    for N in (40, 150, 299):
        idx, knee, r, t = _kernel(obj, rank, N, 0.3, 0.6)  # it returned: it terminates
        assert ((idx >= 0) & (idx < n)).all() and len(set(idx.tolist())) == N


# ---------------------------------------------------------------- 3. above the caps
def _no_kernel(monkeypatch):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name != "knea_select", "the kernel was called where the host path is due"
            return getattr(ops, name)

    monkeypatch.setattr(knea_ops._ext, "ops", lambda: NoKernel())


def test_over_the_row_cap_runs_the_host_path(monkeypatch):
    """n = 8200 rows, of which the two fronts up to the cut hold 140 (so the host loop, which reads the device once per
    member, stays short).  The host path evaluates the keys in float32, so the fixture must also clear float32's reach
    (b and the key gap ≥ 1e-5) and must not depend on the order of tied keys."""
    n, m, N = knea_ops.N_CAP + 8, 3, 100
    obj = ref.objectives(n, m, "front", 3)
    rank = np.repeat(np.arange(3), [60, 80, n - 140]).astype(np.int64)
    obj = np.ascontiguousarray(obj * (1 + 0.25 * rank[:, None]).astype(np.float32), dtype=np.float32)
    idx, knee, r1, t1, q = ref.select(obj, rank, N, 1.0, 0.0, KNEE_RATE)
    assert ref.qualifies(q, b=1e-5) and q["gap"] >= 1e-5, "the fixture no longer qualifies"
    other = ref.select(obj, rank, N, 1.0, 0.0, KNEE_RATE, ties="descending")
    assert np.array_equal(other[0], idx) and np.array_equal(other[1], knee), "the fixture depends on the order of tied keys"
    _no_kernel(monkeypatch)
    got = knea_ops.select(_dev(obj), _dev(rank), N, _word(1.0), _word(0.0), KNEE_RATE)
    assert got[0].is_cuda and got[2].dtype == torch.float64 and got[2].is_cuda and got[2].dim() == 0
    assert np.array_equal(got[0].cpu().numpy(), idx) and np.array_equal(got[1].cpu().numpy(), knee)
    assert abs(float(got[2]) - r1) <= 1e-6 * r1 and float(got[3]) == t1


def test_over_the_objective_cap_runs_the_host_path(monkeypatch):
    n, m, N = 60, knea_ops.M_CAP + 1, 30
    obj, rank = ref.case(n, m, 2, "uniform", 4)
    _no_kernel(monkeypatch)
    idx, knee, r, t = knea_ops.select(_dev(obj), _dev(rank), N, _word(1.0), _word(0.0), KNEE_RATE)
    assert idx.is_cuda and idx.shape == (N,) and len(set(idx.tolist())) == N and r.is_cuda


# ---------------------------------------------------------------- 4. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=10, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.KnEA(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens + 1):  # the first step evaluates the initial population
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


def _same(a, b):
    fa, fb = a.fitness, b.fitness
    fin = torch.isfinite(fa)
    assert torch.equal(fin, torch.isfinite(fb))
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)
    assert torch.equal(a.knee, b.knee) and float(a.r) == float(b.r) and float(a.t) == float(b.t)


def test_ten_captured_generations_equal_ten_eager_ones():
    _, a = _run(False)
    assert a.r.dtype == torch.float64 and a.r.is_cuda and a.r.dim() == 0 and a.t.dtype == torch.float64 and a.t.is_cuda
    wf, b = _run(True)
    assert wf._graph is not None
    _same(a, b)


def test_graph_auto_captures():
    _, a = _run(False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        wf, c = _run("auto")
    assert not [w for w in caught if "not capturable" in str(w.message)]
    assert wf._graph is not None and not wf._graph_failed
    _same(a, c)


def test_tell_reads_nothing_on_the_host(monkeypatch):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.KnEA(lb, ub, M_, POP)
    wf = StdWorkflow(algo, DTLZ2(d=D_, m=M_), graph=False)
    st = wf.init(rnd.PRNGKey(3, device="cuda"))
    for _ in range(3):
        st = wf.step(st)
    a = st.get_child_state("algorithm")
    fit = torch.rand(POP, M_, device="cuda")
    torch.cuda.synchronize()

    def forbidden(*args, **kwargs):
        raise AssertionError("host read in tell")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        for name in ("item", "tolist", "__bool__", "__int__", "__float__"):
            mp.setattr(torch.Tensor, name, forbidden)
        b = algo.tell(a, fit)
    torch.cuda.synchronize()
    assert b.fitness.shape == (POP, M_) and torch.isfinite(b.fitness).all() and b.knee.shape == (POP,)
    assert 0.0 < float(b.t) <= 1.0 and float(b.r) > 0.0


def test_knea_converges_on_dtlz2_on_the_device():
    """IGD after 100 captured generations at N = 100 on DTLZ2 (m = 3, d = 12) against the project's bound of 0.1
    (0.061 on the CPU path).  Measured on an MI355X: 0.0612."""
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] KnEA, DTLZ2 d 12 m 3, N 100, 100 captured generations: {igd:.4f}")
    assert igd < 0.1
