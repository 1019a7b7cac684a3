"""``m2m_select.hip`` against the CPU torch path, and MOEA/D-M2M generations captured into a hipGraph (MI355X,
marked gpu).  Every kernel case is exact equality of ``part``, ``counts`` and ``worst`` with ``ops.m2m.select`` on
CPU tensors of the same float32 input (``test_m2m_select.py`` pins that path to an independent numpy reference and to
the loop ``associate`` ran before).  Dominance is comparisons only, the crowding arithmetic is the same float32
operations in the same order and every sort is stable, so there is no tolerance anywhere.

Inputs (``_m2m_reference.case``): ``uniform`` is rand in [0, 1]^m, ``front`` is |normal| + 1e-3 normalised to the
unit sphere (every row non-dominated: crowding decides everything); the region of a row is the nearest of K seeded
random directions, which gives regions on both sides of S.  The two ``uniform`` n = 8192 oracles take 5 to 7 s each on the host
(the torch path peels every front of an (n, n) dominance matrix) and are built once per session (``cached_oracle``).

Observed on an MI355X (gfx950): every case equal; region sizes 176..1577 at (8192, 3, 16, 256) with cut ranks up to 22,
17 fronts before the cut at (8192, 3, 1, 4096) uniform; IGD after 100 captured generations 0.1437."""
import warnings

import numpy as np
import pytest
import torch

import _m2m_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import m2m as m2m_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(obj, region, rad, K, S):
    part, counts, worst = m2m_ops.select(_dev(obj), _dev(region), _dev(rad), K, S, return_info=True)
    assert part.is_cuda and part.dtype == torch.int64 and part.shape == (K * S,)
    assert counts.dtype == torch.int32 and counts.shape == (K,) and worst.dtype == torch.int32 and worst.shape == (K,)
    return part.cpu().numpy(), counts.cpu().numpy(), worst.cpu().numpy()


def _check(obj, region, rad, K, S, want=None):
    want = ref.oracle(obj, region, rad, K, S) if want is None else want
    got = _kernel(obj, region, rad, K, S)
    for name, g, w in zip(("counts", "worst", "part"), (got[1], got[2], got[0]), (want[1], want[2], want[0])):
        assert np.array_equal(g, w), f"{name} differs from the CPU path at {np.flatnonzero(g != w)[:8]}"
    return got


# ---------------------------------------------------------------- 1. sizes
SIZES = [(20, 3, 10, 1, "uniform"), (65, 2, 10, 3, "uniform"), (200, 3, 10, 10, "uniform"), (200, 3, 10, 10, "front"),
         (257, 5, 10, 12, "uniform"), (257, 16, 8, 16, "uniform"), (1000, 3, 10, 50, "uniform"),
         (2050, 3, 1, 1025, "uniform"), (2050, 3, 1, 1025, "front"),  # the cut front crosses 1024 and 2048: IT = 2 and 4
         (8192, 3, 1, 4096, "uniform"), (8192, 3, 1, 4096, "front"),  # the caps, one region, IT = 8
         (8192, 3, 16, 256, "uniform")]


@pytest.mark.parametrize("n,m,K,S,kind", SIZES)
def test_kernel_equals_the_cpu_path(n, m, K, S, kind):
    obj, region, rad = ref.cached_case(n, m, K, S, kind)
    part, counts, worst = _check(obj, region, rad, K, S, ref.cached_oracle(n, m, K, S, kind))
    print(f"[m2m] ({n}, {m}, {K}, {S}) {kind}: region sizes {counts.min()}..{counts.max()}, cut ranks up to {worst.max()}")
    again = _kernel(obj, region, rad, K, S)  # determinism
    assert all(np.array_equal(a, b) for a, b in zip(again, (part, counts, worst)))


def test_int32_regions_give_the_same_result():
    n, m, K, S, kind = 1000, 3, 10, 50, "uniform"
    obj, region, rad = ref.cached_case(n, m, K, S, kind)
    _check(obj, region.astype(np.int32), rad, K, S, ref.cached_oracle(n, m, K, S, kind))


# ---------------------------------------------------------------- 2. edges
def test_an_empty_region_is_filled_from_rad():
    obj, region, rad = ref.case(100, 3, 4, 8, "uniform", 5)
    region = np.where(region == 2, 3, region)
    part, counts, worst = _check(obj, region, rad, 4, 8)
    assert counts[2] == 0 and worst[2] == -1 and np.array_equal(part[16:24], rad)


def test_a_region_of_exactly_s_members_takes_the_selection_branch():
    obj = ref.objectives(64, 3, "uniform", 9)
    region = np.where(np.arange(64) < 12, 0, 1).astype(np.int64)
    rad = np.arange(12, dtype=np.int64)
    part, counts, worst = _check(obj, region, rad, 2, 12)
    assert counts[0] == 12 and worst[0] >= 0
    assert sorted(part[:12].tolist()) == list(range(12)) and part[:12].tolist() != list(range(12))  # (rank, −cd, row)


def test_a_dominance_chain_needs_one_front_per_member():
    c, S = 300, 150
    obj = np.stack([np.arange(c), np.arange(c) * 2.0, np.arange(c) + 5.0], 1).astype(np.float32)  # row i dominates row i + 1
    part, counts, worst = _check(obj, np.zeros(c, dtype=np.int64), np.zeros(S, dtype=np.int64), 1, S)
    assert worst[0] == S - 1 and part.tolist() == list(range(S))


def test_all_rows_equal():
    n, S = 40, 10
    obj = np.full((n, 3), 0.25, dtype=np.float32)
    part, counts, worst = _check(obj, np.zeros(n, dtype=np.int64), np.zeros(S, dtype=np.int64), 1, S)
    # one front; the extremes of the stable sort (rows 0 and n − 1) get inf, the interior 0/0 = NaN, and NaN sorts last
    assert worst[0] == 0 and part.tolist() == [0, n - 1] + list(range(1, S - 1))


def test_three_equal_rows_keep_the_first_and_the_third():
    obj = np.full((3, 2), 1.0, dtype=np.float32)
    part, _, _ = _check(obj, np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int64), 1, 2)
    assert part.tolist() == [0, 2]


def test_a_block_of_duplicates_inside_a_front():
    n, S = 400, 200
    obj = ref.objectives(n, 3, "front", 6).copy()
    obj[100:150] = obj[5]  # what M2M's own padding produces
    part, _, worst = _check(obj, np.zeros(n, dtype=np.int64), np.zeros(S, dtype=np.int64), 1, S)
    assert worst[0] == 0


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_a_non_finite_objective_is_safe(bad):
    n, K, S = 300, 4, 40
    obj, region, rad = ref.case(n, 3, K, S, "uniform", 3)
    obj = obj.copy()
    obj[np.flatnonzero(region == np.bincount(region, minlength=K).argmax())[7], 1] = bad  # in the largest region
    part, counts, worst = _kernel(obj, region, rad, K, S)  # it returned: it terminates
    assert np.array_equal(counts, np.bincount(region, minlength=K)) and (counts > S).any()
    assert ((part >= 0) & (part < n)).all()
    for k in range(K):
        head = part[k * S:k * S + min(int(counts[k]), S)]
        assert len(set(head.tolist())) == head.size and (region[head] == k).all()


# ---------------------------------------------------------------- 3. above the caps
def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(m2m_ops._ext, "ops", lambda: NoKernel())


def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    # m = 2: the device torch path adds the two crowding terms in either order with the same result, so it is exact too
    n, m, K, S = m2m_ops.N_CAP + 8, 2, 16, 8
    obj, region, rad = ref.case(n, m, K, S, "front", 2)
    want = ref.oracle(obj, region, rad, K, S)[0]
    _no_kernel(monkeypatch, "m2m_select")
    part = m2m_ops.select(_dev(obj), _dev(region), _dev(rad), K, S)
    assert part.is_cuda and np.array_equal(part.cpu().numpy(), want)


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    n, m, K, S = 120, m2m_ops.M_CAP + 1, 4, 10
    obj, region, rad = ref.case(n, m, K, S, "uniform", 4)
    want = ref.oracle(obj, region, rad, K, S)[0]
    _no_kernel(monkeypatch, "m2m_select")
    part = m2m_ops.select(_dev(obj), _dev(region), _dev(rad), K, S)
    assert part.is_cuda and np.array_equal(part.cpu().numpy(), want)


# ---------------------------------------------------------------- 4. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=6, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.MOEADM2M(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


def _same(a, b):
    fa, fb = a.fitness, b.fitness
    fin = torch.isfinite(fa)
    assert torch.equal(fin, torch.isfinite(fb))
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)


def test_generation_is_captured_and_matches_eager():
    _, a = _run(False)
    wf, b = _run(True)
    assert wf._graph is not None
    _same(a, b)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        wf, c = _run("auto")
    assert not [w for w in caught if "not capturable" in str(w.message)]
    assert wf._graph is not None and not wf._graph_failed
    _same(a, c)


def test_ask_and_tell_read_nothing_on_the_host(monkeypatch):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.MOEADM2M(lb, ub, M_, POP)
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
        b = algo.init_tell(a, fit)
        _, b = algo.ask(b)
        b = algo.tell(b, fit)
    torch.cuda.synchronize()
    assert b.fitness.shape == (algo.pop_size, M_) and torch.isfinite(b.fitness).all() and int(b.gen) == int(a.gen) + 1


def test_moeadm2m_converges_on_dtlz2_on_the_device():
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] MOEADM2M, DTLZ2 d 12 m 3, N 100, 100 generations: {igd:.4f}")
    assert igd < 0.2
