"""``spea2_select.hip`` against host references, and SPEA2 generations captured into a hipGraph (MI355X,
marked gpu).  The references are numpy, float64 or int64, on the same float32 objectives
(``_spea2_reference.py``; ``test_spea2_select.py`` pins them to each other and to the torch path).

Inputs: ``uniform`` is rand in [0, 1]^m, ``front`` is |normal| + 1e-3 normalised to the unit sphere (every row
non-dominated, so the mask is everything).  ``uniform`` at m = 3 leaves only 10–25 non-dominated rows of 257,
so the truncation tests on ``uniform`` pass an all-true mask.  Truncation tests keep half of the masked rows.

Fitness, exact parts.  ``S`` (the rows a row dominates), ``nd`` (no row dominates it) and ``R`` (the sum of
its dominators' strengths) equal the int64 reference exactly, R as ``float32(exact sum)``: the kernel sums in
32-bit integers and converts once.  On a chain of 8192 totally ordered rows R reaches n²/2 > 2²⁴, where a
float32 running sum is wrong.

Fitness, D = 1 / (sqrt(second smallest d2) + 2).  With u = 2⁻²⁴: each difference δ_k is rounded once (1 + u),
its square inside the fmaf is exact, and each of the m fmaf rounds once; all terms are positive, so
d2 is within (m + 2)·u relative.  The square root halves that and adds u, the + 2 adds at most u, the
division u: D is within ((m + 2)/2 + 3)·u = (m + 8)·2⁻²⁵.  The second-smallest order statistic is monotone in
its arguments, so the bound on every d2 carries to it even where float32 picks another neighbour.  The test
asserts (m + 6)·2⁻²³, the bound the kernel was specified with: 4·(m + 6)/(m + 8) ≥ 2.9 times this derivation.

Truncation, exact.  Where the float64 reference has, at every step with three live rows or more, exactly two
rows at the minimum nearest-neighbour d2 and a relative gap of at least 1e-5 to the next larger value (about
4× the two-sided float32 error 2(m + 2)·2⁻²⁴ at m = 5), the kernel's order equals the reference's: the lower
row of the exactly tied closest pair leaves.  The gap is asserted on the reference, so an input that stops
qualifying fails.

Truncation, certificate: every other input.  The kernel's own order is replayed in float64; at each step the
removed row's float64 nearest-neighbour d2 is at most (1 + 4(m + 2)·2⁻²⁴) times the float64 minimum over the
live masked rows.

Ties: equal rows leave in index order and a removal among them rescans nothing (asserted: rescans ≤ removals).
Non-finite: a NaN row is outside the mask and stays; a masked row with an infinite objective has +inf
distances and exactly k rows still leave, the lowest index first where every distance is +inf.

Observed on an MI355X (gfx950), worst over the cases of each test:

==============================  ==============================================================
quantity                        worst observed
==============================  ==============================================================
S, nd, R                        equal in every case; the chain's R peaks at 33 550 336 > 2²⁴
D, relative error               2.01·2⁻²⁴ at (257, 16) uniform (bound 44·2⁻²⁴); 1.65·2⁻²⁴ at
                                (1000, 10), 1.46–1.50·2⁻²⁴ at m = 3, 1.26·2⁻²⁴ at m = 2
D, e_k / e_t (record only)      0.51 at most ((257, 16) front); the CPU float32 ``cal_fitness`` is
                                up to 4.6e-2 relative off at (2049, 3) uniform (cdist's
                                matrix-product form cancels for close neighbours)
exact order, smallest gap       1.35e-5 ((1025, 3) front seed 3), 1.40e-5 ((513, 5) seed 2),
                                1.52e-5 ((200, 3) seed 0); the orders are equal in all 14 cases
certificate, ratio − 1          2.1e-8 ((4097, 5) uniform) and 1.5e-8 ((8192, 3) front) against
                                bounds of 1.7e-6 and 1.2e-6; exactly 0 in every other case
rescans per removal             1.51–1.72 at m ≤ 3, 1.75–1.86 at m = 5, 2.0–2.1 at m = 10
all rows equal, n = 2049        0 rescans for 1049 removals; duplicate block: 0 for 49
IGD after 100 generations       0.0576 (the CPU run measures .058)
==============================  ==============================================================
"""
import functools

import numpy as np
import pytest
import torch

import _spea2_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import spea2 as spea2_ops
from evoxmi.problems.numerical import DTLZ2
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu

U = 2.0**-24


def _dev(a):
    return torch.tensor(a).cuda()


def _no_kernel(monkeypatch, *banned):
    ops = _ext.ops()

    class NoKernel:
        def __getattr__(self, name):
            assert name not in banned, "the kernel was called where the torch path is due"
            return getattr(ops, name)

    monkeypatch.setattr(spea2_ops._ext, "ops", lambda: NoKernel())


# ---------------------------------------------------------------- 1. fitness
@functools.lru_cache(maxsize=None)
def _fitness_reference(n, m, kind):
    obj = ref.cached_objectives(n, m, kind, 100 * n + m)
    return obj, ref.fitness_parts(obj)


SHAPES = [(2, 2), (3, 1), (65, 2), (255, 3), (257, 16), (1000, 10), (2049, 3), (8192, 3)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_fitness_parts_are_exact_and_D_within_its_bound(n, m, kind):
    obj, (S64, nd64, R64, D64) = _fitness_reference(n, m, kind)
    sig, S, R, D, nd = spea2_ops.fitness(_dev(obj), return_parts=True)
    assert sig.is_cuda and sig.dtype == torch.float32 and sig.shape == (n,)
    assert S.dtype == torch.int32 and nd.dtype == torch.bool and R.dtype == torch.float32 and D.dtype == torch.float32
    assert np.array_equal(S.cpu().numpy(), S64)
    assert np.array_equal(nd.cpu().numpy(), nd64)
    assert np.array_equal(R.cpu().numpy(), R64.astype(np.float32))
    if kind == "front" and m > 1:
        assert nd64.all()
    rel = lambda d: float(np.max(np.abs(d - D64) / np.where(D64 > 0, D64, 1.0)))  # D64 = 0 only for n = 2 (no second neighbour)
    e_k = rel(D.cpu().numpy().astype(np.float64))
    line = f"[D] ({n}, {m}) {kind}: rel e_k {e_k:.3e} = {e_k / U:.2f}·2^-24, bound {(m + 6) * 2 * U:.3e}"
    if n <= 2049:  # for the record: the float32 torch evaluation on the CPU (cdist's form)
        t = spea2_ops.cal_fitness(torch.tensor(obj)).numpy().astype(np.float64) - R64
        e_t = rel(t)
        line += f", torch e_t {e_t:.3e}, e_k/e_t {e_k / e_t if e_t > 0 else float('inf'):.3f}"
    print(line)
    assert e_k <= (m + 6) * 2.0**-23, line
    assert torch.equal(sig, D + R) and torch.equal(sig < 1, nd)
    again = spea2_ops.fitness(_dev(obj))
    assert torch.equal(again.view(torch.int32), sig.view(torch.int32))


def test_raw_fitness_is_an_integer_sum_above_2_to_24():
    n = 8192
    obj = np.repeat((np.arange(n, dtype=np.float32) / n)[:, None], 3, axis=1)  # row i dominates every row after it
    S64 = n - 1 - np.arange(n, dtype=np.int64)
    R64 = np.concatenate([[0], np.cumsum(S64)[:-1]])
    assert R64.max() > 2**24 and R64.max() < 2**31
    _, S, R, _, nd = spea2_ops.fitness(_dev(obj), return_parts=True)
    assert np.array_equal(S.cpu().numpy(), S64)
    assert np.array_equal(R.cpu().numpy(), R64.astype(np.float32))
    assert np.array_equal(nd.cpu().numpy(), np.arange(n) == 0)


def test_duplicate_rows_get_bit_equal_fitness():
    o = ref.objectives(300, 3, "uniform", 4)
    obj = np.concatenate([o, o[::-1]])
    sig = spea2_ops.fitness(_dev(obj)).cpu()
    assert torch.equal(sig[:300].view(torch.int32), sig[300:].flip(0).view(torch.int32))


# ---------------------------------------------------------------- 2. truncation, exact
def _truncate(obj, mask, n_keep):
    n = obj.shape[0]
    keep, order, n_rescans = spea2_ops.truncate(_dev(obj), _dev(mask), n_keep, return_order=True)
    assert keep.is_cuda and keep.dtype == torch.bool and keep.shape == (n,) and order.dtype == torch.int64
    assert order.shape == (max(n - n_keep, 0),) and n_rescans.dtype == torch.int32
    k = max(0, int(mask.sum()) - n_keep)
    keep, order = keep.cpu().numpy(), order.cpu().numpy()
    assert (order[k:] == -1).all() and (order[:k] >= 0).all() and (order[:k] < n).all()
    expect = mask.copy()
    expect[order[:k]] = False
    assert np.array_equal(keep, expect) and int(keep.sum()) == int(mask.sum()) - k, "keep is not the mask without the removed rows"
    return order[:k], int(n_rescans)


EXACT = [(64, 2, "front", 0), (64, 2, "front", 1), (64, 2, "front", 2), (200, 3, "front", 0), (200, 3, "front", 1),
         (200, 3, "front", 2), (257, 3, "uniform", 0), (257, 3, "uniform", 1), (257, 3, "uniform", 2), (513, 5, "front", 2),
         (513, 5, "front", 3), (1025, 3, "front", 1), (1025, 3, "front", 3), (1025, 3, "front", 4)]


@pytest.mark.parametrize("n,m,kind,seed", EXACT)
def test_truncation_matches_the_float64_order(n, m, kind, seed):
    obj = ref.objectives(n, m, kind, seed)
    mask = np.ones(n, dtype=bool)
    n_keep = n // 2
    want, gap, pairs, ref_rescans = ref.incremental_truncation(obj, mask, n - n_keep)
    print(f"[exact] ({n}, {m}) {kind} seed {seed}: gap {gap:.3e}, reference rescans {ref_rescans}")
    assert pairs and gap >= 1e-5, f"the input no longer qualifies: pairs {pairs}, gap {gap:.3e}"
    order, n_rescans = _truncate(obj, mask, n_keep)
    assert np.array_equal(order, want)
    print(f"[exact] ({n}, {m}) {kind} seed {seed}: kernel rescans {n_rescans} for {n - n_keep} removals")


# ---------------------------------------------------------------- 3. truncation, certificate
def _certificate(what, obj, mask, order, n_rescans):
    m = obj.shape[1]
    worst = ref.replay_slack(obj, mask, order)
    bound = 1.0 + 4 * (m + 2) * U
    print(f"[certificate] {what}: worst ratio − 1 = {worst - 1.0:.3e} (bound {bound - 1.0:.3e}), rescans / removal "
          f"{n_rescans / max(len(order), 1):.3f}")
    assert worst <= bound, f"{what}: ratio − 1 = {worst - 1.0:.3e} > {bound - 1.0:.3e}"


ALL_SIZES = [(1000, 10), (2049, 3), (4097, 5), (8191, 2), (8192, 3)]
# both sides of every step in rows per thread and in threads of the truncation kernel
STEPS = [(256, 3), (257, 3), (512, 3), (513, 3), (1024, 3), (1025, 3), (2048, 3), (4096, 3), (4097, 3)]


@pytest.mark.parametrize("kind", ["uniform", "front"])
@pytest.mark.parametrize("n,m", ALL_SIZES + STEPS)
def test_truncation_certificate(n, m, kind):
    obj = ref.objectives(n, m, kind, 100 * n + m)
    mask = np.ones(n, dtype=bool)
    order, n_rescans = _truncate(obj, mask, n // 2)
    assert len(order) == n - n // 2 and len(set(order.tolist())) == len(order)
    _certificate(f"({n}, {m}) {kind}", obj, mask, order, n_rescans)


def test_truncation_of_the_non_dominated_set_of_a_uniform_population():
    """The mask the algorithm uses: sig < 1 of a uniform population (1000, 10), most of it non-dominated."""
    obj = ref.objectives(1000, 10, "uniform", 1)
    sig = spea2_ops.fitness(_dev(obj))
    mask = (sig < 1).cpu().numpy()
    count = int(mask.sum())
    assert 200 < count < 1000
    order, n_rescans = _truncate(obj, mask, count // 2)
    _certificate("(1000, 10) uniform, non-dominated set", obj, mask, order, n_rescans)


# ---------------------------------------------------------------- 4. ties and structure
def test_equal_rows_leave_in_index_order_without_rescans():
    n, n_keep = 2049, 1000
    obj = np.full((n, 3), 0.25, dtype=np.float32)
    order, n_rescans = _truncate(obj, np.ones(n, dtype=bool), n_keep)
    assert np.array_equal(order, np.arange(n - n_keep))
    print(f"[ties] all equal n {n}: rescans {n_rescans} for {n - n_keep} removals")
    assert n_rescans <= n - n_keep


def test_a_block_of_duplicates_inside_a_front():
    n = 400
    obj = ref.objectives(n, 3, "front", 6).copy()
    obj[100:150] = obj[5]  # 51 equal rows: 5 and 100 … 149
    mask = np.ones(n, dtype=bool)
    order, n_rescans = _truncate(obj, mask, n - 49)
    assert order.tolist() == [5] + list(range(100, 148))
    print(f"[ties] duplicate block: rescans {n_rescans} for 49 removals")
    assert n_rescans <= 49
    order, n_rescans = _truncate(obj, mask, n // 2)  # past the block: all but one of the equal rows go first
    assert order[:50].tolist() == [5] + list(range(100, 149))
    _certificate("duplicate block in (400, 3) front", obj, mask, order, n_rescans)


def test_keeping_one_row_and_removing_one_row():
    n, m = 130, 3
    obj = ref.objectives(n, m, "front", 2)
    mask = np.ones(n, dtype=bool)
    want, gap, pairs, _ = ref.incremental_truncation(obj, mask, 1)
    assert pairs and gap >= 1e-5
    order, _ = _truncate(obj, mask, n - 1)
    assert np.array_equal(order, want)
    order, n_rescans = _truncate(obj, mask, 1)
    assert len(order) == n - 1
    _certificate(f"({n}, {m}) front n_keep 1", obj, mask, order, n_rescans)


def test_nothing_leaves_when_the_mask_is_small_and_select_sorts_by_fitness():
    n, n_keep = 257, 100
    obj = ref.objectives(n, 3, "uniform", 8)
    d = _dev(obj)
    sig = spea2_ops.fitness(d)
    mask = (sig < 1).cpu().numpy()
    assert 0 < int(mask.sum()) <= n_keep
    order, n_rescans = _truncate(obj, mask, n_keep)
    assert len(order) == 0 and n_rescans == 0
    idx = spea2_ops.select(d, n_keep)
    assert idx.is_cuda and idx.dtype == torch.int64 and torch.equal(idx, torch.argsort(sig, stable=True)[:n_keep])


def test_select_is_the_truncation_of_the_non_dominated_set():
    n, n_keep = 513, 200
    obj = ref.objectives(n, 3, "front", 3)
    d = _dev(obj)
    keep = spea2_ops.truncate(d, spea2_ops.fitness(d) < 1, n_keep)
    idx = spea2_ops.select(d, n_keep)
    assert int(keep.sum()) == n_keep and torch.equal(idx, torch.nonzero(keep).flatten())
    assert torch.equal(spea2_ops.select(d, n_keep), idx)


# ---------------------------------------------------------------- 5. non-finite objectives
def test_a_nan_row_is_outside_the_mask_and_is_never_removed():
    n, n_keep = 200, 80
    obj = ref.objectives(n, 3, "front", 5).copy()
    obj[17, 1] = np.nan
    d = _dev(obj)
    sig, S, R, D, nd = spea2_ops.fitness(d, return_parts=True)
    assert bool(torch.isnan(sig[17])) and int(torch.isnan(sig).sum()) == 1
    mask = (sig < 1).cpu().numpy()
    assert not mask[17] and int(mask.sum()) == n - 1
    order, _ = _truncate(obj, mask, n_keep)
    assert len(order) == n - 1 - n_keep and 17 not in order.tolist()
    idx = spea2_ops.select(d, n_keep).cpu().numpy()
    assert 17 not in idx.tolist() and len(set(idx.tolist())) == n_keep and mask[idx].all()
    # given in the mask all the same, its distances are +inf: it is the last candidate, not a fault
    full = np.ones(n, dtype=bool)
    order, _ = _truncate(obj, full, n_keep)
    assert len(order) == n - n_keep and 17 not in order.tolist()


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_an_infinite_objective_gives_infinite_distances_and_k_rows_still_leave(bad):
    n, n_keep = 200, 80
    obj = ref.objectives(n, 3, "front", 5).copy()
    obj[17, 1] = bad
    mask = np.ones(n, dtype=bool)
    order, n_rescans = _truncate(obj, mask, n_keep)  # _truncate asserts that exactly k rows left
    assert len(order) == n - n_keep and 17 not in order.tolist()  # every other row has a finite neighbour
    _certificate(f"(200, 3) front with {bad}", obj, mask, order, n_rescans)


def test_rows_without_a_finite_neighbour_leave_lowest_index_first():
    n = 64
    obj = ref.objectives(n, 3, "front", 5).copy()
    obj[:, 0] = np.inf  # inf − inf: every d2 is NaN, which counts as +inf
    mask = np.ones(n, dtype=bool)
    mask[::5] = False
    order, n_rescans = _truncate(obj, mask, 20)
    assert np.array_equal(order, np.flatnonzero(mask)[: int(mask.sum()) - 20]) and n_rescans == 0


# ---------------------------------------------------------------- 6. caps
def _frozen_tell_selection(merged_fit, pop_size):
    sig = spea2_ops.cal_fitness(merged_fit)
    mask = sig < 1
    num_valid = int(mask.sum())
    if num_valid <= pop_size:
        order = torch.argsort(sig, stable=True)
    else:
        keep = spea2_ops.truncation(merged_fit, num_valid - pop_size, mask)
        order = torch.argsort((~keep).to(torch.int64), stable=True)
    return order[:pop_size]


def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    n = spea2_ops.N_CAP + 1
    obj = _dev(ref.objectives(n, 3, "uniform", 1))
    want = _frozen_tell_selection(obj, n // 2)
    _no_kernel(monkeypatch, "spea2_truncate")
    got = spea2_ops.select(obj, n // 2)
    assert got.is_cuda and torch.equal(got, want)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[:300] = True
    assert torch.equal(spea2_ops.truncate(obj, mask, 290), spea2_ops.truncation(obj, 10, mask))


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    obj = _dev(ref.objectives(100, spea2_ops.M_CAP + 1, "uniform", 1))
    sig = spea2_ops.cal_fitness(obj)
    want = _frozen_tell_selection(obj, 50)
    _no_kernel(monkeypatch, "spea2_fitness", "spea2_truncate")
    assert torch.equal(spea2_ops.fitness(obj), sig)
    assert torch.equal(spea2_ops.select(obj, 50), want)


# ---------------------------------------------------------------- 7. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=5, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.SPEA2(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


@pytest.fixture
def kernel_calls(monkeypatch):
    ops, calls = _ext.ops(), {"spea2_fitness": 0, "spea2_truncate": 0}

    class Counting:
        def __getattr__(self, name):
            if name in calls:
                calls[name] += 1
            return getattr(ops, name)

    monkeypatch.setattr(spea2_ops._ext, "ops", lambda: Counting())
    return calls


def test_generation_is_captured_and_is_bitwise_the_eager_one(kernel_calls):
    _, a = _run(False)
    assert kernel_calls["spea2_fitness"] >= 2 and kernel_calls["spea2_truncate"] >= 1  # ask and tell
    before = dict(kernel_calls)
    wf, b = _run(True)
    assert wf._graph is not None
    assert kernel_calls["spea2_fitness"] > before["spea2_fitness"] and kernel_calls["spea2_truncate"] > before["spea2_truncate"]
    assert torch.isfinite(a.fitness).all()
    assert torch.equal(a.population, b.population) and torch.equal(a.fitness, b.fitness)
    _, c = _run(True)
    assert torch.equal(b.population, c.population) and torch.equal(b.fitness, c.fitness)


def test_ask_and_tell_read_nothing_on_the_host(monkeypatch):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.SPEA2(lb, ub, M_, POP)
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
        _, a = algo.ask(a)
        a = algo.tell(a, fit)
    torch.cuda.synchronize()
    assert a.fitness.shape == (POP, M_) and torch.isfinite(a.fitness).all()


def test_spea2_converges_on_dtlz2_on_the_device():
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] SPEA2, DTLZ2 d 12 m 3, N 100, 100 generations: {igd:.4f}")
    assert igd < 0.1
