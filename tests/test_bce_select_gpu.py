"""``bce_select.hip`` against host references, and BCE-IBEA generations captured into a hipGraph (MI355X, marked
gpu).  The references are numpy float64 on the same float32 objectives (``_bce_reference.py``;
``test_bce_select.py`` pins them to the torch path).

Inputs: ``front`` is |normal| + 1e-3 normalised to the unit sphere (every row non-dominated), ``uniform`` is rand in
[0, 1]^m and is passed an all-true mask, because few of its rows are non-dominated.  Every test keeps half of the
masked rows.

Rounding count, u = 2⁻²⁴, first order.  δ_k = (o_ik − o_jk) / span_k: the difference rounds once, the span (a
float32 difference) once, the division once, 3u; its square 6u; the m fmaf round once each and every term is
positive: d2 within (m + 6)·u.  t = sqrt(third smallest d2): (m/2 + 3)·u and one rounding, (m/2 + 4)·u; the order
statistic is monotone in its arguments, so the bound holds where float32 picks another neighbour.  r = Σ t / n_nd:
the longest path of the ordered sum has depth = ⌈n / 256⌉ + 9 additions at most (the thread's chain, six tree
levels, three wave sums), the division rounds once: (m/2 + 5 + depth)·u.  A factor R = min(sqrt(d2) / r, 1):
(m/2 + 4) + (m/2 + 5 + depth) + 1 = (m + 10 + depth)·u (the clamp is monotone).  A product of F factors below 1
(the factors equal to 1 multiply exactly): F·(m + 10 + depth)·u and F − 1 multiplications,
b(F, m, n) = (F·(m + 11 + depth) − 1)·u (``_bce_reference.product_bound``).

Niche radius: t within (m/2 + 4)·u and r within (m/2 + 5 + depth)·u relative of float64, asserted.

Exact order.  The kernel compares the rows on P (the least P is the greatest 1 − P).  Where the float64 reference
has, at every step, its two smallest live products either exactly tied or at a relative gap of at least 1e-4, every
exact tie a pair of rows that are each other's only live neighbour within r (one symmetric factor each: bitwise equal
in float32 too, the lower index leaves), and b(F, m, n) for the reference's own F at most a quarter of 1e-4 (the two
products err by b each, so half the gap would do), the kernel's removal order equals the reference's.  All three are
asserted on the reference, so an input that stops qualifying fails.

Certificate, every other input.  The kernel's own order is replayed in float64; at each step the removed row's
float64 P is at most (1 + b) times the float64 minimum over the live rows, with b for the case's m, n and the
reference's F.  (Both products err, so the two-sided derivation gives (1 + b) / (1 − b) ≈ 1 + 2b; the test asserts the
tighter 1 + b.)

Observed on an MI355X (gfx950), worst over the cases of each test:

==============================  ==============================================================
quantity                        worst observed
==============================  ==============================================================
t, relative error               2.48·2⁻²⁴ at (257, 16) uniform (bound 12·2⁻²⁴); 2.36·2⁻²⁴ at
                                (1000, 10), 1.96·2⁻²⁴ at m = 3, 1.61·2⁻²⁴ at m = 2
r, relative error               1.36·2⁻²⁴ at (257, 3) uniform (bound 17.5·2⁻²⁴)
exact order, smallest gap       1.09e-4 ((257, 3) uniform seed 1), 1.67e-4 (seed 3), 1.88e-4
                                ((64, 2) front seed 3); 1–33 tied steps, at most 10 factors,
                                bound at most 1.48e-5; the orders are equal in all 15 cases
certificate, ratio − 1          exactly 0 in every case (bounds b of 1.0e-5 to 4.5e-5; 2.8e-4 with
                                an infinite objective, 199 factors)
rescans per removal             2.63–2.71 at m ≤ 5, 2.89 at m = 10, 3.32 at m = 16
all rows equal, n = 2049        0 rescans for 1025 removals; duplicate block: 2.0 per removal;
                                an infinite objective: 0
exploration                     no row differs from float64; 0–3 rows of 257 exempt, 1–2 of 513
                                (n_nd = n), 0–1 with n_nd = n // 2
IGD after 100 generations       0.0576 (the CPU run measures .055)
==============================  ==============================================================
"""
import warnings

import numpy as np
import pytest
import torch

import _bce_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.metrics import IGD
from evoxmi.ops import _ext
from evoxmi.ops import bce as bce_ops
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

    monkeypatch.setattr(bce_ops._ext, "ops", lambda: NoKernel())


def _depth(n):
    return -(-n // 256) + 9


# ---------------------------------------------------------------- 1. niche radius
@pytest.mark.parametrize("kind", ["front", "uniform"])
@pytest.mark.parametrize("n,m", [(3, 2), (65, 2), (257, 3), (513, 5), (257, 16), (1000, 10)])
def test_niche_radius_is_within_its_bound(n, m, kind):
    obj = ref.cached_objectives(n, m, kind, 100 * n + m)
    mask = ref.nd_mask(obj) if kind == "front" else None
    t64, r64, _ = ref.niche(obj, mask)
    r, t = bce_ops.niche_radius(_dev(obj), None if mask is None else _dev(mask))
    assert t.is_cuda and t.dtype == torch.float32 and t.shape == (n,) and r.dim() == 0
    t, r = t.cpu().numpy().astype(np.float64), float(r)
    fin = np.isfinite(t64)
    assert np.array_equal(np.isfinite(t), fin) and np.array_equal(t[~fin], t64[~fin])
    e_t = float(np.max(np.abs(t[fin] - t64[fin]) / np.where(t64[fin] > 0, t64[fin], 1.0))) if fin.any() else 0.0
    b_t, b_r = (m / 2 + 4) * U, (m / 2 + 5 + _depth(n)) * U
    if np.isfinite(r64):
        e_r = abs(r - r64) / r64
    else:
        e_r = 0.0 if r == r64 else float("inf")
    print(f"[niche] ({n}, {m}) {kind}: t rel {e_t / U:.2f}·2^-24 (bound {b_t / U:.1f}), r rel {e_r / U:.2f}·2^-24 (bound {b_r / U:.1f})")
    assert e_t <= b_t and e_r <= b_r
    if mask is not None:  # outside the mask t is 0
        assert (t[~mask] == 0).all()


# ---------------------------------------------------------------- 2. removal, exact
def _select(obj, n_keep, mask=None, nd=None):
    """``pc_select`` with its outputs checked against one another; ``mask`` is handed to the kernel, ``nd`` is the
    reference's non-dominated set where the caller already has it."""
    n = obj.shape[0]
    idx, n_nd, order, n_rescans = bce_ops.pc_select(_dev(obj), n_keep, return_order=True, mask=None if mask is None else _dev(mask))
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.shape == (n_keep,) and n_nd.dtype == torch.int64 and n_nd.dim() == 0
    assert order.dtype == torch.int64 and order.shape == (max(n - n_keep, 0),) and n_rescans.dtype == torch.int32
    m_ = mask if mask is not None else nd if nd is not None else ref.nd_mask(obj)
    count = int(m_.sum())
    assert int(n_nd) == count
    k = max(0, count - n_keep)
    idx, order = idx.cpu().numpy(), order.cpu().numpy()
    assert (order[k:] == -1).all() and (order[:k] >= 0).all() and (order[:k] < n).all()
    assert len(set(order[:k].tolist())) == k and m_[order[:k]].all(), "a row left twice or from outside the mask"
    assert np.array_equal(idx, ref.select_indices(n, m_, order[:k], n_keep)), "idx is not the mask without the removed rows"
    return order[:k], int(n_rescans)


EXACT = ([(64, 2, "front", s) for s in range(5)] + [(200, 3, "front", s) for s in range(5)] + [(257, 3, "front", 0), (257, 3, "front", 4)]
         + [(257, 3, "uniform", s) for s in (0, 1, 3)])


@pytest.mark.parametrize("n,m,kind,seed", EXACT)
def test_removal_matches_the_float64_order(n, m, kind, seed):
    obj, mask, (want, gap, ties_ok, ties, factors, ref_rescans) = ref.cached_removal(n, m, kind, seed, kind == "uniform")
    assert mask.all()
    bound = ref.product_bound(factors, m, n)
    print(f"[exact] ({n}, {m}) {kind} seed {seed}: gap {gap:.3e}, tied steps {ties}, factors {factors}, bound {bound:.3e}, "
          f"reference rescans {ref_rescans}")
    assert gap >= 1e-4, f"the input no longer qualifies: gap {gap:.3e}"
    assert ties_ok, "the input no longer qualifies: an exact tie that is not a mutual pair"
    assert bound <= 0.25e-4, f"the input no longer qualifies: bound {bound:.3e}"
    order, n_rescans = _select(obj, n // 2, mask if kind == "uniform" else None, mask)
    print(f"[exact] ({n}, {m}) {kind} seed {seed}: kernel rescans {n_rescans} for {len(order)} removals")
    assert np.array_equal(order, want)


# ---------------------------------------------------------------- 3. removal, certificate
def _certificate(what, obj, mask, order, n_rescans):
    n, m = obj.shape
    worst, factors = ref.replay_ratio(obj, mask, order)
    bound = 1 + ref.product_bound(factors, m, n)
    print(f"[certificate] {what}: worst ratio − 1 = {worst - 1.0:.3e} (bound {bound - 1.0:.3e}, {factors} factors), rescans / removal "
          f"{n_rescans / max(len(order), 1):.3f}")
    assert worst <= bound, f"{what}: ratio − 1 = {worst - 1.0:.3e} > {bound - 1.0:.3e}"


# (1500, 4) is beyond the issue's list: the only size class with eight rows per thread in four waves (two partial products
# per thread) and the only case with four objectives
@pytest.mark.parametrize("n,m,kind", [(513, 5, "front"), (257, 10, "front"), (257, 16, "front"), (1500, 4, "front"),
                                      (2049, 3, "uniform"), (4097, 5, "uniform"), (8192, 3, "front")])
def test_removal_certificate(n, m, kind):
    obj = ref.cached_objectives(n, m, kind, 100 * n + m)
    mask = np.ones(n, dtype=bool)
    given, nd = (mask, None) if kind == "uniform" else (None, ref.nd_mask(obj))  # a front: the kernel finds the mask itself
    assert nd is None or nd.all()
    order, n_rescans = _select(obj, n // 2, given, nd)
    assert len(order) == n - n // 2
    _certificate(f"({n}, {m}) {kind}", obj, mask, order, n_rescans)
    again, _ = _select(obj, n // 2, given, nd)
    assert np.array_equal(again, order)


# ---------------------------------------------------------------- 4. edges
def test_equal_rows_leave_in_index_order_without_rescans():
    n, n_keep = 2049, 1024
    obj = np.full((n, 3), 0.25, dtype=np.float32)
    order, n_rescans = _select(obj, n_keep)  # no row dominates an equal row: the mask is everything
    assert np.array_equal(order, np.arange(n - n_keep))
    print(f"[edges] all equal n {n}: rescans {n_rescans} for {n - n_keep} removals")
    assert n_rescans == 0  # r = 0: every factor is NaN, a removal only lowers the NaN counts


def test_a_block_of_duplicates_inside_a_front():
    n = 400
    obj = ref.objectives(n, 3, "front", 6).copy()
    obj[100:150] = obj[5]  # 51 equal rows, 5 and 100 … 149: factor 0 to one another, P = 0
    mask = np.ones(n, dtype=bool)
    order, n_rescans = _select(obj, n - 49)
    assert order.tolist() == [5] + list(range(100, 148))
    order, n_rescans = _select(obj, n // 2)  # past the block: all but one of the equal rows go first
    assert order[:50].tolist() == [5] + list(range(100, 149))
    _certificate("duplicate block in (400, 3) front", obj, mask, order, n_rescans)


def test_fewer_non_dominated_rows_than_places_pads_with_the_first():
    n, n_keep = 257, 100
    obj = ref.objectives(n, 3, "uniform", 8)
    mask = ref.nd_mask(obj)
    count = int(mask.sum())
    assert 0 < count <= n_keep
    order, n_rescans = _select(obj, n_keep)  # _select asserts idx against the padded reference indices
    assert len(order) == 0 and n_rescans == 0
    idx, n_nd = bce_ops.pc_select(_dev(obj), n_keep)
    rows = np.flatnonzero(mask)
    assert np.array_equal(idx.cpu().numpy(), np.concatenate([rows, np.full(n_keep - count, rows[0])])) and int(n_nd) == count
    idx, n_nd = bce_ops.pc_select(_dev(obj), count)  # n_nd = n_keep: every masked row, no padding
    assert np.array_equal(idx.cpu().numpy(), rows)


def test_one_row_more_than_places():
    n, m = 130, 3
    obj = ref.objectives(n, m, "front", 2)
    order, n_rescans = _select(obj, n - 1)
    assert len(order) == 1
    _certificate(f"({n}, {m}) front, one removal", obj, np.ones(n, dtype=bool), order, n_rescans)


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_an_infinite_objective_still_removes_exactly_k_rows(bad):
    n, n_keep = 200, 100
    obj = ref.objectives(n, 3, "front", 5).copy()
    obj[17, 1] = bad
    mask = np.ones(n, dtype=bool)
    order, n_rescans = _select(obj, n_keep, mask)  # _select asserts k distinct rows in range; the call returned: it terminates
    assert len(order) == n - n_keep
    _certificate(f"(200, 3) front with {bad}", obj, mask, order, n_rescans)


def test_over_the_row_cap_runs_the_torch_path(monkeypatch):
    n = bce_ops.N_CAP + 1
    obj = ref.objectives(n, 3, "uniform", 1)
    mask = ref.nd_mask(obj)
    assert int(mask.sum()) <= n // 2
    _no_kernel(monkeypatch, "bce_pc_select", "bce_niche", "bce_explore")
    idx, n_nd = bce_ops.pc_select(_dev(obj), n // 2)
    assert idx.is_cuda and int(n_nd) == int(mask.sum())
    assert np.array_equal(idx.cpu().numpy(), ref.select_indices(n, mask, [], n // 2))


def test_over_the_objective_cap_runs_the_torch_path(monkeypatch):
    obj = _dev(ref.objectives(100, bce_ops.M_CAP + 1, "uniform", 1))
    want, n_nd = bce_ops.pc_selection_indices(obj, 50)
    s_want = bce_ops.exploration(obj, obj.flip(0), n_nd, 100)
    _no_kernel(monkeypatch, "bce_pc_select", "bce_niche", "bce_explore")
    got, n_nd2 = bce_ops.pc_select(obj, 50)
    assert int(n_nd2) == n_nd and torch.equal(got, want)
    assert torch.equal(bce_ops.explore(obj, obj.flip(0), n_nd, 100), s_want)


# ---------------------------------------------------------------- 5. exploration
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("part", [1, 2])  # n_nd = n and n_nd = n // 2: the radius scales with the device word
@pytest.mark.parametrize("n,m", [(100, 3), (257, 3), (513, 5), (257, 10)])
def test_exploration_matches_float64_outside_the_radius_band(n, m, part, seed):
    pc = ref.objectives(n, m, "front", seed)
    rng = np.random.default_rng(1000 + seed)
    npc = (ref.objectives(n, m, "front", 100 + seed) * (1 + 0.05 * rng.random((n, 1)))).astype(np.float32)
    count = n // part
    want, near = ref.exploration(pc, npc, count)
    n_nd = torch.tensor(count, dtype=torch.int64, device="cuda")
    s = bce_ops.explore(_dev(pc), _dev(npc), n_nd, n)
    assert s.is_cuda and s.dtype == torch.bool and s.shape == (n,)
    s = s.cpu().numpy()
    print(f"[explore] ({n}, {m}) n_nd {count} seed {seed}: {int(want.sum())} candidates, {int(near.sum())} rows exempt, "
          f"{int((s != want).sum())} rows differ")
    assert near.sum() <= 0.02 * n
    assert np.array_equal(s[~near], want[~near])
    if part == 1:
        assert 0 < want.sum() < n  # both answers occur
    else:  # the smaller radius changes the answer: a kernel that ignored n_nd would fail here
        full, near_full = ref.exploration(pc, npc, n)
        assert (want & ~full & ~near & ~near_full).any()


# ---------------------------------------------------------------- 6. generations
D_, M_, POP = 12, 3, 100


def _run(graph, gens=6, seed=11):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    wf = StdWorkflow(A.BCEIBEA(lb, ub, M_, POP), DTLZ2(d=D_, m=M_), graph=graph)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    return wf, st.get_child_state("algorithm")


def test_generation_is_captured_in_both_variants_and_matches_eager():
    _, a = _run(False)
    wf, b = _run(True)
    assert wf._graph is not None and set(wf._graphs) == {"explore", "ibea"}
    fa, fb = a.fitness, b.fitness
    fin = torch.isfinite(fa)
    assert torch.equal(fin, torch.isfinite(fb))
    assert torch.allclose(fa[fin], fb[fin], rtol=1e-5, atol=1e-5)
    assert int(a.counter) == 6 and int(b.counter) == 6 and int(a.n_nd) == int(b.n_nd)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        wf, c = _run("auto")
    # graph="auto" keeps BCE-IBEA eager (BCEIBEA.graph_auto), without a failed capture behind it
    assert not [w for w in caught if "not capturable" in str(w.message)]
    assert wf._graph is None and not wf._graph_failed and torch.equal(a.fitness, c.fitness)


def test_ask_and_tell_read_nothing_on_the_host(monkeypatch):
    lb, ub = torch.zeros(D_, device="cuda"), torch.ones(D_, device="cuda")
    algo = A.BCEIBEA(lb, ub, M_, POP)
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
        for variant in ("explore", "ibea"):
            with algo.graph_variant_context(variant):
                _, a = algo.ask(a)
                a = algo.tell(a, fit)
    torch.cuda.synchronize()
    assert a.fitness.shape == (POP, M_) and torch.isfinite(a.fitness).all() and int(a.counter) == 4


def test_bce_ibea_converges_on_dtlz2_on_the_device():
    _, a = _run(True, gens=100, seed=42)
    fit = a.fitness
    assert torch.isfinite(fit).all()
    igd = float(IGD(DTLZ2(d=D_, m=M_).pf())(fit.cpu()))
    print(f"[igd] BCEIBEA, DTLZ2 d 12 m 3, N 100, 100 generations: {igd:.4f}")
    assert igd < 0.1
