"""KnEA's knee-point selection on the CPU: ``KnEA.tell`` through ``ops.knea.select`` against a verbatim copy of the loop
it ran before, the torch host path against the numpy reference of ``_knea_reference.py`` on fixtures whose result does
not hang on float32 rounding, and the reference itself on inputs whose result can be read off the contract.

The host path evaluates the keys in float32 (a float32 LAPACK solve and a float32 dot), so a fixture is compared with
it only when b ≥ 1e-5, the float32 keys of every front are at least 1e-5 apart (``gap``) or equal, and the result does
not depend on the order of equal keys (the reference run with ties by descending position gives the same output).
``a``, the distance of a float64 key from a float32 rounding boundary, cannot exceed half a float32 ulp (6e-8), so it
is held to the kernel's 1e-12; what float32's reach has to clear is the distance between two keys, which is ``gap``."""
import numpy as np
import pytest
import torch

import _knea_reference as ref
import evoxmi.algorithms as A
from evoxmi import random as rnd
from evoxmi.algorithms.mo import knea as knea_mod
from evoxmi.algorithms.mo.knea import _plane, calc_DW  # noqa: F401  (both stay importable from here)
from evoxmi.operators.selection.non_dominate import non_dominated_sort
from evoxmi.ops import knea as knea_ops


# ---------------------------------------------------------------- 1. tell against the loop it ran before
def _tell_before(self, state, fitness):
    """``KnEA.tell`` as it was before the selection moved into ``ops.knea`` (verbatim)."""
    N, m = self.pop_size, self.n_objs
    pop = torch.cat([state.population, state.next_generation])
    obj = torch.cat([state.fitness, fitness])
    rank = non_dominated_sort(obj)
    order = torch.argsort(rank, stable=True)
    rank, pop, obj = rank[order], pop[order], obj[order]
    last = int(rank[N])
    n = obj.shape[0]
    knee = torch.zeros(n, dtype=torch.bool, device=obj.device)
    r, t = float(state.r), float(state.t)
    plane = torch.ones(m, device=obj.device)
    for i in range(last + 1):
        idx = torch.nonzero(rank == i).flatten()
        f = obj[idx]
        mx, mn = f.max(0).values, f.min(0).values
        plane = _plane(f[torch.argmax(f, 0)], m)
        dist_order = idx[torch.argsort(f @ plane, stable=True)]
        r = r * float(torch.exp(torch.tensor(-(1 - t / self.knee_rate) / m)))
        R = (mx - mn) * r
        cand = torch.ones(n, dtype=torch.bool, device=obj.device)
        cand[idx] = True
        front_knee = torch.zeros(n, dtype=torch.bool, device=obj.device)
        front_knee[idx] = True
        for p in dist_order.tolist():
            if bool(front_knee[p]):
                nb = (torch.abs(obj[idx] - obj[p]) < R).all(1)
                nb_idx = idx[nb]
                front_knee[nb_idx] = False
                front_knee[p] = True
        knee |= front_knee
        t = float((front_knee[idx]).sum()) / idx.shape[0]
    knee &= rank <= last
    selected = (rank < last) | knee
    dif = int(selected.sum()) - N
    last_mask = rank == last
    if dif > 0:
        cand = torch.nonzero(knee & last_mask).flatten()
        far = cand[torch.argsort(-(obj[cand] @ plane), stable=True)][:dif]
        selected[far] = False
    elif dif < 0:
        cand = torch.nonzero(~knee & last_mask).flatten()
        near = cand[torch.argsort(obj[cand] @ plane, stable=True)][:-dif]
        selected[near] = True
    idx = torch.nonzero(selected).flatten()[:N]
    return state.update(population=pop[idx], fitness=obj[idx], knee=knee[idx], r=r, t=t)


@pytest.mark.parametrize("seed,m,N", [(1, 3, 60), (2, 2, 40), (3, 3, 100)])
def test_tell_equals_the_loop_it_ran_before(seed, m, N):
    d = 8
    algo = A.KnEA(torch.zeros(d), torch.ones(d), m, N)
    st = algo.setup(rnd.PRNGKey(seed))
    assert isinstance(st.r, float) and isinstance(st.t, float)  # Python floats on the CPU
    kind = "front" if seed % 2 else "uniform"
    st = algo.init_tell(st, torch.from_numpy(ref.objectives(N, m, kind, 10 * seed)) * 1.2)
    for gen in range(3):  # r and t carry over: three merged populations per seed
        off, st = algo.ask(st)
        fit = torch.from_numpy(ref.objectives(N, m, kind, 10 * seed + gen + 1)) * (1.1 - 0.1 * gen)
        want = _tell_before(algo, st, fit)
        st = algo.tell(st, fit)
        for name in ("population", "fitness", "knee"):
            assert torch.equal(getattr(st, name), getattr(want, name)), f"{name} differs in generation {gen}"
        assert st.r == want.r and st.t == want.t and isinstance(st.r, float) and isinstance(st.t, float)


# ---------------------------------------------------------------- 2. the torch path against the reference
# (n, m, layers, kind, seed, N, r, t)
FIXTURES = [(200, 3, 6, "uniform", 2, 100, 1.0, 0.0), (200, 3, 6, "uniform", 2, 66, 0.3, 0.6), (200, 3, 6, "uniform", 4, 66, 1.0, 0.0),
            (200, 2, 4, "front", 3, 100, 1.0, 0.0), (200, 2, 4, "front", 4, 66, 0.3, 0.6), (120, 3, 3, "front", 1, 40, 0.3, 0.6),
            (120, 3, 3, "front", 2, 60, 1.0, 0.0), (120, 3, 3, "front", 5, 40, 1.0, 0.0), (65, 2, 4, "uniform", 0, 21, 0.3, 0.6),
            (65, 2, 4, "uniform", 4, 21, 1.0, 0.0)]


@pytest.mark.parametrize("n,m,layers,kind,seed,N,r,t", FIXTURES)
def test_host_path_equals_the_reference(n, m, layers, kind, seed, N, r, t):
    obj, rank = ref.cached_case(n, m, layers, kind, seed)
    idx, knee, r1, t1, q = ref.select(obj, rank, N, r, t, 0.5)
    print(f"[knea] ({n}, {m}, {layers}) {kind} seed {seed} N {N}: a {q['a']:.1e} b {q['b']:.1e} c {q['c']:.1f} gap {q['gap']:.1e} "
          f"dif {q['dif']} fallbacks {q['fallbacks']} (front, knees) {q['knees']}")
    assert ref.qualifies(q, b=1e-5) and q["gap"] >= 1e-5, "the fixture no longer qualifies"
    other = ref.select(obj, rank, N, r, t, 0.5, ties="descending")
    assert np.array_equal(other[0], idx) and np.array_equal(other[1], knee), "the fixture depends on the order of tied keys"
    got = knea_ops.select(torch.from_numpy(obj), torch.from_numpy(rank), N, r, t, 0.5)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.bool and isinstance(got[2], float) and isinstance(got[3], float)
    assert np.array_equal(got[0].numpy(), idx) and np.array_equal(got[1].numpy(), knee)
    assert abs(got[2] - r1) <= 1e-6 * r1 and got[3] == t1


def test_fixtures_cover_both_signs_of_dif_and_dif_zero():
    signs = {ref.select(*ref.cached_case(n, m, layers, kind, seed), N, r, t, 0.5)[4]["dif"] for n, m, layers, kind, seed, N, r, t in FIXTURES}
    assert signs == {-1, 0, 1}


# ---------------------------------------------------------------- 3. the reference on hand cases
def _hand(name):
    obj, rank, N, r, t = ref.hand_cases()[name]
    return ref.select(obj, rank, N, r, t, 0.5)


def test_reference_a_front_of_one_row():
    idx, knee, r, t, q = _hand("one_row_front")
    assert q["knees"][0] == (1, 1) and knee[0] and q["fallbacks"] >= 1 and idx[0] == 0 and idx.size == 2
    assert r == pytest.approx(0.3 * np.exp(-0.5) * np.exp(-(1 - 1 / 0.5) / 2))  # front 0: t = 0; front 1: t = 1


def test_reference_all_rows_equal():
    idx, knee, r, t, q = _hand("all_equal")
    assert knee.all() and t == 1.0 and q["fallbacks"] == 1 and q["dif"] == 1
    assert idx.tolist() == [2, 3, 4, 5]  # equal keys: the lower positions are unselected first


def test_reference_a_block_of_copies_keeps_the_first():
    idx, knee, r, t, q = _hand("copies")
    assert r == 0.01 and knee[4] and not knee[5:9].any() and knee[:4].all() and knee[9:].all()
    assert q["knees"] == [(12, 8)] and t == 8 / 12


def test_reference_a_zero_column():
    idx, knee, r, t, q = _hand("zero_column")
    assert q["fallbacks"] == 1 and knee.all() and idx.size == 5


def test_reference_the_three_signs_of_dif():
    for name, sign, want in (("dif_positive", 1, [1, 9]), ("dif_zero", 0, [0, 1, 9]), ("dif_negative", -1, [0, 1, 2, 3, 4, 9])):
        idx, knee, r, t, q = _hand(name)
        assert q["dif"] == sign and np.flatnonzero(knee).tolist() == [0, 1, 9] and idx.tolist() == want, name


def test_hand_cases_through_the_host_path_keep_n_rows():
    for name, (obj, rank, N, r, t) in ref.hand_cases().items():
        idx, knee, _, _ = knea_ops.select(torch.from_numpy(obj), torch.from_numpy(np.asarray(rank, dtype=np.int64)), N, r, t, 0.5)
        assert idx.shape == (N,) and len(set(idx.tolist())) == N and knee.shape == (obj.shape[0],), name


def test_module_exports():
    assert knea_mod._plane is knea_ops._plane and callable(knea_ops.knee_select_host)
    assert knea_ops.N_CAP == 8192 and knea_ops.M_CAP == 16
    assert not knea_ops.on_device(200, 3, "cpu")
