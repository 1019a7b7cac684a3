"""The MOEA/D generation kernels of ``csrc/kernels/moead.hip`` and the one-wave scan of ``mo_scan.hip`` one by one,
each against the float64 references of ``_moead_reference.py`` at the shapes where its code takes another path.
Runs on an MI355X (marked gpu).  Inputs are drawn on the CPU from seeded generators; the ops are called through
``evoxmi.ops.mo``.

What is compared how
--------------------
* Index outputs, copies and selections (``parents``, ``replace``/``halo_replace`` ``win`` and objective rows,
  ``select_rows``, ``halo_gather``, the ``row0``/``rows``/``win``/``out=`` variants of ``variation``): bit for bit.
* ``replace`` decides on float32 aggregates, the reference on float64 ones.  Every case first asserts, on the CPU,
  that no decision of the reference is closer than 64 float32 ulps (``margin``: best against occupant, best against
  the second-best distinct value); no slot is excluded.  64 ulps cover the kernels' error: at most M + 2 ≤ 18
  roundings of a sum of positive terms of the aggregate's magnitude for weighted sum, two such sums, a division
  and a square root for PBI (whose d1 and d2 are each within a few ulps of the aggregate's magnitude), one rounding
  per term for the Tchebycheff forms.  Seeds were chosen on the CPU so that the margin holds.
* ``variation``: the project's rule for accumulated float32 results (``test_cmaes_kernels_gpu.py``): with ``e_t``
  the largest deviation of the CPU float32 operators (``SimulatedBinary(type=2)`` + ``Polynomial`` + clamp) from
  the float64 reference and ``e_k`` the kernel's, ``e_k <= 4·e_t + 2·ulp32(max |ref|)``, per group of columns of
  equal span.  The branch-coverage conditions (both PM branches occur at N = 101; rows without crossover occur
  at N = 101, pro_c = 0.6) are asserted from the reference's counts before the kernel runs; at N = 1 and 2 there
  are too few rows to demand them and pro_c = 1 never skips a crossover.
* ``moead_scan``: funcs 0 and 3 (one rounding per term, no a·b + c to contract) bit for bit against the float32 CPU
  ``moead_scan``; funcs 1 and 2 against ``scan_ref`` after asserting its margin of 64 ulps.  In the NaN cases with
  ``update_z`` the ideal point turns NaN and stays NaN, as ``torch.minimum`` has it.

``halo_gather`` with world 3 gives every rank a buffer of its own (the IPC layout), the empty rank a full-size
poison buffer: with one contiguous buffer (``_tell_owner`` without IPC, the world 1 and the ``one buffer`` cases)
every rank's pointer and start resolve to the same address, so a wrong rank lookup would go unseen.

Seeded mutations and the cases that catch them: dropping chain u >= 1 — every replace row longer than 64;
an off-by-one in the ``q0 + 64·u < e`` tail — rows of 63/64/65, 255/256/257, 511/512/513 with the minimum at the
last position (``test_replace_minimum_at_last_position``); the lowest-index tie-break — ``test_replace_ties``;
``<=`` against the occupant — ``test_replace_best_equal_to_occupant``; ignoring ``pro_c`` — the no_x rows of the
pro_c = 0.6 variation cases; ``row0``-relative counters — the ``row0``/``rows`` slices of parents and variation;
a wrong rank lookup in ``starts`` — ``test_halo_gather`` at world 3.

Observed on an MI355X (gfx950), largest over the cases of each test; the baseline for later rewrites:

===========================================  ================  ================  ==========================
check                                        worst e_k / e_t   worst e_k / bound  smallest margin (ulp32)
===========================================  ================  ================  ==========================
variation4 (d % 4 == 0)  span 1e-3           1.00              0.19
variation4               span 1              1.25              0.21
variation4               span 4              1.13              0.19
variation4               span 1e3            1.50              0.20
variation1 (other d)     span 1e-3           1.00              0.19
variation1               span 1              1.00              0.19
variation1               span 4              1.30              0.24
variation1               span 1e3            1.60              0.27
variation row0/rows, win, out=               exact
parents, select_rows, halo_gather, first     exact
replace / halo_replace  tchebycheff          exact                               3908
replace / halo_replace  pbi                  exact                               7355
replace / halo_replace  weighted_sum         exact                               951
replace / halo_replace  modified_tchebycheff exact                               5008
replace / halo_replace  tchebycheff_norm     exact                               6966
moead_scan  tchebycheff, modified            exact (float32 CPU scan)
moead_scan  pbi                              exact                               89
moead_scan  weighted_sum                     exact                               85
===========================================  ================  ================  ==========================

``bound`` is ``4·e_t + 2·ulp32(max |ref|)``.  e_t itself is up to 1.3e-4 at span 1e3 (two ulp32 of 1e3) and 8.4e-7
over the other spans of these inputs, and in most small cases e_k equals e_t to the digit (the same rounded result);
where e_t = 0 (N = 1 cases without a site in the column group) e_k was 0 too.  ``sbx_child``'s ``__log2f`` stays
inside the rule: no accurate ``log2f`` and no wider factor was needed.  In every replace case between 0.38 and 0.55
of the slots replace.
"""
import functools

import pytest
import torch

import _moead_reference as ref
from evoxmi.ops import _ext
from evoxmi.ops import mo as mo_ops
from evoxmi.ops import random as rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
FUNCS = ["tchebycheff", "pbi", "weighted_sum", "modified_tchebycheff", "tchebycheff_norm"]
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 10007 + int(v) + 1
    return torch.Generator().manual_seed(s)


def _dev(*ts):
    out = tuple(t.to(DEV) for t in ts)
    return out if len(out) > 1 else out[0]


def _i32(t):
    return t.to(torch.int32).to(DEV)


def _same(a, b):
    """Bit-for-bit on values, NaN equal to NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------- parents
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129, 300])
@pytest.mark.parametrize("N", [1, 5, 300])
def test_parents(N, T):
    nb = torch.randint(0, 1_000_000, (N, T), generator=_gen(1, N, T))
    key = rnd.PRNGKey(9 + N + T)
    r0, r1 = ref.parents_ref(nb, key)
    p0, p1 = mo_ops.moead_parents(_dev(nb), _dev(key))
    assert p0.dtype == torch.int32 and p0.shape == (N,)
    assert torch.equal(p0.cpu().long(), r0) and torch.equal(p1.cpu().long(), r1)
    if T == 1:
        assert torch.equal(r0, r1)
    for row0, rows in ((0, 1), (3, 1), (N - 2, 2)):
        if row0 < 0 or row0 + rows > N:
            continue
        s0, s1 = ref.parents_ref(nb, key, row0, rows)
        q0, q1 = mo_ops.moead_parents(_dev(nb), _dev(key), row0, rows)
        assert torch.equal(q0.cpu().long(), s0) and torch.equal(q1.cpu().long(), s1), (row0, rows)


# ---------------------------------------------------------------- variation
SPANS = (1e-3, 1.0, 4.0, 1e3)
DIS_C, DIS_M = 20.0, 20.0


@functools.lru_cache(maxsize=None)
def _var_case(N, d, mode):
    """Bounds differ per column (spans of 1e-3, 1, 4 and 1e3: column 0 has 1e-3, the last column 1e3), parents
    inside them.  mode 0: (pro_c, pro_m) = (1, 1); mode 1: (0.6, d / 2)."""
    from evoxmi.operators.crossover import SimulatedBinary
    from evoxmi.operators.mutation import Polynomial

    g = _gen(2, N, d)
    group = torch.randint(0, len(SPANS), (d,), generator=g)
    group[0], group[-1] = 0, len(SPANS) - 1
    lb = torch.rand(d, generator=g) * 4 - 2
    ub = lb + torch.tensor(SPANS, dtype=torch.float32)[group]
    assert bool((ub > lb).all())
    pop = torch.maximum(torch.minimum(lb + torch.rand(N, d, generator=g) * (ub - lb), ub), lb)
    p0, p1 = torch.randint(0, N, (N,), generator=g), torch.randint(0, N, (N,), generator=g)
    kx, km = rnd.PRNGKey(100 + d), rnd.PRNGKey(200 + N)
    pro_c, pro_m = ((1.0, 1.0), (0.6, d / 2))[mode]
    y, counts = ref.variation_ref(pop, p0, p1, kx, km, lb, ub, pro_c, DIS_C, pro_m, DIS_M)
    off = SimulatedBinary(pro_c=pro_c, dis_c=DIS_C, type=2)(kx, torch.cat([pop[p0], pop[p1]], 0))
    t32 = torch.clamp(Polynomial((lb, ub), pro_m=pro_m, dis_m=DIS_M)(km, off), lb, ub)
    return dict(pop=pop, p0=p0.int(), p1=p1.int(), kx=kx, km=km, lb=lb, ub=ub, pro_c=pro_c, pro_m=pro_m, ref=y, t32=t32, counts=counts,
                group=group)


def _variation(c, **kw):
    return mo_ops.moead_variation(_dev(c["pop"]), _dev(c["p0"]), _dev(c["p1"]), _dev(c["kx"]), _dev(c["km"]), _dev(c["lb"]), _dev(c["ub"]),
                                  c["pro_c"], DIS_C, c["pro_m"], DIS_M, **kw)


def _rule(what, out, t32, ref64):
    """e_k <= 4·e_t + 2 ulp32(max |ref|), see the module docstring."""
    assert out.dtype == torch.float32 and t32.dtype == torch.float32 and ref64.dtype == torch.float64
    assert out.shape == ref64.shape and t32.shape == ref64.shape, (what, out.shape, t32.shape, ref64.shape)
    assert torch.isfinite(out).all(), what
    e_k = float((out.double() - ref64).abs().max())
    e_t = float((t32.double() - ref64).abs().max())
    floor = 2.0 * float(ref.ulp32(ref64.abs().max().reshape(1)))
    print(f"[rule] {what}: e_k {e_k:.3e} e_t {e_t:.3e} e_k/e_t {e_k / e_t if e_t > 0 else float('inf'):.3f} floor {floor:.3e} "
          f"e_k/bound {e_k / (4.0 * e_t + floor):.3f}")
    assert e_k <= 4.0 * e_t + floor, f"{what}: e_k {e_k:.3e} > 4·e_t + floor = {4.0 * e_t + floor:.3e} (e_t {e_t:.3e})"


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [1, 2, 101])
@pytest.mark.parametrize("d", [4, 64, 1000, 1, 37, 1003])
def test_variation_accuracy(d, N, mode):
    c = _var_case(N, d, mode)
    n = c["counts"]
    print(f"[variation] d {d} N {N} mode {mode}: {n}")
    if N == 101:
        assert n["pm_lo"] > 0 and n["pm_hi"] > 0, n
        if mode == 1:
            assert 0 < n["no_x"] < N, n
    out = _variation(c).cpu()
    assert out.shape == (N, d)
    assert bool((out >= c["lb"]).all() and (out <= c["ub"]).all())
    for gi, span in enumerate(SPANS):
        cols = c["group"] == gi
        if bool(cols.any()):
            _rule(f"variation d={d} N={N} mode={mode} span={span:g}", out[:, cols], c["t32"][:, cols], c["ref"][:, cols])


@pytest.mark.parametrize("d", [64, 37])
def test_variation_row_slices_winners_and_out_are_bit_identical(d):
    """``row0``/``rows``, the SELECT instantiation (``win``) and ``out=`` against the rows of the full launch."""
    N = 101
    c = _var_case(N, d, 1)
    full = _variation(c)
    for row0, rows in ((0, 1), (3, 1), (N - 2, 2), (50, 51)):
        part = _variation(c, row0=row0, rows=rows)
        assert part.shape == (rows, d) and torch.equal(part, full[row0 : row0 + rows]), (row0, rows)
    win = torch.randint(0, N, (N,), generator=_gen(3, d))
    win[::3] = -1
    win[1], win[2], win[4], win[5], win[7] = 0, N - 1, 17, 17, 17
    assert {-1, 0, N - 1} <= set(win.tolist())
    sel = _variation(c, win=_dev(win))
    pop = _dev(c["pop"])
    want = torch.where((_dev(win) >= 0)[:, None], full[_dev(win).clamp_min(0)], pop)
    assert torch.equal(sel, want)
    buf = torch.full((N + 3, d), -7.0, device=DEV)
    got = _variation(c, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:N], full) and bool((buf[N:] == -7.0).all())
    buf2 = torch.full((4, d), -7.0, device=DEV)
    _variation(c, row0=N - 2, rows=2, out=buf2)
    assert torch.equal(buf2[:2], full[N - 2 :]) and bool((buf2[2:] == -7.0).all())


# ---------------------------------------------------------------- replace
R_OFF = 1200
LENS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1100)
N_SLOTS = 73  # 6 × LENS + one more row of 513: not a multiple of the 4 slots of a workgroup
# seed per (M, func) where the default seed (M) leaves a decision inside the 64-ulp margin; chosen on the CPU
SEEDS = {}


def _csr(lens, g, r_off=R_OFF):
    """CSR built directly: row s holds ``lens[s]`` distinct offspring, ascending."""
    rows = [torch.sort(torch.randperm(r_off, generator=g)[:n]).values for n in lens]
    rowptr = torch.zeros(len(lens) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    return rowptr, torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64)


def _inputs(lens, M, g):
    N = len(lens)
    rowptr, owner = _csr(lens, g)
    W = torch.rand(N, M, generator=g) + 0.05
    off = torch.rand(R_OFF, M, generator=g)
    z = torch.full((M,), -0.01)
    zmax = 1.1 + 0.1 * torch.rand(M, generator=g)
    return rowptr, owner, W, off, z, zmax


def _occupants(rowptr, owner, W, off, z, zmax, func, g):
    """Occupants drawn so that about half of the slots replace: the slot's best candidate scaled by 1.05 or 0.95
    (a random row for a slot without candidates)."""
    N, M = W.shape
    best = ref.replace_ref(torch.full((N, M), 1e6), off, W, z, zmax, rowptr, owner, func)[0]
    coin = torch.rand(N, generator=g) < 0.5
    scale = torch.where(coin, torch.tensor(1.05), torch.tensor(0.95))[:, None]
    return torch.where((best >= 0)[:, None], off[best.clamp_min(0)] * scale, torch.rand(N, M, generator=g))


@functools.lru_cache(maxsize=None)
def _replace_case(M, func, n_slots=N_SLOTS):
    g = _gen(4, SEEDS.get((M, func, n_slots), M), n_slots)
    lens = (LENS * 6 + (513,))[:n_slots] if n_slots > 1 else (513,)
    rowptr, owner, W, off, z, zmax = _inputs(lens, M, g)
    pop_obj = _occupants(rowptr, owner, W, off, z, zmax, func, g)
    win, new_obj, info = ref.replace_ref(pop_obj, off, W, z, zmax, rowptr, owner, func)
    return dict(pop_obj=pop_obj, off=off, W=W, z=z, zmax=zmax, rowptr=rowptr, owner=owner, win=win, new_obj=new_obj, info=info)


def _replace(c, func, pop_obj=None, off=None):
    win, new_obj = mo_ops.moead_replace(_dev(c["pop_obj"] if pop_obj is None else pop_obj), _dev(c["off"] if off is None else off),
                                        _dev(c["W"]), _dev(c["z"]), _dev(c["zmax"]), _i32(c["rowptr"]), _i32(c["owner"]), func)
    assert win.dtype == torch.int32
    return win.cpu().long(), new_obj.cpu()


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 16])
def test_replace(M, func):
    c = _replace_case(M, func)
    info = c["info"]
    print(f"[replace] M {M} {func}: {info}")
    assert c["pop_obj"].shape[0] % 4 != 0
    assert info["margin"] >= 64 and info["ties_occupant"] == 0, info
    assert 0.2 <= info["replaced"] <= 0.8, info
    win, new_obj = _replace(c, func)
    assert torch.equal(win, c["win"])
    assert torch.equal(new_obj, c["new_obj"])


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [3, 4])
def test_replace_single_slot(M, func):
    c = _replace_case(M, func, 1)
    assert c["info"]["margin"] >= 64 and c["info"]["ties_occupant"] == 0, c["info"]
    for pop_obj in (c["pop_obj"], c["pop_obj"] * 0.5, c["pop_obj"] * 2.0):  # kept and replaced, whatever the coin
        w, n, info = ref.replace_ref(pop_obj, c["off"], c["W"], c["z"], c["zmax"], c["rowptr"], c["owner"], func)
        assert info["margin"] >= 64, info
        win, new_obj = _replace(c, func, pop_obj=pop_obj)
        assert torch.equal(win, w) and torch.equal(new_obj, n)


def _star(z, M, g, scale):
    """A row that beats every offspring drawn from [0, 1)^M under all five aggregations: z + scale·r, r in (0.5, 1)."""
    return z + scale * (0.5 + 0.5 * torch.rand(M, generator=g))


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [3, 5])
def test_replace_ties(M, func):
    """The minimal row stands at several owners of a row: same lane in another chain (p, p + 64·3), another lane
    and chain, and another pass of the outer loop.  The lowest owner wins."""
    g = _gen(5, M)
    rowptr, owner, W, off, z, zmax = _inputs((513, 1100, 257, 65), M, g)
    star = _star(z, M, g, 1e-4)
    expect = []
    for s, positions in enumerate(((200, 7, 7 + 192, 7 + 192 + 5, 7 + 448), (1099, 600 + 64 * 3, 600, 1024 + 3), (256, 70), (64, 1))):
        b = int(rowptr[s])
        for p in positions:
            off[owner[b + p]] = star
        expect.append(int(owner[b + min(positions)]))
    pop_obj = torch.rand(4, M, generator=g)
    w, n, info = ref.replace_ref(pop_obj, off, W, z, zmax, rowptr, owner, func)
    # an owner of one row's copies may stand earlier in another row: the reference decides, and row 0 is as crafted
    assert w[0] == expect[0] and bool((w >= 0).all())
    assert info["margin"] >= 64, info
    c = dict(pop_obj=pop_obj, off=off, W=W, z=z, zmax=zmax, rowptr=rowptr, owner=owner)
    win, new_obj = _replace(c, func)
    assert torch.equal(win, w) and torch.equal(new_obj, n)


@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [3, 5])
def test_replace_minimum_at_last_position(M, func):
    """The minimum is the last entry of rows of 63, 64, 65, 255, 256, 257, 511, 512, 513 and 1100 candidates."""
    g = _gen(6, M)
    lens = (63, 64, 65, 255, 256, 257, 511, 512, 513, 1100)
    N = len(lens)
    # row s draws from the offspring below 1000 + 20·s and ends at offspring 1000 + 20·s: no row holds the last
    # owner of a later row, and row s's star is smaller than those of the rows before it
    rows = [torch.cat([torch.sort(torch.randperm(1000 + 20 * s, generator=g)[: n - 1]).values, torch.tensor([1000 + 20 * s])])
            for s, n in enumerate(lens)]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(lens), 0)
    owner = torch.cat(rows)
    W = torch.rand(N, M, generator=g) + 0.05
    off = torch.rand(R_OFF, M, generator=g)
    z, zmax = torch.full((M,), -0.01), 1.1 + 0.1 * torch.rand(M, generator=g)
    r = 0.5 + 0.5 * torch.rand(M, generator=g)
    for s in range(N):
        off[1000 + 20 * s] = z + 1e-4 * (N - s) * r
    pop_obj = torch.rand(N, M, generator=g)
    w, n, info = ref.replace_ref(pop_obj, off, W, z, zmax, rowptr, owner, func)
    assert w.tolist() == [1000 + 20 * s for s in range(N)]
    assert info["margin"] >= 64, info
    win, new_obj = _replace(dict(pop_obj=pop_obj, off=off, W=W, z=z, zmax=zmax, rowptr=rowptr, owner=owner), func)
    assert torch.equal(win, w) and torch.equal(new_obj, n)


@pytest.mark.parametrize("func", ["tchebycheff", "modified_tchebycheff", "tchebycheff_norm"])
@pytest.mark.parametrize("M", [3, 5])
def test_replace_best_equal_to_occupant(M, func):
    """An occupant bit-equal to the slot's best candidate stays (strict improvement only).  The Tchebycheff forms
    only: weighted sum and PBI are compiled with FMA contraction, so two evaluations of the same row need not round
    alike."""
    c = _replace_case(M, func)
    best = ref.replace_ref(torch.full_like(c["pop_obj"], 1e6), c["off"], c["W"], c["z"], c["zmax"], c["rowptr"], c["owner"], func)[0]
    tie = torch.arange(N_SLOTS) % 2 == 1
    pop_obj = torch.where((tie & (best >= 0))[:, None], c["off"][best.clamp_min(0)], c["pop_obj"])
    w, n, info = ref.replace_ref(pop_obj, c["off"], c["W"], c["z"], c["zmax"], c["rowptr"], c["owner"], func)
    assert info["ties_occupant"] == int((tie & (best >= 0)).sum()) >= 30 and info["margin"] >= 64, info
    assert bool((w[tie] == -1).all()) and bool((w[~tie] >= 0).any())
    win, new_obj = _replace(c, func, pop_obj=pop_obj)
    assert torch.equal(win, w) and torch.equal(new_obj, n)


def _poison(c, func, case):
    """The NaN and +inf cases: the offspring that wins the most slots gets one NaN objective, the runner-up becomes
    all +inf, and one replacing slot's occupant gets a NaN objective."""
    pop_obj, off = c["pop_obj"].clone(), c["off"].clone()
    M = off.shape[1]
    wins = torch.bincount(c["win"][c["win"] >= 0], minlength=R_OFF)
    top = torch.argsort(wins, descending=True, stable=True)
    assert wins[top[1]] >= 1
    slot = int((c["win"] >= 0).nonzero()[-1])
    if case in ("nan_offspring", "all"):
        off[top[0], M // 2] = float("nan")
    if case in ("inf_offspring", "all"):
        off[top[1]] = float("inf")
    if case in ("nan_occupant", "all"):
        pop_obj[slot, M - 1] = float("nan")
    w, n, info = ref.replace_ref(pop_obj, off, c["W"], c["z"], c["zmax"], c["rowptr"], c["owner"], func)
    assert info["margin"] >= 64, info
    if case in ("nan_offspring", "all"):
        assert not bool((w == top[0]).any())
    if case in ("inf_offspring", "all"):
        assert not bool((w == top[1]).any())
    if case in ("nan_occupant", "all"):
        assert w[slot] == -1
    return pop_obj, off, w, n


@pytest.mark.parametrize("case", ["nan_offspring", "nan_occupant", "inf_offspring", "all"])
@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [3, 5])
def test_replace_nan_and_inf_follow_the_sequential_scan(M, func, case):
    c = _replace_case(M, func)
    pop_obj, off, w, n = _poison(c, func, case)
    win, new_obj = _replace(c, func, pop_obj=pop_obj, off=off)
    assert torch.equal(win, w)
    assert _same(new_obj, n)


# ---------------------------------------------------------------- halo_replace
def _halo_replace(c, func, slots, pop_obj=None, off=None):
    obj = _dev(c["pop_obj"] if pop_obj is None else pop_obj).clone()
    win_h = torch.full((slots.numel(),), -5, dtype=torch.int32, device=DEV)
    mo_ops.moead_halo_replace(obj, _dev(c["off"] if off is None else off), _dev(c["W"]), _dev(c["z"]), _dev(c["zmax"]), _i32(c["rowptr"]),
                              _i32(c["owner"]), _i32(slots), func, win_h)
    return obj.cpu(), win_h.cpu().long()


@pytest.mark.parametrize("H", [0, 1, 5, 71])
@pytest.mark.parametrize("func", FUNCS)
@pytest.mark.parametrize("M", [2, 3, 5])
def test_halo_replace(M, func, H):
    """In place, on an unsorted strict subset of the slots: the reference's winners there, every other row untouched."""
    c = _replace_case(M, func)
    assert c["info"]["margin"] >= 64
    slots = torch.randperm(N_SLOTS, generator=_gen(7, M, H))[:H]
    if H > 1:
        assert H < N_SLOTS and not torch.equal(slots, torch.sort(slots).values)
    obj, win_h = _halo_replace(c, func, slots)
    assert torch.equal(win_h, c["win"][slots])
    want = c["pop_obj"].clone()
    want[slots] = c["new_obj"][slots]
    assert torch.equal(obj, want)
    if H == 71:
        assert bool((win_h >= 0).any()) and bool((win_h < 0).any())


@pytest.mark.parametrize("func", FUNCS)
def test_halo_replace_nan_and_inf(func):
    c = _replace_case(3, func)
    pop_obj, off, w, n = _poison(c, func, "all")
    slots = torch.randperm(N_SLOTS, generator=_gen(8))[:71]
    obj, win_h = _halo_replace(c, func, slots, pop_obj=pop_obj, off=off)
    want = pop_obj.clone()
    want[slots] = n[slots]
    assert torch.equal(win_h, w[slots]) and _same(obj, want)


# ---------------------------------------------------------------- select_rows / select_rows_
@pytest.mark.parametrize("d", [4, 1000, 5, 1003])
def test_select_rows(d):
    g = _gen(9, d)
    N, R = 37, 53
    pop, off = torch.rand(N, d, generator=g), torch.rand(R, d, generator=g) + 2
    win = torch.randint(0, R, (N,), generator=g)
    win[::4] = -1
    win[1], win[2], win[3], win[5] = 0, R - 1, 44, 44
    want = torch.where((win >= 0)[:, None], off[win.clamp_min(0)], pop)
    out = mo_ops.moead_select_rows(_dev(pop), _dev(off), _dev(win))
    assert torch.equal(out.cpu(), want)
    buf = _dev(pop).clone()
    ret = mo_ops.moead_select_rows_(buf, _dev(off), _dev(win))
    assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf.cpu(), want)
    assert torch.equal(buf.cpu()[win < 0], pop[win < 0])
    keep = torch.full((N,), -1)
    mo_ops.moead_select_rows_(buf, _dev(off), _dev(keep))
    assert torch.equal(buf.cpu(), want)


# ---------------------------------------------------------------- halo_gather
@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("layout", ["world1", "world3_one_buffer", "world3_rank_buffers"])
@pytest.mark.parametrize("d", [8, 1003])
def test_halo_gather(d, layout, dedup):
    """One process.  ``one_buffer``: the pointer table of ``_tell_owner`` without IPC (``data_ptr + offsets`` into one
    offspring buffer).  ``rank_buffers``: every rank's rows in an allocation of its own, the empty rank's pointer to
    a poison buffer.  Rank 1 of 3 is empty (starts[1] == starts[2])."""
    g = _gen(10, d)
    n_off, n_pop = 40, 50
    full = torch.rand(n_off, d, generator=g) + 2
    starts = [0, n_off] if layout == "world1" else [0, 17, 17, n_off]
    world = len(starts) - 1
    slots = torch.randperm(n_pop, generator=g)[:24]
    win_h = torch.randint(0, n_off, (24,), generator=g)
    win_h[::5] = -1
    # offspring 23 wins four halo slots; first and last offspring of ranks 0 and 2
    win_h[1], win_h[2], win_h[3], win_h[4] = 0, 16, 17, n_off - 1
    win_h[6], win_h[9], win_h[13], win_h[22] = 23, 23, 23, 23
    pop = torch.rand(n_pop, d, generator=g)
    full_d = _dev(full)
    if layout == "world3_rank_buffers":
        poison = torch.full((n_off, d), -7.0, device=DEV)
        bufs = [full_d[starts[q] : starts[q + 1]].clone() if starts[q + 1] > starts[q] else poison for q in range(world)]
        table = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=DEV)
    else:
        offsets = torch.tensor([4 * a * d for a in starts[:-1]], dtype=torch.int64, device=DEV)
        table = torch.full_like(offsets, full_d.data_ptr()) + offsets
    pop_d = _dev(pop)
    first = torch.full((n_off,), -3, dtype=torch.int32, device=DEV) if dedup else None
    mo_ops.moead_halo_gather(pop_d, _i32(slots), _i32(win_h), table, _i32(torch.tensor(starts)), first)
    want = pop.clone()
    want[slots[win_h >= 0]] = full[win_h[win_h >= 0]]
    assert torch.equal(pop_d.cpu(), want)
    if dedup:
        f = torch.full((n_off,), INT_MAX, dtype=torch.int64)
        for h in range(23, -1, -1):
            if win_h[h] >= 0:
                f[win_h[h]] = h
        assert f[23] == 6
        assert torch.equal(first.cpu().long(), f)
    # no halo slot: nothing is launched, nothing changes
    mo_ops.moead_halo_gather(pop_d, _i32(slots[:0]), _i32(win_h[:0]), table, _i32(torch.tensor(starts)), first)
    assert torch.equal(pop_d.cpu(), want)


# ---------------------------------------------------------------- moead_scan (mo_scan.hip)
SCAN_FUNCS = ["tchebycheff", "pbi", "weighted_sum", "modified_tchebycheff"]
SCAN_SEEDS = {(16, "pbi", 64, 64, False): 1}


@functools.lru_cache(maxsize=None)
def _scan_inputs(T, M, seed):
    g = _gen(11, T, M, seed)
    N, R = 64, 100
    objs = torch.rand(N, M, generator=g)
    off = torch.rand(R, M, generator=g) * 0.9 - 0.05  # reaches below z: the ideal point moves
    P = torch.stack([torch.randperm(N, generator=g)[:T] for _ in range(R)])
    W = torch.rand(N, M, generator=g) + 0.05
    z = objs.min(0).values - 0.01
    return objs, off, P, W, z


def _scan_gpu(objs, off, P, W, z, func, nr, update_z):
    owner, o, zz = mo_ops.moead_scan(_dev(objs), _dev(off), _dev(P), _dev(W), _dev(z), func, nr=nr, update_z=update_z)
    return owner.cpu(), o.cpu(), zz.cpu()


@pytest.mark.parametrize("update_z", [False, True])
@pytest.mark.parametrize("T,nr", [(1, 1), (64, 1), (64, 64)])
@pytest.mark.parametrize("func", SCAN_FUNCS)
@pytest.mark.parametrize("M", [2, 5, 16])
def test_moead_scan(M, func, T, nr, update_z):
    objs, off, P, W, z = _scan_inputs(T, M, SCAN_SEEDS.get((M, func, T, nr, update_z), 0))
    if func in ("tchebycheff", "modified_tchebycheff"):
        owner, o, zz = mo_ops.moead_scan(objs, off, P, W, z, func, nr=nr, update_z=update_z)  # float32 CPU oracle
    else:
        owner, o, zz, info = ref.scan_ref(objs, off, P, W, z, func, nr=nr, update_z=update_z)
        print(f"[scan] M {M} {func} T {T} nr {nr} update_z {update_z}: {info}")
        assert info["margin"] >= 64 and info["ties"] == 0, info
    assert bool((zz != z).any()) == update_z
    assert bool((owner >= 0).any())
    got = _scan_gpu(objs, off, P, W, z, func, nr, update_z)
    assert torch.equal(got[0], owner) and torch.equal(got[1], o) and torch.equal(got[2], zz)


@pytest.mark.parametrize("nr", [1, 64])
def test_moead_scan_equal_offspring_later_one_owns(nr):
    """Tchebycheff, two identical offspring rows one after the other: ``>=`` lets the later one take the slots."""
    objs, off, P, W, z = (t.clone() for t in _scan_inputs(64, 5, 0))
    off[40] = z + 1e-3  # better than every occupant
    off[41] = off[40]
    P[41] = P[40]
    off[42:] = 10.0  # nothing after them replaces anything
    owner, o, zz = mo_ops.moead_scan(objs, off, P, W, z, "tchebycheff", nr=nr, update_z=False)
    assert bool((owner == 41).any()) and not bool((owner == 40).any())
    got = _scan_gpu(objs, off, P, W, z, "tchebycheff", nr, False)
    assert torch.equal(got[0], owner) and torch.equal(got[1], o) and torch.equal(got[2], zz)


@pytest.mark.parametrize("update_z", [False, True])
@pytest.mark.parametrize("func", SCAN_FUNCS)
@pytest.mark.parametrize("M", [2, 5])
def test_moead_scan_nan_and_inf(M, func, update_z):
    """One offspring with one NaN objective, one all-+inf offspring, one occupant with a NaN objective, against the
    CPU oracle (float32, ``amax``, ``sum`` and ``minimum`` propagate the NaN): the NaN offspring takes nothing, the NaN
    occupant stays, and with ``update_z`` the ideal point is NaN from that offspring on."""
    objs, off, P, W, z = (t.clone() for t in _scan_inputs(64, M, 0))
    clean = mo_ops.moead_scan(objs, off, P, W, z, func, nr=64, update_z=False)[0]
    held = torch.bincount(clean[clean >= 0], minlength=off.shape[0])
    i_nan = int(held.argmax())
    i_inf = 0 if i_nan != 0 else 1  # takes a slot when it arrives on the clean input
    assert bool((mo_ops.moead_scan(objs, off[: i_inf + 1], P[: i_inf + 1], W, z, func, nr=64, update_z=False)[0] == i_inf).any())
    off[i_nan, M // 2] = float("nan")
    off[i_inf] = float("inf")
    slot = int((clean >= 0).nonzero()[0])
    objs[slot, 0] = float("nan")
    if func in ("tchebycheff", "modified_tchebycheff"):
        owner, o, zz = mo_ops.moead_scan(objs, off, P, W, z, func, nr=64, update_z=update_z)
    else:
        owner, o, zz, info = ref.scan_ref(objs, off, P, W, z, func, nr=64, update_z=update_z)
        assert info["margin"] >= 64, info
        cpu = mo_ops.moead_scan(objs, off, P, W, z, func, nr=64, update_z=update_z)
        assert torch.equal(cpu[0], owner) and _same(cpu[1], o) and _same(cpu[2], zz)
    assert bool(torch.isnan(zz).any()) == update_z
    assert not bool((owner == i_nan).any()) and not bool((owner == i_inf).any()) and owner[slot] == -1
    got = _scan_gpu(objs, off, P, W, z, func, 64, update_z)
    assert torch.equal(got[0], owner) and _same(got[1], o) and _same(got[2], zz)


# ---------------------------------------------------------------- binding checks (raised before any launch)
def test_row_count_above_grid_limit_is_refused():
    """One grid row per population row / halo slot: 65 536 rows must raise, not leave the output unwritten."""
    n = 65536
    pop, off = torch.zeros(n, 1, device=DEV), torch.ones(2, 1, device=DEV)
    win = torch.zeros(n, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="65535"):
        mo_ops.moead_select_rows(pop, off, win)
    with pytest.raises(RuntimeError, match="65535"):
        mo_ops.moead_select_rows_(pop, off, win)
    table = torch.tensor([off.data_ptr()], dtype=torch.int64, device=DEV)
    starts = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="65535"):
        mo_ops.moead_halo_gather(pop, torch.arange(n, dtype=torch.int32, device=DEV), win, table, starts)
    assert bool((pop == 0).all())


def test_halo_replace_checks_shapes_and_func():
    c = _replace_case(3, "pbi")
    N, M = c["pop_obj"].shape
    good = dict(obj=_dev(c["pop_obj"]).clone(), off=_dev(c["off"]), W=_dev(c["W"]), z=_dev(c["z"]), zmax=_dev(c["zmax"]), rowptr=_i32(c["rowptr"]),
                owner=_i32(c["owner"]), slots=_i32(torch.arange(5)), func=1, win_h=torch.full((5,), -5, dtype=torch.int32, device=DEV))
    bad = [
        dict(obj=torch.zeros(N, 0, device=DEV), off=torch.zeros(R_OFF, 0, device=DEV), W=torch.zeros(N, 0, device=DEV),
             z=torch.zeros(0, device=DEV), zmax=torch.zeros(0, device=DEV)),  # M = 0
        dict(W=good["W"][:-1].contiguous()),
        dict(W=torch.zeros(N, M + 1, device=DEV)),
        dict(z=torch.zeros(M + 1, device=DEV)),
        dict(zmax=torch.zeros(M - 1, device=DEV)),
        dict(rowptr=good["rowptr"][:-1].contiguous()),
        dict(off=torch.zeros(R_OFF, M + 1, device=DEV)),
        dict(func=5),
        dict(func=-1),
        dict(win_h=torch.zeros(4, dtype=torch.int32, device=DEV)),
    ]
    for change in bad:
        a = {**good, **change}
        with pytest.raises(RuntimeError):
            mo_ops.moead_halo_replace(a["obj"], a["off"], a["W"], a["z"], a["zmax"], a["rowptr"], a["owner"], a["slots"], a["func"], a["win_h"])
    assert torch.equal(good["obj"].cpu(), c["pop_obj"]) and bool((good["win_h"] == -5).all())
