"""Non-dominated sort (``nds.hip``) and NSGA-II selection (``nsga_select.hip``) against
references that share no code with them.

References (plain numpy, nothing imported from ``evoxmi`` inside them)
    ``ref_rank``    builds the dominance matrix with IEEE comparisons on the float32 values
                    (``(a <= b).all(-1) & (a < b).any(-1)``) and takes the rank from the longest
                    chain of dominators: rows in ascending dominator count, ``rank[j] = 0``
                    without dominators, else ``1 + max(rank[dominators])``.  The kernel and the
                    project's CPU path both *peel* fronts; this does not.
    analytic inputs whose ranks are known by construction, for the sizes at which ``ref_rank``
                    is too slow: layers of anti-diagonals (rank = layer), a chain (rank = value),
                    identical rows (rank 0) and one objective with ties (rank = dense rank).
    ``ref_select``  the crowding distance on the rows of the cut front alone, per objective a
                    stable argsort of the −0 → +0 canonicalised cost, ends +inf, interior
                    ``(c[p+1] − c[p−1]) / (c[last] − c[0])`` in float32, summed in objective
                    order; survivors = rows of smaller rank in (rank, row) order, then the front
                    by stable argsort of −cd.  The kernel does the same single-rounded float32
                    operations in the same order, so every comparison below is exact.
The CPU tests (no ``gpu`` mark) validate the references: ``ref_rank`` against the analytic ranks
and against the project's CPU peel, ``ref_select`` against the CPU torch path
(``non_dominated_sort → crowding_distance → lexsort``) on finite inputs.

The +inf divergence
    The torch path keys masked-out rows +inf and sorts all n rows, so a cut-front row holding
    +inf ties with masked rows and "last valid" can be a masked row; ``ref_select`` and the kernel
    sort the front only.  ``test_torch_path_differs_with_inf_on_cut_front`` records that the two
    differ there (and only asserts that they do).  On finite inputs they are identical.

What the GPU groups pin (all through ``_ext.ops().nds`` / ``_ext.ops().nsga_select`` directly, so
no fall-back can hide a failure; the sticky device error word must be clean after every test)
    ``test_nds_edge_mix``       the generic ``dominance_kernel<0>`` at m = 1, 4, 8 and the m = 2, 3
                                instantiations; n either side of a 32-bit word, a 64-row peel
                                workgroup and a 256-thread dominance block; n < 256 (empty word
                                parts); ties, duplicates, ±0, ±inf and NaN objectives.
    ``test_nds_analytic``       deep fronts across 16-word resume chunks, a chain of n fronts,
                                a single front, n up to the binding's 65536 and just past
                                the sizes at which the default grid needs a second row pass.
    ``test_nds_until*``         the early stop, ``until`` on and off a front boundary and past n.
    ``test_nds_multipass``      the ``pass > 0`` row loop (forced with EVOXMI_NDS_BLOCKS=4 in a
                                child process), the "cannot be co-resident" error and the
                                wrapper's fall-back; ``test_nds_wrapper_m9`` the m > 8 fall-back.
    ``test_select_sizes``       cut-front sizes at the 1/2/4/8-items switches, F = 1, 2, 3,
                                lo = 0, hi = n, n not a multiple of 8, rows labelled n.
    ``test_select_kinds``       ties, duplicates, a constant objective (0/0), ±0 and ±inf on the front.
    ``test_nsga2_survivors_end_to_end``  both kernels together against both references.

Was the ``pass > 0`` loop reached without EVOXMI_NDS_BLOCKS?  The grid size is not returned to
Python, so it is read from the n = 65536 cases' behaviour.  With the grid sized by the occupancy
query alone (4 workgroups per CU, 1024 = 65536 / 64 on 256 CUs: a single pass) layered
(65536, K = 256) timed out at its first grid barrier on an MI355X: every rank came back n with
the error word set, after 92 s.  The kernel allocates 96 SGPRs, a band in which the hardware
admits 7 waves per SIMD, three 512-thread workgroups per CU, not the four the query answers.
``evx_nds_peel_blocks`` now caps the grid at 2 workgroups per CU, so on 256 CUs every n > 32768
takes two row passes by default, the n = 65536 cases here among them; below that only
``test_nds_multipass`` reaches the loop.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

INF = np.float32(np.inf)


# ---------------------------------------------------------------- references
def ref_rank(f):
    f = np.ascontiguousarray(f, dtype=np.float32)
    n = f.shape[0]
    dom_t = np.zeros((n, n), dtype=bool)  # dom_t[j, i]: i dominates j
    with np.errstate(invalid="ignore"):
        for i0 in range(0, n, 128):
            a = f[i0:i0 + 128, None, :]
            b = f[None, :, :]
            dom_t[:, i0:i0 + 128] = ((a <= b).all(-1) & (a < b).any(-1)).T
    count = dom_t.sum(1)
    rank = np.zeros(n, dtype=np.int64)
    for j in np.argsort(count, kind="stable"):
        d = dom_t[j]
        rank[j] = 1 + rank[d].max() if count[j] else 0
    return rank


def ref_select(f, rank, N, mask_pos):
    f = np.asarray(f, dtype=np.float32)
    rank = np.asarray(rank, dtype=np.int64)
    worst = np.sort(rank, kind="stable")[mask_pos]
    front = np.flatnonzero(rank == worst)
    F = front.shape[0]
    cd = np.zeros(F, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(f.shape[1]):
            c = f[front, k]
            c = np.where(c == 0, np.float32(0), c)
            o = np.argsort(c, kind="stable")
            s = c[o]
            d = np.empty(F, dtype=np.float32)
            d[1:-1] = (s[2:] - s[:-2]) / (s[-1] - s[0])
            d[0] = INF
            d[-1] = INF
            cd[o] = cd[o] + d
        key = -cd
        key = np.where(key == 0, np.float32(0), key)
    better = np.flatnonzero(rank < worst)
    better = better[np.argsort(rank[better], kind="stable")]
    return np.concatenate([better, front[np.argsort(key, kind="stable")]])[:N]


# ---------------------------------------------------------------- inputs
def edge_mix(n, m, seed, finite=False):
    f = np.random.default_rng(seed).random((n, m), dtype=np.float32)
    if n > 40:
        k = n // 5
        f[:k] = np.round(f[:k] * 4) / 4
        f[k + 1] = f[k + 3]
        f[k + 5] = -0.0
        f[k + 6] = 0.0
        if not finite:
            f[k + 8] = np.inf
            f[k + 10, m - 1] = -np.inf
            f[k + 12, 0] = np.nan
            f[k + 14, 0] = -np.inf
            f[k + 14, m - 1] = np.nan
    return f


def layered(K, P, seed):
    """K layers of P points (p + l, P − p + l): coordinate sums P + 2l share a parity, a
    dominance step adds at least 2 to the sum, and (p, ·) of layer l − 1 dominates (p, ·) of
    layer l, so the rank is l."""
    l, p = np.divmod(np.arange(K * P), P)
    perm = np.random.default_rng(seed).permutation(K * P)
    f = np.stack([p + l, P - p + l], 1).astype(np.float32)[perm]
    return f, l[perm].astype(np.int64)


def chain(n, seed):
    pi = np.random.default_rng(seed).permutation(n)
    return np.stack([pi, pi], 1).astype(np.float32), pi.astype(np.int64)


def identical(n):
    return np.tile(np.array([[0.25, -1.5, 3.0]], dtype=np.float32), (n, 1)), np.zeros(n, dtype=np.int64)


def one_objective(n, seed):
    v = np.random.default_rng(seed).integers(0, 97, n)
    return (v[:, None] * 0.5 - 7).astype(np.float32), np.unique(v, return_inverse=True)[1].astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_case(n, m, finite=False):
    f = edge_mix(n, m, 1000 * m + n, finite)
    r = ref_rank(f)
    f.setflags(write=False)
    r.setflags(write=False)
    return f, r


@functools.lru_cache(maxsize=None)
def analytic_case(kind, a, b=0):
    f, r = {"layered": lambda: layered(a, b, a + b), "chain": lambda: chain(a, a), "identical": lambda: identical(a),
            "m1": lambda: one_objective(a, a)}[kind]()
    f.setflags(write=False)
    r.setflags(write=False)
    return f, r


def simplex(n, m, rng):
    a = rng.random((n, m), dtype=np.float32) + np.float32(1e-3)
    return a / a.sum(1, keepdims=True)


KINDS = ["simplex", "quant8", "dup4", "const", "zeros", "inf"]


def select_case(lo, F, rest, m, kind, seed, rest_label_n=False):
    """Objectives and int32 layer labels of three layers of sizes [lo, F, rest] (simplex points
    + the layer number), rows permuted; `kind` shapes the objectives of the middle layer."""
    rng = np.random.default_rng(seed)
    n = lo + F + rest
    a = simplex(F, m, rng)
    if kind in ("quant8", "zeros"):
        a = np.round(a * 8) / 8
    if kind == "dup4":
        a = a[np.arange(F) % ((F + 3) // 4)]
    if kind == "const":
        a[:, 1] = 0.5
    if kind == "zeros":
        a[::3, 0] = -0.0
        a[1::3, 0] = 0.0
        a[::2, m - 1] = -0.0
    if kind == "inf":
        a[F // 3, 0] = np.inf
        a[(2 * F) // 3, m - 1] = -np.inf
    f = np.concatenate([simplex(lo, m, rng) - 1, a, simplex(rest, m, rng) + 1]).astype(np.float32)
    label = np.concatenate([np.zeros(lo), np.ones(F), np.full(rest, n if rest_label_n else 2)]).astype(np.int32)
    perm = rng.permutation(n)
    return f[perm], label[perm]


def cuts(lo, F, n):
    """(N, mask_pos) pairs: N at the start, the middle and the end of the cut front."""
    out = []
    for N in sorted({min(n, lo + 1), min(n, lo + (F + 1) // 2), min(n, lo + F)}):
        out += [(N, N - 1)] + ([(N, N)] if N < n else [])
    return out


# ---------------------------------------------------------------- CPU: the references
def test_ref_rank_matches_analytic_ranks():
    for f, r in (layered(64, 64, 1), chain(2000, 2), one_objective(1500, 3), identical(70)):
        assert np.array_equal(ref_rank(f), r)


@pytest.mark.parametrize("n,m", [(1, 1), (33, 1), (257, 2), (1000, 3), (300, 8)])
def test_ref_rank_matches_cpu_peel(n, m):
    from evoxmi.operators.selection import non_dominated_sort

    f, r = edge_case(n, m)
    assert np.array_equal(non_dominated_sort(torch.from_numpy(f.copy())).numpy(), r)


def _torch_path(f, N, mask_pos):
    from evoxmi.operators.selection.non_dominate import crowding_distance, lexsort, non_dominated_sort

    f = torch.from_numpy(np.array(f, dtype=np.float32))
    rank = non_dominated_sort(f)
    worst = torch.sort(rank).values[mask_pos]
    cd = crowding_distance(f, rank == worst)
    return lexsort([-cd, rank.to(cd.dtype)])[:N].numpy()


def _finite_select_inputs():
    rng = np.random.default_rng(7)
    yield "rand-ties", edge_mix(300, 3, 5, finite=True), 150
    yield "one-front", simplex(200, 3, rng), 100
    for kind in ("const", "dup4", "quant8", "zeros"):
        yield kind, select_case(40, 90, 60, 3, kind, 11)[0], 80
    for F in (2, 3):
        yield f"F={F}", select_case(5, F, 7, 2, "simplex", F)[0], 6


def test_ref_select_matches_torch_path_on_finite_inputs():
    for name, f, N in _finite_select_inputs():
        r = ref_rank(f)
        for mask_pos in (N - 1, N):
            assert np.array_equal(ref_select(f, r, N, mask_pos), _torch_path(f, N, mask_pos)), (name, mask_pos)


def test_torch_path_differs_with_inf_on_cut_front():
    """Three layers A, A+1, A+2 of 2-D simplex points, one middle-layer row set to (+inf, 1),
    the cut inside the middle layer.  The torch path keys the masked rows +inf as well, so its
    crowding distances on the cut front are not those of the front alone.  Whoever aligns the two
    paths turns this into an equality."""
    A = simplex(20, 2, np.random.default_rng(3))
    f = np.concatenate([A, A + 1, A + 2]).astype(np.float32)
    f[27] = (np.inf, 1.0)
    r = ref_rank(f)
    assert np.array_equal(r, np.repeat(np.arange(3), 20))
    assert not np.array_equal(ref_select(f, r, 30, 30), _torch_path(f, 30, 30))


# ---------------------------------------------------------------- GPU
@pytest.fixture
def ext():
    from evoxmi.ops import _ext

    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    yield _ext
    torch.cuda.synchronize()
    _ext.check_kernel_errors()


def _nds(ext, f, until=0):
    f = torch.from_numpy(np.array(f, dtype=np.float32)).cuda()
    return ext.ops().nds(f, until, ext.error_flag(f.device)).cpu().numpy()


def _check_until(out, ref, until):
    n = ref.shape[0]
    cut = np.sort(ref)[min(until, n) - 1]
    exact = ref <= cut
    assert np.array_equal(out[exact], ref[exact])
    assert (out[~exact] == n).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000])
def test_nds_edge_mix(ext, n, m):
    f, r = edge_case(n, m)
    assert np.array_equal(_nds(ext, f), r)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(4097, 3), (4096, 8)])
def test_nds_edge_mix_large(ext, n, m):
    f, r = edge_case(n, m)
    assert np.array_equal(_nds(ext, f), r)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("layered", 128, 64), ("layered", 256, 256), ("layered", 1, 65536), ("layered", 57, 576),
                                  ("layered", 64, 769), ("chain", 4096), ("identical", 5000), ("m1", 3000)],
                         ids=lambda c: "-".join(map(str, c)))
def test_nds_analytic(ext, case):
    """57 × 576 = 32832 rows are 64 past what 2 workgroups per CU cover in one pass on 256 CUs;
    64 × 769 = 49216 are 64 past what 3 per CU cover."""
    f, r = analytic_case(*case)
    assert np.array_equal(_nds(ext, f), r)


@pytest.mark.gpu
@pytest.mark.parametrize("until", [1, 64, 65, 128, 4095, 4096, 5000])
def test_nds_until_layered(ext, until):
    f, r = analytic_case("layered", 64, 64)
    _check_until(_nds(ext, f, until), r, until)


@pytest.mark.gpu
@pytest.mark.parametrize("until", [1, 500])
def test_nds_until_edge_mix(ext, until):
    f, r = edge_case(1000, 3)
    _check_until(_nds(ext, f, until), r, until)


_MULTIPASS_CHILD = """
import sys
import numpy as np
import torch
from evoxmi.ops import _ext, nds
inp = np.load(sys.argv[1])
out = {}
for name in inp.files:
    f = torch.from_numpy(inp[name]).cuda()
    if f.shape[0] == 1025:
        try:
            _ext.ops().nds(f, 0, _ext.error_flag(f.device))
        except RuntimeError as e:
            assert 'co-resident' in str(e), str(e)
            print('RAISED')
        out[name] = nds.non_dominated_sort(f).cpu().numpy()
        continue
    for until in (0, 300):
        out[f'{name}/{until}'] = _ext.ops().nds(f, until, _ext.error_flag(f.device)).cpu().numpy()
torch.cuda.synchronize()
_ext.check_kernel_errors()
np.savez(sys.argv[2], **out)
print('SAVED')
"""


@pytest.mark.gpu
def test_nds_multipass(tmp_path):
    """EVOXMI_NDS_BLOCKS=4 (read once per process, hence the child): 257 rows take two row
    passes, 1000 and 1024 four (the last one partial at 1000), 1025 cannot run."""
    cases = {"e257": edge_case(257, 3), "e1000": edge_case(1000, 3), "e1024": edge_case(1024, 3),
             "l1024": analytic_case("layered", 16, 64), "e1025": edge_case(1025, 3)}
    np.savez(tmp_path / "in.npz", **{k: v[0] for k, v in cases.items()})
    env = dict(os.environ, EVOXMI_NDS_BLOCKS="4")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _MULTIPASS_CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "RAISED" in p.stdout and "SAVED" in p.stdout
    out = np.load(tmp_path / "out.npz")
    for name, (_, r) in cases.items():
        if name == "e1025":
            assert np.array_equal(out[name], r), name
            continue
        assert np.array_equal(out[f"{name}/0"], r), name
        _check_until(out[f"{name}/300"], r, 300)


@pytest.mark.gpu
def test_nds_wrapper_m9(ext):
    from evoxmi.ops.nds import non_dominated_sort

    f, r = edge_case(300, 9)
    assert np.array_equal(non_dominated_sort(torch.from_numpy(f.copy()).cuda()).cpu().numpy(), r)


def _select(ext, f, label, N, mask_pos):
    return ext.ops().nsga_select(label, f, N, mask_pos).cpu().numpy()


_SIZES = [(lo, F, rest) for F in (1, 2, 3, 1023, 1024, 1025, 2048, 2049, 4096, 4097) for lo in (0, 5) for rest in (0, 7)] + [(0, 8192, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("lo,F,rest", _SIZES)
def test_select_sizes(ext, lo, F, rest):
    n = lo + F + rest
    i = _SIZES.index((lo, F, rest))
    for j in range(2):
        kind, m = KINDS[(i + 3 * j) % 6], (2, 3, 5)[(i + j) % 3]
        f, label = select_case(lo, F, rest, m, kind, 100 * i + j, rest_label_n=(lo + j) % 2 == 1)
        fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(label).cuda()
        for N, mask_pos in cuts(lo, F, n):
            assert np.array_equal(_select(ext, fd, ld, N, mask_pos), ref_select(f, label, N, mask_pos)), (kind, m, N, mask_pos)


@pytest.mark.gpu
def test_select_single_row(ext):
    f = np.array([[0.5, -0.0, np.inf]], dtype=np.float32)
    out = _select(ext, torch.from_numpy(f).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"), 1, 0)
    assert np.array_equal(out, [0])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3, 5])
@pytest.mark.parametrize("lo,F,rest", [(5, 41, 7), (0, 130, 3), (5, 3001, 7)])
@pytest.mark.parametrize("kind", KINDS)
def test_select_kinds(ext, kind, lo, F, rest, m):
    n = lo + F + rest
    f, label = select_case(lo, F, rest, m, kind, F + m, rest_label_n=m == 3)
    fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(label).cuda()
    for N, mask_pos in cuts(lo, F, n):
        assert np.array_equal(_select(ext, fd, ld, N, mask_pos), ref_select(f, label, N, mask_pos)), (N, mask_pos)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,N", [(600, 3, 300), (4097, 2, 2048)])
def test_nsga2_survivors_end_to_end(ext, n, m, N):
    from evoxmi.ops.nds import nsga2_survivors

    f, r = edge_case(n, m, True)
    out = nsga2_survivors(torch.from_numpy(f.copy()).cuda(), N, N, until=N + 1).cpu().numpy()
    assert np.array_equal(out, ref_select(f, r, N, N))
