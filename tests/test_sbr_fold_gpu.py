"""The device eigensolver's folded schedule and gemm_ks's skip / select words.

* Folded ≡ separate: :class:`DeviceSBR` runs slot j's control step inside slot j + 1's rank
  launch (``fold=True``, the default) or as the two launches it replaced (``fold=False``).  The
  arithmetic is the same code run by the same threads, so every output and every persistent
  word must be bit-identical, eagerly and when the folded solve is replayed from a hipGraph on
  fresh inputs (the control step of slot −1, now inside rank(0), resets the persistent words).
* gemm_ks's control words, whatever the order in which the kernel loads them and its operands
  (loading the operands first measured slower and is not in the tree, profiles/NOTES.md): a
  launch with ``skip = 0`` must equal the launch without a skip word, ``skip = 1`` must write
  nothing, and ``sel`` must pick the operands it names.
"""
import pytest
import torch

from evoxmi.ops import _ext, sbr_device
from evoxmi.ops.linalg import mm

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------ inputs (built once, never modified)
_INPUTS = {}


def _spd(n):
    """C = U diag(λ) Uᵀ with λ ∈ [0.5, 2], U, and U times a small rotation (all seeded, float64 → float32)."""
    if n not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + n)
        U = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))[0]
        lam = 0.5 + 1.5 * torch.rand(n, generator=g, dtype=torch.float64)
        C = (U * lam) @ U.T
        C = 0.5 * (C + C.T)
        # rotation generator of Frobenius norm ≈ 0.014·√n: κ ≈ 0.2 at n = 1000, inside the late schedule's undamped range,
        # and far enough from the eigenbasis that the solve takes several slots
        S = 1e-2 / n**0.5 * torch.randn(n, n, generator=g, dtype=torch.float64)
        R = torch.linalg.matrix_exp(S - S.T)
        _INPUTS[n] = tuple(t.float().to(DEV).contiguous() for t in (C, U @ R))
    return _INPUTS[n]


def _diag(n):
    d = torch.linspace(0.5, 2.0, n)[torch.randperm(n, generator=torch.Generator().manual_seed(n))]
    return torch.diag(d).to(DEV).contiguous(), torch.eye(n, device=DEV)


def _solver(n, level, fold, iters=None):
    """A fresh workspace on the ``level`` schedule (``iters``: that many full slots instead)."""
    if iters is None:
        sch = sbr_device.schedule(level, n)
    else:
        sch = sbr_device.Schedule(int(iters), None, None, sbr_device.DEVICE_CFG["ns_iters"], False)
    cfg = sbr_device.device_config(sch.ns_iters)
    return sbr_device.DeviceSBR(n, DEV, cfg, sch.iters, sch.lean_from, sch.xgate, sch.damp_from, sch.basis_x3, fold=fold)


_STATE = ("eig_stats", "hist", "ctrl", "st", "alpha", "theta")


def _snapshot(ws, out):
    d = {"w": out[0].clone(), "B": out[1].clone()}
    d.update({k: getattr(ws, k).clone() for k in _STATE})
    return d


def _solve_both(n, level, C, B, iters=None):
    res = []
    for fold in (False, True):
        ws = _solver(n, level, fold, iters)
        res.append(_snapshot(ws, ws.solve(C, B)))
    torch.cuda.synchronize()
    return res


def _assert_same(sep, fol):
    for k in sep:
        # bit for bit; NaN-free by construction (a NaN would also be a failure here)
        assert torch.equal(sep[k], fol[k]), (k, sep[k].flatten()[:8], fol[k].flatten()[:8])


# ------------------------------------------------------------------ 1. folded ≡ separate
@pytest.mark.parametrize("n", [64, 200])
def test_fold_equals_separate_converged_at_start(n):
    """(a) C diagonal, B_prev = I: converged at ctrl(−1), every slot skipped — the folded order
    still ranks in the stopped slots."""
    C, B = _diag(n)
    sep, fol = _solve_both(n, "warm", C, B)
    _assert_same(sep, fol)
    assert float(fol["eig_stats"][1]) == 0.0 and float(fol["eig_stats"][2]) == 0.0
    assert int(fol["st"][0]) == 1 and bool((fol["ctrl"].view(-1, sbr_device.CW)[:, 0] == 1).all())


@pytest.mark.parametrize("n,level", [(64, "late"), (64, "warm"), (200, "late"), (200, "warm"), (1000, "late")])
def test_fold_equals_separate_warm_started(n, level):
    """(b) a warm-started real solve on the late / warm schedules."""
    C, B = _spd(n)
    sep, fol = _solve_both(n, level, C, B)
    print(n, level, "eig_stats", fol["eig_stats"].tolist())
    _assert_same(sep, fol)
    assert float(fol["eig_stats"][1]) == 0.0, fol["eig_stats"]
    assert float(fol["eig_stats"][2]) >= 1.0


@pytest.mark.parametrize("n", [64, 200])
def test_fold_equals_separate_cold_started(n):
    """(c) the same C from B_prev = I on the cold schedule."""
    C, _ = _spd(n)
    sep, fol = _solve_both(n, "cold", C, torch.eye(n, device=DEV))
    print(n, "cold eig_stats", fol["eig_stats"].tolist())
    _assert_same(sep, fol)
    assert float(fol["eig_stats"][1]) == 0.0, fol["eig_stats"]


@pytest.mark.parametrize("n", [64, 200])
@pytest.mark.parametrize("iters", [0, 1])
def test_fold_equals_separate_short_schedules(n, iters):
    """(d) no slot at all (the single ctrl(−1) stays a launch of its own) and one slot."""
    C, B = _spd(n)
    sep, fol = _solve_both(n, None, C, B, iters=iters)
    _assert_same(sep, fol)
    assert float(fol["eig_stats"][2]) == float(iters)


def test_fold_equals_separate_matrix_smaller_than_half_a_block():
    """n = 8 with 32-blocks: the half-block shift (16) is reduced mod n, so odd slots rank into perm[0, n)."""
    n = 8
    C, B = _spd(n)
    sep, fol = _solve_both(n, "warm", C, B)
    _assert_same(sep, fol)
    assert bool(torch.isfinite(fol["B"]).all())
    ws = _solver(n, "warm", True)
    ws.perm.fill_(-1)
    ws.solve(C, B)
    assert sorted(ws.perm.tolist()) == list(range(n))


# ------------------------------------------------------------------ 2. replay ≡ eager
def test_folded_solve_replays_like_eager_on_fresh_inputs():
    n = 200
    C0, B0 = _spd(n)
    g = torch.Generator().manual_seed(7)
    mats = []
    for scale in (1e-2, 0.0, 1e-3):  # C0 itself and two perturbed matrices: solves of different lengths
        E = scale * torch.randn(n, n, generator=g)
        mats.append((C0 + (E + E.T).to(DEV)).contiguous())
    eager = _solver(n, "warm", True)
    ws = _solver(n, "warm", True)
    Cs, Bs = C0.clone(), B0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ws.solve(Cs, Bs)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = ws.solve(Cs, Bs)
    for C in mats:
        Cs.copy_(C)
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(ws, out)
        ref = _snapshot(eager, eager.solve(C, B0))
        torch.cuda.synchronize()
        _assert_same(ref, got)


# ------------------------------------------------------------------ 3. gemm_ks: skip and select words
_LAYOUTS = {"NN": (False, False), "NT": (False, True), "TN": (True, False)}


def _operands(M, N, K, ta, tb, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((K, M) if ta else (M, K), generator=g).to(DEV)
    A2 = torch.randn((K, M) if ta else (M, K), generator=g).to(DEV)
    B = torch.randn((N, K) if tb else (K, N), generator=g).to(DEV)
    return A, A2, B


@pytest.mark.parametrize("prec", [None, "x3"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("layout", ["NN", "NT", "TN"])
@pytest.mark.parametrize("shape", [(96, 96, 96), (200, 200, 1000)])
def test_gemm_ks_skip_and_sel_words(shape, layout, mode, prec):
    M, N, K = shape
    ta, tb = _LAYOUTS[layout]
    A, A2, B = _operands(M, N, K, ta, tb, seed=M + K + mode)
    nparts = int(_ext.ops().gemm_ks_grid(M, N, mode))
    word = lambda v: torch.full((1,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    fill = 7.0

    def run(a, alpha, out, skip=None, part=None, **kw):
        return mm(a, B, ta=ta, tb=tb, mode=mode, alpha=alpha, out=out, skip=skip, prec=prec,
                  stat_part=part if mode == 1 else None, **kw)

    def outs():
        return torch.full((M, N), fill, device=DEV), torch.full((4 * nparts,), fill, dtype=torch.float64, device=DEV)

    # the plain calls (no control word at all) on both operand sets
    ref, ref_part = outs()
    run(A, 1.0, ref, None, ref_part)
    ref2, ref2_part = outs()
    run(A2, -0.5, ref2, None, ref2_part)
    assert not torch.equal(ref, ref2)

    # skip = 0: bit-equal to the call without a skip word
    o, p = outs()
    run(A, 1.0, o, word(0), p)
    assert torch.equal(o, ref)
    if mode == 1:
        assert torch.equal(p, ref_part)
    # skip = 1: output and stats partials untouched
    o, p = outs()
    run(A, 1.0, o, word(1), p)
    assert bool((o == fill).all()) and bool((p == fill).all())

    # sel = 0 / 1 with A2, alpha2, C2 (under a skip word of 0, as the solver launches it)
    for sv, want, want_part in ((0, ref, ref_part), (1, ref2, ref2_part)):
        o, p = outs()
        o2, _ = outs()
        run(A, 1.0, o, word(0), p, sel=word(sv), A2=A2, alpha2=-0.5, C2=o2)
        hit, miss = (o2, o) if sv else (o, o2)
        assert torch.equal(hit, want), sv
        assert bool((miss == fill).all()), sv
        if mode == 1:
            assert torch.equal(p, want_part), sv
    # sel under skip = 1: nothing written to either output
    o, p = outs()
    o2, _ = outs()
    run(A, 1.0, o, word(1), p, sel=word(1), A2=A2, alpha2=-0.5, C2=o2)
    assert bool((o == fill).all()) and bool((o2 == fill).all()) and bool((p == fill).all())
