"""The eight CMA-ES tell kernels of ``csrc/kernels/cmaes.hip`` one by one, each against a float64
restatement of the reference tell (``es_variants/cma_es.py:162-198``) at the shapes where its code
takes another path.  Runs on an MI355X (marked gpu).

Inputs are drawn on the CPU from a seeded ``torch.Generator``; the ops are called through
``evoxmi.ops._ext.ops()``.

Bounds.  No bound below uses a number measured on a kernel: every one comes from the float64
reference and from the same formula evaluated with ordinary float32 torch ops on the CPU.

* Accumulated results (``_rule``): with ``e_t`` the largest deviation of the float32 torch
  evaluation from the float64 reference and ``e_k`` the kernel's, ``e_k <= 4·e_t + floor``.
  The 4 covers another summation order (64-lane tree, strided partials) and FMA contraction
  (``-ffp-contract=fast``), each of which can about double a rounding error; ``floor`` is two
  float32 ulps of the output's largest magnitude, so ``e_t = 0`` cannot empty the check.
* Copies, selections and single correctly rounded operations are compared bit for bit or within
  1–2 float32 ulps of the float64 value (``_assert_ulps``: |out − ref64| <= n·ulp32(ref64)).

``cma_delta_gemv``: the float4 path forms δ inline as ``(mean + cm·dm) − mean``; it rounds exactly
as the stored ``delta`` (same two operations), so ``y`` is held to the plain rule against
``M·delta`` with the kernel's own ``delta`` and no ``Σ|M_rc|·ulp(mean_c)`` term is added.

Observed on an MI355X (gfx950), largest over the cases of each test; the baseline for
later rewrites of these kernels:

==============================  ================  =========================
output                          worst e_k / e_t   worst ulp distance (bound)
==============================  ================  =========================
delta_gemv  mean_out                              0.50 (1)
delta_gemv  delta                                 exact
delta_gemv  y                   1.09
paths       ps                  1.48
paths       pc                  1.00              0.60 (1) where hσ = 0
paths       sigma               1.71
paths       a, hsig                               0.16 (2), exact
cov_pad     Cn                  1.00              Cp, Bp: exact
eig_out     B / D / BdivD                         exact / 0.50 (1) / 1.47 (2)
center_rows Y[:, :d] / column d                   1.96 (2) / 0.96 (2)
local_select, sym_pack/unpack                     exact
tell_sharded mean               1.19
tell_sharded ps                 1.11
tell_sharded pc                 1.00
tell_sharded sigma              3.69
tell_sharded C                  1.00
==============================  ================  =========================

In every ``_rule`` check e_k stayed below 0.28 of its bound.  ``center_rows`` rounds four times
(sqrt, divide, subtract, multiply): 1.96 ulp on these seeded inputs is close to its bound, which a
rewrite that adds a rounding will cross.  In ``tell_sharded`` e_t is the unsharded ``tell``.
"""
import math

import pytest
import torch

from evoxmi.ops import _ext

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"


def _ops():
    return _ext.ops()


def _gen(*seed):
    s = 0
    for v in seed:
        s = s * 10007 + int(v) + 1
    return torch.Generator().manual_seed(s)


def _dev(*ts):
    out = tuple(t.to(DEV) for t in ts)
    return out if len(out) > 1 else out[0]


def _ulp32(ref64):
    """Spacing of float32 at |ref| (float64 tensor): 2^(e − 24) for |ref| = m·2^e, m in [0.5, 1)."""
    _, e = torch.frexp(ref64.abs().clamp_min(2.0**-126))
    return (((e.to(torch.int64) - 24).clamp_min(-149) + 1023) << 52).view(torch.float64)  # the exact power of two


def _assert_ulps(what, out, ref64, n):
    ref64 = ref64.to(out.device)
    assert out.dtype == torch.float32 and out.shape == ref64.shape, (what, out.dtype, out.shape, ref64.shape)
    assert torch.isfinite(out).all(), what
    dist = (out.double() - ref64).abs() / _ulp32(ref64)
    worst = float(dist.max()) if dist.numel() else 0.0
    print(f"[ulp] {what}: worst {worst:.3f} (bound {n})")
    assert worst <= n, f"{what}: {int((dist > n).sum())} elements further than {n} ulp from the float64 value, worst {worst:.3f}"


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


# ---------------------------------------------------------------- 1. cma_delta_gemv
@pytest.mark.parametrize("d", [1, 3, 4, 37, 256, 260, 1000, 1003])
def test_delta_gemv(d):
    """mean' = mean + cm·dm, δ = mean' − mean, y = M·δ.  The flagship's regime: |mean| ≈ 80 and
    |cm·dm| ≈ 0.1, so δ loses bits against the mean; M is not symmetric (a transposed read fails)."""
    g = _gen(1, d)
    cm = 0.75
    M = torch.randn(d, d, generator=g)
    mean = torch.rand(d, generator=g) * 160 - 80
    dm = torch.randn(d, generator=g) * (0.1 / cm)
    mean_out, delta, y = (t.cpu() for t in _ops().cma_delta_gemv(*_dev(M, mean, dm), cm))
    assert mean_out.shape == delta.shape == y.shape == (d,)
    _assert_ulps("delta_gemv.mean", mean_out, mean.double() + cm * dm.double(), 1)
    assert torch.equal(delta, mean_out - mean)
    _rule("delta_gemv.y", y, M @ delta, M.double() @ delta.double())


# ---------------------------------------------------------------- 2. cma_paths
CS, CC, MUEFF, DAMPS, C1, CMU = 0.5, 0.3, 4.0, 1.5, 0.01, 0.05


def _path_consts(d):
    chiN = d**0.5 * (1 - 1 / (4 * d) + 1 / (21 * d**2))
    return [CS, math.sqrt(CS * (2 - CS) * MUEFF), CC, math.sqrt(CC * (2 - CC) * MUEFF), chiN, DAMPS, C1, CMU, (1.4 + 2 / (d + 1)) * chiN]


def _paths_formula(ps, pc, y, delta, sigma, count, k, dtype):
    """Reference tell, paths and step size (cma_es.py:170-190), ``y = invsqrtC·δ`` given."""
    cs, c_ps, cc, c_pc, chiN, damps, c1, cmu, thresh = k
    ps, pc, y, delta, sigma = (t.to(dtype) for t in (ps, pc, y, delta, sigma))
    ps_n = (1 - cs) * ps + c_ps * y / sigma
    nrm = torch.linalg.norm(ps_n)
    ratio = nrm / torch.sqrt(1 - torch.tensor(1 - cs, dtype=dtype) ** (2 * count)) / thresh
    hs = (ratio < 1).to(dtype)
    pc_n = (1 - cc) * pc + hs * c_pc * delta / sigma
    a = (1 - c1 - cmu) + c1 * (1 - hs) * cc * (2 - cc)
    sig_n = sigma * torch.exp((cs / damps) * (nrm / chiN - 1))
    return ps_n, pc_n, sig_n.reshape(1), a.reshape(1), hs.reshape(1), float(ratio)


# (count_iter, count_eigen given): with count_eigen the kernel advances the counters and uses
# count_iter + 1.  ‖p_σ‖ is 0.92 of the threshold, so hσ = 0 up to a count of 1 and 1 from 2 on:
# count_iter = 1 decides differently in the two forms.
@pytest.mark.parametrize("count_iter,advance", [(0, True), (1, True), (49, True), (0, False), (1, False), (2, False), (50, False)])
@pytest.mark.parametrize("d", [1, 37, 1000, 1025, 4099])
def test_paths(d, count_iter, advance):
    g = _gen(2, d)
    k = _path_consts(d)
    sigma = torch.tensor([1.7])
    ps0, y0 = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
    v0 = (1 - CS) * ps0 + k[1] * y0 / sigma.double()
    s = 0.92 * k[8] / float(torch.linalg.norm(v0))
    ps, y = (ps0 * s).float(), (y0 * s).float()
    pc = torch.randn(d, generator=g)
    delta = torch.randn(d, generator=g) * 0.1 + 0.05  # not zero: a wrong hσ shows in p_c
    used = count_iter + 1 if advance else count_iter
    want_hs = 0.0 if used < 2 else 1.0

    ref = _paths_formula(ps, pc, y, delta, sigma, used, k, torch.float64)
    t32 = _paths_formula(ps, pc, y, delta, sigma, used, k, torch.float32)
    # the case is usable: the decision is at least 3 % from the threshold in both evaluations
    assert abs(ref[5] - 1) >= 0.03 and abs(t32[5] - 1) >= 0.03, (ref[5], t32[5])
    assert float(ref[4]) == want_hs and float(t32[4]) == want_hs

    ci = torch.tensor([count_iter], dtype=torch.int64)
    ce = torch.tensor([7], dtype=torch.int64)
    out = _ops().cma_paths(*_dev(ps, pc, y, delta, sigma, ci), k, _dev(ce) if advance else None)
    if advance:
        assert len(out) == 7
        assert out[5].dtype == torch.int64 and out[6].dtype == torch.int64
        assert out[5].cpu().tolist() == [count_iter + 1] and out[6].cpu().tolist() == [8]
    else:
        assert len(out) == 5
    ps_k, pc_k, sig_k, a_k, hs_k = (t.cpu() for t in out[:5])
    assert hs_k.tolist() == [want_hs]
    _assert_ulps("paths.a", a_k, ref[3], 2)
    _rule("paths.ps", ps_k, t32[0], ref[0])
    _rule("paths.pc", pc_k, t32[1], ref[1])
    _rule("paths.sigma", sig_k, t32[2], ref[2])
    if want_hs == 0.0:
        _assert_ulps("paths.pc(hsig=0)", pc_k, (1 - CC) * pc.double(), 1)


# ---------------------------------------------------------------- 3. cma_cov_pad
def _aug_ld(d):
    return (d + 1 + 3) // 4 * 4


# the last case has np − d >= 64: whole tile rows of padding
@pytest.mark.parametrize("d,np_", [(1, 32), (31, 32), (32, 32), (33, 64), (37, 64), (64, 64), (100, 128), (1000, 1024), (20, 96)])
def test_cov_pad(d, np_):
    """C' = a·C + c1·p_c p_cᵀ + cμ·S; Cp = (C' symmetrised from its upper half) ⊕ I; Bp = B_prev ⊕ I.
    C and S carry a deliberate asymmetry, so taking the lower half or averaging fails."""
    g = _gen(3, d, np_)
    c1, cmu = 0.01, 0.05
    sym = torch.randn(d, d, generator=g)
    C = sym + sym.T + 1e-3 * torch.randn(d, d, generator=g)
    sym = torch.randn(d, d, generator=g)
    S = sym + sym.T + 1e-3 * torch.randn(d, d, generator=g)
    assert d == 1 or (not torch.equal(C, C.T) and not torch.equal(S, S.T))
    pc = torch.randn(d, generator=g)
    a = torch.tensor([0.9412])
    Bprev = torch.randn(d, d, generator=g)
    ref = a.double() * C.double() + c1 * torch.outer(pc.double(), pc.double()) + cmu * S.double()
    t32 = a * C + c1 * torch.outer(pc, pc) + cmu * S

    Cd, pcd, ad, Bd = _dev(C, pc, a, Bprev)
    ld = _aug_ld(d)
    Sbuf0 = torch.randn(d + 1, ld, generator=g)
    Sbuf0[:d, :d] = S
    eye_pad = torch.eye(np_)
    base = None
    for strided in (False, True):
        Sbuf = _dev(Sbuf0.clone())
        Sd = Sbuf[:d, :d] if strided else _dev(S)
        assert Sd.stride(0) == (ld if strided else d) or d == 1
        for want_bp in (True, False):
            for out_kind in ("none", "fresh", "alias"):
                tag = f"strided={strided} want_bp={want_bp} Cn_out={out_kind}"
                Cin = Cd.clone()
                given = None if out_kind == "none" else (torch.full_like(Cd, float("nan")) if out_kind == "fresh" else Cin)
                Cn, Cp, Bp = _ops().cma_cov_pad(Cin, Sd, pcd, ad, c1, cmu, Bd, np_, given, want_bp)
                if given is not None:
                    assert Cn.data_ptr() == given.data_ptr(), tag
                if out_kind != "alias":
                    assert torch.equal(Cin, Cd), tag  # the input covariance is only read
                Cn, Cp, Bp = Cn.cpu(), Cp.cpu(), Bp.cpu()
                assert Cn.shape == (d, d) and Cp.shape == (np_, np_), tag
                if base is None:
                    base = (Cn, Cp)
                    _rule("cov_pad.Cn", Cn, t32, ref)
                    assert torch.equal(Cp[:d, :d], torch.triu(Cn) + torch.triu(Cn, 1).T)
                    assert torch.equal(Cp, Cp.T)
                    pad = Cp.clone()
                    pad[:d, :d] = torch.eye(d)
                    assert torch.equal(pad, eye_pad)
                else:  # aliased, preallocated and strided-S calls: the same bits as the first call
                    assert torch.equal(Cn, base[0]) and torch.equal(Cp, base[1]), tag
                if want_bp:
                    want = eye_pad.clone()
                    want[:d, :d] = Bprev
                    assert torch.equal(Bp, want), tag
                else:
                    assert Bp.numel() == 0, tag
        assert torch.equal(Sbuf.cpu(), Sbuf0)  # S and the buffer around the view are only read


# ---------------------------------------------------------------- 4. cma_eig_out
def _eig_w(n, d, g):
    w = torch.rand(n, generator=g) * 3 + 0.01
    for i, v in enumerate((0.0, -1.5, 1e-35)):  # clamped to 1e-30 (as many as fit in d)
        if i < d:
            w[(i * 7) % d if d > 14 else i] = v
    return w


def _check_eig_out(tag, out, src_block, w, d):
    B, D, BdivD = out
    assert B.shape == (d, d) and D.shape == (d,) and BdivD.shape == (d, d)
    assert torch.equal(B, src_block), tag
    D64 = torch.sqrt(torch.clamp(w[:d].double(), min=1e-30))
    assert torch.isfinite(D).all() and torch.isfinite(BdivD).all(), tag
    _assert_ulps(f"eig_out.D {tag}", D, D64, 1)
    _assert_ulps(f"eig_out.BdivD {tag}", BdivD, src_block.double() / D64, 2)


# (4100, 4128): more rows than the grid of 4096 workgroups, the grid-stride loop
@pytest.mark.parametrize("d,np_", [(1, 32), (37, 64), (1000, 1024), (96, 96), (4100, 4128)])
def test_eig_out(d, np_):
    g = _gen(4, d, np_)
    Bp = _dev(torch.randn(np_, np_, generator=g))
    w = _dev(_eig_w(np_, d, g))
    assert (w[:d] <= 0).any()
    _check_eig_out(f"d={d}", _ops().cma_eig_out(Bp, w, d), Bp[:d, :d], w, d)


@pytest.mark.parametrize("keep", [0, 1])
def test_eig_out_keep_word(keep):
    """While the keep word is 0 the basis is B_alt (row stride d), otherwise Bp's block (row stride np)."""
    d, np_ = 37, 64
    g = _gen(5, keep)
    Bp, Balt = _dev(torch.randn(np_, np_, generator=g), torch.randn(d, d, generator=g))
    w = _dev(_eig_w(np_, d, g))
    kw = torch.tensor([keep], dtype=torch.int32, device=DEV)
    out = _ops().cma_eig_out(Bp, w, d, None, Balt, kw)
    _check_eig_out(f"keep={keep}", out, Bp[:d, :d] if keep else Balt, w, d)
    assert out[0].data_ptr() != Balt.data_ptr()


# ---------------------------------------------------------------- 5. cma_center_rows
# (37, 5): scalar path, ld = 40; (1003, 64): d + 1 = ld; (1000, 120) and (4, 1): float4 path
@pytest.mark.parametrize("aug", [True, False])
@pytest.mark.parametrize("d,K", [(37, 5), (1003, 64), (1000, 120), (4, 1)])
def test_center_rows(d, K, aug):
    """Y[i] = (pop[rows[i]] − mean)·sqrt(wᵢ)/σ, with ``aug`` one more column σ·sqrt(wᵢ)."""
    g = _gen(6, d, K)
    N = K + 7
    sigma = torch.tensor([1.3])
    mean = torch.rand(d, generator=g) * 160 - 80
    pad4 = (4 - d % 4) % 4 + 4  # row stride d + pad4 is a multiple of 4, d + pad4 + 1 is not
    wsets = [torch.rand(K, generator=g) + 0.05]
    if K > 1:
        wsets[0][K // 2] = 0.0  # the sharded tell pads with zero weights
    else:
        wsets.append(torch.zeros(1))
    rows = torch.randint(0, N, (K,), generator=g, dtype=torch.int32)
    rows[0] = 0
    rows[-1] = rows[K // 2]  # a repeat
    for pad in (0, pad4, pad4 + 1):
        big = torch.cat([mean + 20.0 * torch.randn(N, d, generator=g), torch.randn(N, pad, generator=g)], 1)
        bigd = _dev(big)
        popd = bigd[:, :d]
        assert popd.stride(0) == d + pad
        for w in wsets:
            for use_rows in (True, False):
                tag = f"d={d} K={K} aug={aug} ldp={d + pad} rows={use_rows} w0={float(w[0]):.2f}"
                Y = _ops().cma_center_rows(popd, _dev(rows) if use_rows else None, _dev(mean), _dev(sigma), _dev(w), aug)
                assert torch.equal(bigd.cpu(), big), tag
                if aug:
                    assert Y.shape == (K, d + 1) and Y.stride(0) % 4 == 0 and Y.stride(1) == 1, tag
                else:
                    assert Y.shape == (K, d), tag
                Y = Y.cpu()
                sel = big[:, :d][rows.long()] if use_rows else big[:K, :d]
                sw = torch.sqrt(w.double())
                _assert_ulps(f"center_rows.Y {tag}", Y[:, :d].contiguous(), (sel.double() - mean.double()) * sw[:, None] / sigma.double(), 2)
                if aug:
                    _assert_ulps(f"center_rows.aug {tag}", Y[:, d].contiguous(), sigma.double() * sw, 2)
                assert (Y[w == 0] == 0).all(), tag


# ---------------------------------------------------------------- 6. cma_local_select
def _slices(n, world):
    q, r = divmod(n, world)
    out, start = [], 0
    for i in range(world):
        out.append((start, q + (1 if i < r else 0)))
        start += out[-1][1]
    return out


def _local_select_ref(order, mu, w, start, size):
    """The CPU branch of ``CMAES.tell_sharded`` (cma_es.py:541-548)."""
    K = min(mu, size)
    top = order[:mu].long()
    mine = (top >= start) & (top < start + size)
    lsel = torch.zeros(K, dtype=torch.int64)
    wsel = torch.zeros(K, dtype=torch.float32)
    n = int(mine.sum())
    lsel[:n] = top[mine] - start
    wsel[:n] = w[mine]
    return lsel.to(torch.int32), wsel, n


# μ = 1250 crosses one chunk of 1024; μ = 2050 takes three chunks, the last with 2 elements
@pytest.mark.parametrize("arange", [False, True])
@pytest.mark.parametrize("lam,mu,slices", [(10, 5, [(0, 5)]), (2500, 1250, _slices(2500, 3)), (4100, 2050, _slices(4100, 8)),
                                           (64, 32, _slices(64, 64))])
def test_local_select(lam, mu, slices, arange):
    g = _gen(7, lam, mu)
    order = torch.arange(lam, dtype=torch.int32) if arange else torch.randperm(lam, generator=g).to(torch.int32)
    w = torch.rand(mu, generator=g) + 0.01
    od, wd = _dev(order, w)
    total, full, empty = 0, 0, 0
    for start, size in slices:
        K = min(mu, size)
        rows = torch.full((K,), -7, dtype=torch.int32, device=DEV)
        wk = torch.full((K,), -1.0, device=DEV)
        _ops().cma_local_select(od, mu, wd, start, size, rows, wk)
        want_rows, want_w, n = _local_select_ref(order, mu, w, start, size)
        assert torch.equal(rows.cpu(), want_rows), (start, size)
        assert torch.equal(wk.cpu(), want_w), (start, size)
        got = int((wk > 0).sum())
        assert got == n
        total += got
        full += n == K == size
        empty += n == 0
    if len(slices) > 1 or slices[0][1] == lam:
        assert total == mu
    if arange and len(slices) > 1:  # the top μ lie in the leading slices: both extremes occur
        assert full > 0 and empty > 0


# ---------------------------------------------------------------- 7. sym_pack / sym_unpack
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("d", [1, 2, 37, 257, 1001])
def test_sym_pack_unpack(d, strided):
    g = _gen(8, d)
    P_len, tail = d * (d + 1) // 2, 5
    S0 = torch.randn(d, d, generator=g)  # not symmetric: only the upper triangle may be read
    wide0 = torch.randn(d + 2, d + 3, generator=g)
    wide0[:d, :d] = S0
    wide = _dev(wide0.clone())
    Sd = wide[:d, :d] if strided else _dev(S0)
    P = torch.full((P_len + tail,), -3.0, device=DEV)
    _ops().sym_pack(Sd, P)
    iu = torch.triu_indices(d, d)
    Pc = P.cpu()
    assert torch.equal(Pc[:P_len], S0[iu[0], iu[1]])
    assert torch.equal(Pc[P_len:], torch.full((tail,), -3.0))
    assert torch.equal(wide.cpu(), wide0)

    wide.fill_(float("nan"))
    Su = wide[:d, :d] if strided else torch.full((d, d), float("nan"), device=DEV)
    _ops().sym_unpack(P, Su)
    assert torch.equal(P.cpu(), Pc)
    got = Su.cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, torch.triu(S0) + torch.triu(S0, 1).T)
    outside = wide.cpu()
    outside[:d, :d] = float("nan")
    assert torch.isnan(outside).all()  # nothing outside the view is written


# ---------------------------------------------------------------- 8. the sharded tell in one process
class _OneProcessDist:
    """Rank ``rank`` of ``world`` for ``tell_sharded``, which uses only these two methods.  Pass 1
    (``total`` None) records a clone of the rank's buffer; pass 2 copies the ranks' sum in."""

    def __init__(self, rank, world, total=None):
        self.rank, self.world, self.total, self.recorded = rank, world, total, []

    def slice_of(self, n):
        return _slices(n, self.world)[self.rank]

    def all_reduce_(self, t, op=None):
        if self.total is None:
            self.recorded.append(t.clone())
        else:
            assert t.shape == self.total.shape
            t.copy_(self.total)
        return t


def _tell_f64(alg, st, pop, fit, count):
    """The reference tell (cma_es.py:162-198) in float64 on the CPU, B and D left out."""
    f = lambda t: t.detach().double().cpu()
    w, mean, sigma, ps, pc, C, W = f(alg.weights), f(st.mean), f(st.sigma), f(st.ps), f(st.pc), f(st.C), f(st.invsqrtC)
    d = alg.dim
    order = torch.argsort(f(fit), stable=True)[: alg.mu]
    diff = f(pop)[order] - mean
    y = diff / sigma
    S = (y.T * w) @ y
    mean_n = mean + alg.cm * (w @ diff)
    delta = mean_n - mean
    ps_n = (1 - alg.cs) * ps + math.sqrt(alg.cs * (2 - alg.cs) * alg.mueff) * (W @ delta) / sigma
    nrm = torch.linalg.norm(ps_n)
    ratio = float(nrm / math.sqrt(1 - (1 - alg.cs) ** (2 * count)) / ((1.4 + 2 / (d + 1)) * alg.chiN))
    hs = 1.0 if ratio < 1 else 0.0
    pc_n = (1 - alg.cc) * pc + hs * math.sqrt(alg.cc * (2 - alg.cc) * alg.mueff) * delta / sigma
    a = (1 - alg.c1 - alg.cmu) + alg.c1 * (1 - hs) * alg.cc * (2 - alg.cc)
    C_n = a * C + alg.c1 * torch.outer(pc_n, pc_n) + alg.cmu * S
    sigma_n = sigma * torch.exp((alg.cs / alg.damps) * (nrm / alg.chiN - 1))
    return {"mean": mean_n, "ps": ps_n, "pc": pc_n, "sigma": sigma_n, "C": C_n}, ratio


_TELL_FIELDS = ("mean", "ps", "pc", "sigma", "C")


# plain_gemm "evoxmi": the packed (d+1)(d+2)/2 augmented form; "blas": d(d+1)/2 + d;
# λ = 4200 on 8 ranks: μ = 2100 is more than two chunks of the selection kernel
@pytest.mark.parametrize("d,lam,world,plain", [(64, 512, 2, "evoxmi"), (64, 512, 3, "evoxmi"), (64, 512, 2, "blas"), (64, 512, 3, "blas"),
                                               (100, 4200, 8, "evoxmi")])
def test_tell_sharded_in_one_process(d, lam, world, plain):
    """Every rank of a W-rank ``tell_sharded`` on one device: the replicas agree bit for bit, and
    mean, p_σ, p_c, σ and C are as close to a float64 tell of the full population as the unsharded
    ``tell`` is (B and D are not compared: an eigenbasis is not continuous in C)."""
    from evoxmi import config
    from evoxmi import random as rnd
    from evoxmi.algorithms import CMAES
    from evoxmi.problems.numerical import CEC2022TestSuit
    from evoxmi.workflows import StdWorkflow

    with config.override(plain_gemm=plain):
        alg = CMAES(torch.linspace(-3, 3, d, device=DEV), init_stdev=2.0, pop_size=lam)
        wf = StdWorkflow(alg, CEC2022TestSuit.create(1))
        st = wf.init(rnd.PRNGKey(5, device=DEV))
        for _ in range(2):  # two real generations: C, p_σ and p_c are not trivial
            st = wf.step(st)
        a0 = st.get_child_state("algorithm")
        # p_c is still exactly zero while hσ has been 0 in every generation so far (far from the
        # optimum ‖p_σ‖ is above the threshold): a seeded vector is added, so (1 − cc)·p_c and
        # c1·p_c p_cᵀ are checked on numbers
        a0 = a0.update(pc=a0.pc + 0.3 * torch.randn(d, generator=_gen(9, d)).to(DEV))
        pop, a1 = alg.ask(a0)
        pop = pop.clone()
        fit = wf.problem.evaluate(None, pop)[0].reshape(lam).contiguous()
        count = int(a1.count_iter) + (1 if alg._counts_in_tell(a1) else 0)
        ref, ratio = _tell_f64(alg, a1, pop, fit, count)
        print(f"[state] d={d} lam={lam} W={world} {plain}: count {count} hsig ratio {ratio:.4f} |ps| {float(a1.ps.norm()):.3f}")
        # hσ is decided away from its threshold: float32 moves ‖p_σ‖ by about 1e-6 of itself, 1 % is 10⁴ times that
        assert abs(ratio - 1) >= 0.01, ratio
        whole = alg.tell(a1.update(population=pop), fit)

        def run(total):
            dists, outs = [], []
            for r in range(world):
                dist = _OneProcessDist(r, world, total)
                start, size = dist.slice_of(lam)
                outs.append(alg.tell_sharded(a1.update(population=pop[start:start + size].contiguous()), fit, dist))
                assert len(dist.recorded) == (1 if total is None else 0)
                dists.append(dist)
            return dists, outs

        dists, _ = run(None)
        total = dists[0].recorded[0].clone()
        for dist in dists[1:]:
            total += dist.recorded[0]
        form = (d + 1) * (d + 2) // 2 if plain == "evoxmi" else d * (d + 1) // 2 + d
        assert total.numel() == form
        _, outs = run(total)
        for k in _TELL_FIELDS:
            for o in outs[1:]:
                assert torch.equal(o[k], outs[0][k]), k  # the replicas agree bit for bit
            shape = ref[k].shape
            _rule(f"tell_sharded.{k} W={world} {plain}", outs[0][k].reshape(shape), whole[k].reshape(shape), ref[k])
