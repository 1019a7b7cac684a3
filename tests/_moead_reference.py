"""Host references of the MOEA/D generation kernels (``csrc/kernels/moead.hip``, ``mo_scan.hip``), shared by
test_moead_reference.py and test_moead_kernels_gpu.py.  Torch on the CPU, no device code.

Decisions that the kernels take on exactly representable float32 values are taken on the same float32 values here:
the uniforms ``u24`` of the Philox words, ``u24 < pro_m / d`` (with ``pro_m / d`` formed in float32), ``u24 > pro_c``
and ``μ <= 0.5``.  Everything after those decisions is float64 on the float32 inputs.  The word streams are drawn with
``rnd.split`` / ``rnd.bits`` exactly as the CPU operators draw them; nothing else of the code under test is imported.

``replace_ref`` and ``scan_ref`` also return how far their input is from a decision that float32 rounding could turn
(``margin``, in float32 ulps of the larger of the two compared magnitudes), so a test can require an input on which
the float32 kernels must take every decision as float64 does.
"""
import math

import torch

from evoxmi.ops import random as rnd

INT_MAX = 2**31 - 1
FUNCS = {"tchebycheff": 0, "pbi": 1, "weighted_sum": 2, "modified_tchebycheff": 3, "tchebycheff_norm": 4}


def ulp32(x64):
    """Spacing of float32 at |x| (float64 tensor): 2^(e − 24) for |x| = m·2^e, m in [0.5, 1)."""
    _, e = torch.frexp(x64.abs().clamp(2.0**-126, 2.0**127))
    return (((e.to(torch.int64) - 24).clamp_min(-149) + 1023) << 52).view(torch.float64)


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


# ---------------------------------------------------------------- parents
def parents_ref(nb, key, row0=0, rows=0):
    """(p0, p1) int64: the first two entries of a random permutation of every neighbour row,
    ``argsort(uniform(key, (N, T)), stable=True)[:, :2]`` gathered from ``nb``; T = 1 gives the one entry twice.
    ``rows > 0``: rows outside [row0, row0 + rows) are zero."""
    N, T = nb.shape
    perm = torch.argsort(rnd.uniform(key, (N, T)), dim=1, stable=True)
    j0, j1 = perm[:, 0], perm[:, 1 if T > 1 else 0]
    nb = nb.to(torch.int64)
    p0, p1 = nb.gather(1, j0[:, None])[:, 0], nb.gather(1, j1[:, None])[:, 0]
    if rows > 0:
        keep = (torch.arange(N) >= row0) & (torch.arange(N) < row0 + rows)
        p0, p1 = torch.where(keep, p0, torch.zeros_like(p0)), torch.where(keep, p1, torch.zeros_like(p1))
    return p0, p1


# ---------------------------------------------------------------- variation
def variation_ref(pop, p0, p1, key_x, key_m, lb, ub, pro_c, dis_c, pro_m, dis_m):
    """clip(PM(SBX_type2(pop[p0], pop[p1]))) in float64.  Returns (offspring float64 (n, d), counts) with counts =
    dict(pm_lo: PM sites with μ <= 0.5, pm_hi: PM sites with μ > 0.5, no_x: rows without crossover)."""
    n, d = p0.numel(), pop.shape[1]
    nm = n if n == 1 else (n // 2) * 2
    lo, hi = lb.to(torch.float32).expand(d).double(), ub.to(torch.float32).expand(d).double()
    gene_key, pair_key = rnd.split(key_x, 2)
    w = rnd.bits(gene_key, (n, d))
    mu32 = rnd._u24(w)
    no_x = rnd._u24(rnd.bits(pair_key, (n, 1))) > _f32(pro_c)
    mu = mu32.double()
    e = 1.0 / (dis_c + 1.0)
    beta = torch.where(mu32 <= 0.5, (2.0 * mu) ** e, (2.0 - 2.0 * mu) ** (-e))
    beta = torch.where((w & 1) == 1, -beta, beta)
    beta = torch.where(((w >> 1) & 1) == 1, torch.ones_like(beta), beta)
    beta = torch.where(no_x.expand(n, d), torch.ones_like(beta), beta)
    a, b = pop[p0.long()].double(), pop[p1.long()].double()
    y = 0.5 * (a + b) + beta * (0.5 * (a - b))
    # polynomial mutation of rows < nm
    k_site, k_mu = rnd.split(key_m, 2)
    pr = _f32(pro_m) / _f32(d)
    site = rnd._u24(rnd.bits(k_site, (nm, d))) < pr
    m32 = rnd._u24(rnd.bits(k_mu, (nm, d)))
    m = m32.double()
    x = torch.maximum(torch.minimum(y[:nm], hi), lo)
    span = hi - lo
    e1, inv = dis_m + 1.0, 1.0 / (dis_m + 1.0)
    low = site & (m32 <= 0.5)
    high = site & (m32 > 0.5)
    x_lo = x + span * ((2.0 * m + (1.0 - 2.0 * m) * (1.0 - (x - lo) / span) ** e1) ** inv - 1.0)
    x_hi = x + span * (1.0 - (2.0 * (1.0 - m) + 2.0 * (m - 0.5) * (1.0 - (hi - x) / span) ** e1) ** inv)
    x = torch.where(low, x_lo, torch.where(high, x_hi, x))
    y = torch.cat([x, y[nm:]], 0)
    y = torch.maximum(torch.minimum(y, hi), lo)
    return y, dict(pm_lo=int(low.sum()), pm_hi=int(high.sum()), no_x=int(no_x.sum()))


# ---------------------------------------------------------------- aggregation
def agg_ref(func, f, w, z, zmax=None):
    """Aggregate of the rows of ``f`` (K, M) for weights ``w`` ((M,) or (K, M)), float64.  A NaN term makes the
    aggregate NaN (``amax`` and ``sum`` propagate it)."""
    if func == 2:
        return (f * w).sum(-1)
    if func == 1:
        nw = torch.sqrt((w * w).sum(-1, keepdim=True))
        d1 = ((f - z) * w).sum(-1, keepdim=True) / nw
        d2 = torch.sqrt(((f - z - d1 * w / nw) ** 2).sum(-1))
        return d1[..., 0] + 5.0 * d2
    a = (f - z).abs()
    if func == 3:
        v = a / w
    elif func == 4:
        v = a / (zmax - z) * w
    else:
        v = a * w
    return v.amax(-1)


def _gap_ulps(a, b):
    """|a − b| in float32 ulps of the larger magnitude; inf where exactly one side is infinite, and for a == b
    (callers ask for distinct values only)."""
    if a == b:
        return math.inf
    if math.isinf(a) or math.isinf(b):
        return math.inf
    big = torch.tensor([max(abs(a), abs(b))], dtype=torch.float64)
    return abs(a - b) / float(ulp32(big))


# ---------------------------------------------------------------- replacement
def replace_ref(pop_obj, off_obj, W, z, zmax, rowptr, owner, func):
    """Per slot, in float64 on the float32 inputs: the first strict minimiser of the aggregate over the slot's CSR
    row (the lowest owner on equal values), taken only on strict improvement over the occupant.  As in the sequential
    scan (``f_old > f_new`` is false when either side is NaN) a candidate with a NaN aggregate never takes the slot
    and an occupant with a NaN aggregate stays.

    Returns (win int64 (N,), new_obj float32 (N, M), info) with info = dict(margin, ties_occupant, replaced):
    ``margin`` is the smallest gap, over the slots, of best against occupant and of best against the second-best
    distinct value, in float32 ulps of the larger magnitude; ``ties_occupant`` counts the slots whose best candidate
    equals the occupant exactly; ``replaced`` is the share of slots that take an offspring."""
    fid = FUNCS[func] if isinstance(func, str) else int(func)
    N, M = pop_obj.shape
    po, oo, Wd, zd, zm = (t.to(torch.float32).double() for t in (pop_obj, off_obj, W, z, zmax))
    rp, ow = rowptr.to(torch.int64).tolist(), owner.to(torch.int64)
    win = torch.full((N,), -1, dtype=torch.int64)
    margin, ties = math.inf, 0
    for s in range(N):
        cand = ow[rp[s] : rp[s + 1]]
        old = float(agg_ref(fid, po[s : s + 1], Wd[s], zd, zm)[0])
        if cand.numel() == 0:
            continue
        v = agg_ref(fid, oo[cand], Wd[s], zd, zm)
        ok = ~torch.isnan(v)
        if not bool(ok.any()):
            continue
        v, cand = v[ok], cand[ok]
        best = float(v.min())
        bi = int(cand[v == best].min())
        rest = v[v != best]
        if rest.numel():
            margin = min(margin, _gap_ulps(best, float(rest.min())))
        if math.isnan(old):
            continue
        if best == old:
            ties += 1
        else:
            margin = min(margin, _gap_ulps(best, old))
        if best < old:
            win[s] = bi
    new_obj = torch.where((win >= 0)[:, None], off_obj.to(torch.float32)[win.clamp_min(0)], pop_obj.to(torch.float32))
    return win, new_obj, dict(margin=margin, ties_occupant=ties, replaced=float((win >= 0).double().mean()) if N else 0.0)


# ---------------------------------------------------------------- sequential scan (MOEA/D-DRA, EAG-MOEA/D)
def scan_ref(objs, off_objs, P, W, z, func, nr=None, update_z=False):
    """The sequential ``moead_scan`` in float64: for i = 0..R−1 (optionally z ← min(z, f_i), NaN propagating as
    ``torch.minimum``), the slots P[i, t] with g(old) >= g(f_i) are taken by offspring i, at most ``nr`` (first in P
    order); every slot of a row is judged before any of them is written.

    Returns (owner int64 (N,), objs float32, z float32, info) with info = dict(margin, ties): the smallest non-zero
    |g_old − g_new| in float32 ulps of the larger magnitude, and the number of exact ties."""
    fid = FUNCS[func] if isinstance(func, str) else int(func)
    T = P.shape[1]
    nr = T if nr is None else int(nr)
    o32, f32 = objs.to(torch.float32).clone(), off_objs.to(torch.float32)
    o, Wd, zz = o32.double(), W.to(torch.float32).double(), z.to(torch.float32).double().clone()
    owner = torch.full((objs.shape[0],), -1, dtype=torch.int64)
    margin, ties = math.inf, 0
    for i in range(f32.shape[0]):
        fo = f32[i].double()
        if update_z:
            zz = torch.minimum(zz, fo)
        p = P[i].long()
        g_old = agg_ref(fid, o[p], Wd[p], zz)
        g_new = agg_ref(fid, fo[None].expand(len(p), -1), Wd[p], zz)
        fin = torch.isfinite(g_old) & torch.isfinite(g_new)
        gap = (g_old - g_new).abs()[fin]
        big = torch.maximum(g_old.abs(), g_new.abs())[fin]
        ties += int((gap == 0).sum())
        nz = gap > 0
        if bool(nz.any()):
            margin = min(margin, float((gap[nz] / ulp32(big[nz])).min()))
        sel = p[g_old >= g_new][:nr]
        o[sel] = fo
        o32[sel] = f32[i]
        owner[sel] = i
    return owner, o32, zz.to(torch.float32), dict(margin=margin, ties=ties)
