"""``cma_small_ask`` / ``cma_small_tell`` (``csrc/kernels/cma_small.hip``) and ``CMAES(fused_small=True)`` against one
float64 restatement of ask and tell (plain torch, ``torch.linalg.eigh`` in float64).  Runs on an MI355X (marked gpu).

Inputs come from a seeded CPU generator.  Bounds follow ``tests/test_cmaes_kernels_gpu.py`` and none is a number
measured on the kernel: ``e_k <= 4·e_t + floor`` with ``e_t`` the float32 torch evaluation of the same formula on the CPU
against float64 (for the decomposition: float32 ``torch.linalg.eigh`` of the same Cs) and ``floor`` two float32 ulps of
the output's largest magnitude (1 for the orthogonality, whitening and relative residuals).

Observed on an MI355X (gfx950), largest e_k / e_t over the cases of each test:

==========================  ==================================================
output                      worst e_k / e_t
==========================  ==================================================
ask  x                      2.42
tell mean / ps / sigma      1.00 / 1.00 / 1.00
tell pc / C                 6.86 (d = 2) / 4.51 (d = 1), both inside the floor
tell |BᵀB − I|              1.09
tell residual / D² / white  1.54 / 2.27 / 1.00
==========================  ==================================================

In every check e_k stayed below 0.6 of its bound.  The solves took 1–5 sweeps and none was capped.
"""
import functools
import math

import pytest
import torch

from evoxmi import random as rnd
from evoxmi.algorithms import CMAES
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.ops import _ext
from evoxmi.problems.numerical import Sphere
from evoxmi.workflows import StdWorkflow

pytestmark = pytest.mark.gpu
DEV = "cuda"
TELL_CASES = [(1, None), (2, None), (5, None), (33, None), (64, None), (8, 1024)]


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"


def _rule(what, e_k, e_t, magnitude):
    floor = 2.0 * 2.0 ** (math.frexp(magnitude)[1] - 24)  # two float32 ulps at `magnitude`
    print(f"[rule] {what}: e_k {e_k:.3e} e_t {e_t:.3e} e_k/e_t {e_k / e_t if e_t > 0 else float('inf'):.3f} floor {floor:.3e}")
    assert math.isfinite(e_k) and e_k <= 4.0 * e_t + floor, f"{what}: e_k {e_k:.3e} > 4·e_t + floor (e_t {e_t:.3e}, floor {floor:.3e})"


def _rule_t(what, out, t32, ref64):
    out, ref64 = out.detach().cpu().double(), ref64.cpu()
    assert out.shape == ref64.shape, (what, out.shape, ref64.shape)
    _rule(what, float((out - ref64).abs().max()), float((t32.double() - ref64).abs().max()), float(ref64.abs().max()))


# ---------------------------------------------------------------- the restatement (dtype of its inputs: float64, or float32 for e_t)
def ask_ref(mean, sigma, B, D, z):
    return mean + sigma * (z * D) @ B.T


def tell_ref(a, s, pop, order, count):
    """mean, ps, pc, sigma, C of CMAES._finish_tell for the selected rows ``order``; ``s`` holds the state in one dtype."""
    w = a.weights.cpu().to(pop.dtype)
    diff = pop[order] - s["mean"]
    mean = s["mean"] + a.cm * (w @ diff)
    delta = mean - s["mean"]
    ps = (1 - a.cs) * s["ps"] + math.sqrt(a.cs * (2 - a.cs) * a.mueff) * (s["invsqrtC"] @ delta) / s["sigma"]
    hs = float(ps.norm() / math.sqrt(1 - (1 - a.cs) ** (2 * count)) < (1.4 + 2 / (a.dim + 1)) * a.chiN)
    pc = (1 - a.cc) * s["pc"] + hs * math.sqrt(a.cc * (2 - a.cc) * a.mueff) * delta / s["sigma"]
    y = diff / s["sigma"]
    C = (1 - a.c1 - a.cmu + a.c1 * (1 - hs) * a.cc * (2 - a.cc)) * s["C"] + a.c1 * torch.outer(pc, pc) + a.cmu * (y.T * w) @ y
    sigma = s["sigma"] * torch.exp((a.cs / a.damps) * (ps.norm() / a.chiN - 1))
    return dict(mean=mean, ps=ps, pc=pc, sigma=sigma, C=C)


def _orth(d, g):
    return torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64)).Q.contiguous()


# ---------------------------------------------------------------- ask
@pytest.mark.parametrize("d,lam", [(1, 4), (5, 37), (64, 1024)])
def test_ask_normal_stream(d, lam):
    keys = torch.stack([rnd.PRNGKey(s, device=DEV) for s in (3, 4, 5)])
    eye = torch.eye(d, device=DEV).expand(3, d, d).contiguous()
    x = _ext.ops().cma_small_ask(keys, torch.zeros(3, d, device=DEV), torch.ones(3, device=DEV), eye, torch.ones(3, d, device=DEV), lam)
    z = _ext.ops().philox_fill(keys, lam * d, 1, 0).reshape(3, lam, d)
    assert torch.equal(x, z) and not torch.equal(x[0], x[1])


@pytest.mark.parametrize("lam", [4, 37])
@pytest.mark.parametrize("d", [1, 2, 5, 33, 64])
def test_ask_product(d, lam):
    g = torch.Generator().manual_seed(100 * d + lam)
    key = rnd.PRNGKey(d + lam, device=DEV)
    B, D = _orth(d, g), torch.logspace(-3, 3, d, dtype=torch.float64) if d > 1 else torch.tensor([0.3], dtype=torch.float64)
    mean, sigma = 5 * torch.randn(d, generator=g, dtype=torch.float64), torch.tensor(0.7, dtype=torch.float64)
    f32 = [t.float() for t in (mean, sigma, B, D)]
    x = _ext.ops().cma_small_ask(key, *[t.to(DEV) for t in f32], lam)
    z = _ext.ops().philox_fill(key, lam * d, 1, 0).reshape(lam, d).cpu()
    _rule_t(f"ask d={d} lam={lam}", x, ask_ref(*f32, z), ask_ref(*[t.double() for t in f32], z.double()))


# ---------------------------------------------------------------- tell
@functools.lru_cache(maxsize=None)
def _tell_case(d, lam):
    """Inputs, the kernel's outputs (through CMAES.tell) and both references of one case, computed once."""
    g = torch.Generator().manual_seed(7 * d + (lam or 0))
    a = CMAES(torch.zeros(d, device=DEV), 1.0, pop_size=lam, fused_small=True)
    lam, mu = a.pop_size, a.mu
    Q = _orth(d, g)
    C = ((Q * torch.logspace(-2, 2, d, dtype=torch.float64)) @ Q.T).float() if d > 1 else torch.tensor([[2.5]])
    w, V = torch.linalg.eigh(C.double())
    s = dict(C=C, B=V.float(), D=w.sqrt().float(), invsqrtC=((V / w.sqrt()) @ V.T).float(), mean=3 * torch.randn(d, generator=g),
             sigma=torch.tensor(0.7), ps=torch.randn(d, generator=g), pc=torch.randn(d, generator=g))
    pop = s["mean"] + s["sigma"] * torch.randn(lam, d, generator=g)
    perm = torch.randperm(lam, generator=g)
    fit = perm.float()
    fit[perm == mu] = float(mu - 1)  # an exact tie straddling rank μ: the lower index is selected
    fit[perm == lam - 1] = float("nan")
    order = torch.sort(fit, stable=True).indices[:mu]
    st0 = a.setup(rnd.PRNGKey(0, device=DEV)).update(population=pop.to(DEV), count_iter=torch.tensor(3, device=DEV),
                                                     **{k: v.to(DEV) for k, v in s.items()})
    out = a.tell(st0, fit.to(DEV))
    ref = tell_ref(a, {k: v.double() for k, v in s.items()}, pop.double(), order, 3)
    t32 = tell_ref(a, s, pop, order, 3)
    return a, st0, fit, out, ref, t32


@pytest.mark.parametrize("d,lam", TELL_CASES)
def test_tell_update(d, lam):
    a, st0, fit, out, ref, t32 = _tell_case(d, lam)
    for name in ("mean", "ps", "pc", "sigma", "C"):
        _rule_t(f"tell d={d} {name}", out[name], t32[name], ref[name])


@pytest.mark.parametrize("d,lam", TELL_CASES)
def test_tell_decomposition(d, lam):
    a, st0, fit, out, ref, t32 = _tell_case(d, lam)
    I = torch.eye(d, dtype=torch.float64)
    Cn = out.C.cpu()
    Cs = (torch.triu(Cn) + torch.triu(Cn, 1).T).double()
    w64 = torch.linalg.eigvalsh(Cs)
    wt, Vt = torch.linalg.eigh(Cs.float())
    B, D2, isc = out.B.cpu().double(), out.D.cpu().double() ** 2, out.invsqrtC.cpu().double()
    it = ((Vt / wt.sqrt()) @ Vt.T).double()
    Vt, wt = Vt.double(), wt.double()
    fro = lambda M: float(torch.linalg.norm(M) / torch.linalg.norm(Cs))
    _rule(f"d={d} |BtB - I|", float((B.T @ B - I).abs().max()), float((Vt.T @ Vt - I).abs().max()), 1.0)
    _rule(f"d={d} residual", fro((B * D2) @ B.T - Cs), fro((Vt * wt) @ Vt.T - Cs), 1.0)
    _rule(f"d={d} D^2", float((D2.sort().values - w64).abs().max()), float((wt - w64).abs().max()), float(w64.max()))
    _rule(f"d={d} whitening", float((isc @ Cs @ isc - I).abs().max()), float((it @ Cs @ it - I).abs().max()), 1.0)
    stats = out.eig_stats.cpu()
    assert stats[3] == 0 and stats[1] >= 1 and int(out.count_eigen) == 1, stats
    again = a.tell(st0, fit.to(DEV))
    assert all(torch.equal(out[k], again[k]) for k in ("mean", "ps", "pc", "sigma", "C", "B", "D", "invsqrtC", "eig_stats"))
    a.decomp_per_iter = 2  # count_iter = 3 is odd: no decomposition this generation
    try:
        skip = a.tell(st0, fit.to(DEV))
    finally:
        a.decomp_per_iter = 1
    assert all(torch.equal(skip[k], st0[k]) for k in ("B", "D", "invsqrtC", "count_eigen"))
    assert torch.equal(skip.C, out.C) and not torch.equal(skip.C, st0.C)


# ---------------------------------------------------------------- the container and the public interface
def _algo():
    return CMAES(torch.full((10,), 3.0, device=DEV), 1.0, fused_small=True)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_runs_equal_solo(graph):
    def batched(graph):
        wf = StdWorkflow(BatchedRuns(_algo(), 3), Sphere(), graph=graph)
        st = wf.init(rnd.PRNGKey(7, device=DEV))
        keys = st.get_child_state("algorithm").runs.key.clone()
        for _ in range(6):
            st = wf.step(st)
        return keys, st.get_child_state("algorithm").runs

    keys, runs = batched(graph)
    for r in range(3):
        a = _algo()
        st = a.init(keys[r])  # keys[r] = split(key, 3)[r], the key BatchedRuns gave run r
        for _ in range(6):
            pop, st = a.ask(st)
            st = a.tell(st, Sphere().evaluate(None, pop)[0])
        for name, v in st._state_dict.items():
            assert torch.equal(runs[name][r], v), f"run {r}: {name} differs from the solo run"
    assert not torch.equal(runs.mean[0], runs.mean[1])
    if graph:
        eager = batched(False)[1]
        assert all(torch.equal(runs[name], v) for name, v in eager._state_dict.items())


def test_it_optimises():
    b = BatchedRuns(_algo(), 8)
    st = b.init(rnd.PRNGKey(7, device=DEV))
    for _ in range(150):
        pop, st = b.ask(st)
        st = b.tell(st, (pop * pop).sum(1))
    f = (st.runs.mean ** 2).sum(1)
    print("f(mean) of the 8 runs:", f.tolist(), "sweeps", st.runs.eig_stats[:, 1].tolist())
    assert bool((f <= 1e-4).all()) and bool((st.runs.eig_stats[:, 3] == 0).all())


def test_caps():
    with pytest.raises(ValueError):
        CMAES(torch.zeros(65, device=DEV), 1.0, fused_small=True)
    with pytest.raises(ValueError):
        CMAES(torch.zeros(8, device=DEV), 1.0, pop_size=1025, fused_small=True)
    from evoxmi.ops import batching

    batching.register()
    z = lambda *s: torch.zeros(3, *s, device=DEV)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda k, m, s, B, D: _ext.ops().cma_small_ask(k, m, s, B, D, 8))(
            torch.zeros(3, 2, dtype=torch.int64, device=DEV), z(65), z(), z(65, 65), z(65))
