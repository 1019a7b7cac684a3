"""``ops.geom.hype_fitness`` on ``hype_fitness.hip`` (MI355X, marked gpu): ``torch.equal`` against the composition it replaces
(``uniform`` → ``hv_count`` → ``hv_contrib``), and against float64 numpy on the same float32 samples within the derived bound
(⌈n_sample / 256⌉ + 8) · 2⁻²⁴ · Σ_s (terms of point i); counts exactly through an α of ones.  Every case has two duplicate rows and a
row equal to ``ref`` (at n ≤ 2 every row is ``ref``); (7, 3, 257) has a row of column minima; (33, 7, 1000) is the m ≤ 8
instantiation; (2048, 3, 10000) needs two LDS tiles of points."""
import functools

import numpy as np
import pytest
import torch
from torch.func import vmap

from evoxmi import random as rnd

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (2, 2, 255), (7, 3, 257), (33, 7, 1000), (64, 16, 4096), (200, 3, 10000), (2048, 3, 10000)]


@pytest.fixture
def geom():
    from evoxmi.ops import _ext, batching, geom

    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    batching.register()
    yield geom
    torch.cuda.synchronize()
    _ext.check_kernel_errors()


def _points(n, m, seed):
    p, ref = torch.rand(n, m, generator=torch.Generator().manual_seed(seed)), torch.full((m,), 1.1)
    if n > 2:
        p[1] = p[0]
        if (n, m) == (7, 3):
            p[2] = p.min(0).values
    else:
        p[:] = ref
    p[n - 1] = ref
    return p.cuda(), ref.cuda()


def _composition(geom, p, ref, alpha, key, ns):
    f_min = p.min(0).values
    samples = rnd.uniform(key, (ns, p.shape[1])) * (ref - f_min) + f_min
    return geom.hv_contrib(samples, p, geom.hv_count(samples, p, strict=False), alpha), samples


@functools.lru_cache(maxsize=None)
def case(n, m, ns):
    """points, ref, α, key, the composition's f, and the float64 dominance matrix and weights on its float32 samples."""
    from evoxmi.ops import geom

    p, ref = _points(n, m, 100 * n + m)
    alpha = (1.0 / torch.arange(1, n + 1, dtype=torch.float32)).cuda()
    key = rnd.PRNGKey(1000 + n, device="cuda")
    want, samples = _composition(geom, p, ref, alpha, key, ns)
    dom = (p.cpu().numpy()[:, None, :] <= samples.cpu().numpy()[None, :, :]).all(-1)  # (n, ns)
    c = dom.sum(0)
    w = np.where(c > 0, alpha.cpu().numpy().astype(np.float64)[np.maximum(c - 1, 0)], 0.0)
    return p, ref, alpha, key, want, dom, w


@pytest.mark.parametrize("n,m,ns", SHAPES)
def test_fused_equals_composition_and_float64(geom, n, m, ns):
    p, ref, alpha, key, want, dom, w = case(n, m, ns)
    assert geom.hype_fused_ok(n, m, ns)
    f = geom.hype_fitness(p, ref, alpha, key, ns)
    assert f.shape == (n,) and f.dtype == torch.float32
    assert torch.equal(f, want), f"differs from the composition in {int((f != want).sum())} of {n} rows"
    err, bound = np.abs(f.cpu().numpy().astype(np.float64) - dom @ w), (-(-ns // 256) + 8) * 2.0**-24 * (dom @ np.abs(w))
    print(f"[hype_fitness] ({n}, {m}, {ns}): max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    ones = geom.hype_fitness(p, ref, torch.ones_like(alpha), key, ns)
    assert np.array_equal(ones.cpu().numpy(), dom.sum(1).astype(np.float32))
    assert torch.equal(geom.hype_fitness(p, ref, alpha, key, ns), f)  # a second call


@pytest.mark.parametrize("n,m,ns", [(7, 3, 257), (33, 7, 1000), (200, 3, 10000)])
def test_batched_equals_per_run_calls(geom, n, m, ns):
    runs = [_points(n, m, seed) for seed in (1, 2, 3)]
    P, R = torch.stack([p for p, _ in runs]), torch.stack([r for _, r in runs]) * torch.tensor([[1.0], [1.5], [2.0]], device="cuda")
    alpha, keys = case(n, m, ns)[2], rnd.split(rnd.PRNGKey(4, device="cuda"), 3)
    f = geom.hype_fitness(P, R, alpha, keys, ns)
    assert f.shape == (3, n) and not torch.equal(f[0], f[1])
    for b in range(3):
        assert torch.equal(f[b], geom.hype_fitness(P[b], R[b], alpha, keys[b], ns)), f"run {b}"
    assert torch.equal(vmap(lambda p, r, k: geom.hype_fitness(p, r, alpha, k, ns))(P, R, keys), f)
    with pytest.raises(NotImplementedError, match="alpha must be shared"):
        vmap(lambda p, r, k, a: geom.hype_fitness(p, r, a, k, ns))(P, R, keys, alpha.expand(3, n))


def test_outside_the_caps(geom, monkeypatch):
    n, m, ns = 2049, 2, 300
    assert not geom.hype_fused_ok(n, m, ns) and not geom.hype_fused_ok(8, 17, ns) and geom.hype_fused_ok(2048, 16, ns)
    P = torch.rand(2, n, m, device="cuda")
    R, alpha, keys = torch.full((2, m), 1.2, device="cuda"), torch.ones(n, device="cuda"), rnd.split(rnd.PRNGKey(6, device="cuda"), 2)
    with pytest.raises(NotImplementedError, match="n = 2049"):
        geom.hype_fitness(P, R, alpha, keys, ns)
    with pytest.raises(NotImplementedError, match="hv_count vmap rule"):
        vmap(lambda p, r, k: geom.hype_fitness(p, r, alpha, k, ns))(P, R, keys)
    with pytest.raises(NotImplementedError, match="hype_fitness vmap rule.*n = 2049"):
        vmap(lambda p, r, k: torch.ops.evoxmi.hype_fitness(p, r, alpha, k, ns))(P, R, keys)
    ops = geom._ext.ops()

    class NoKernel:  # a solo call takes the composition, not the kernel
        def __getattr__(self, name):
            assert name != "hype_fitness", "the kernel was called where the composition is due"
            return getattr(ops, name)

    monkeypatch.setattr(geom._ext, "ops", lambda: NoKernel())
    assert torch.equal(geom.hype_fitness(P[0], R[0], alpha, keys[0], ns), _composition(geom, P[0], R[0], alpha, keys[0], ns)[0])
