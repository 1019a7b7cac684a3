"""``rvea_small.hip`` (MI355X, marked gpu): the APD selection of B runs in one launch, a workgroup per run.

1. Every output of run r equals, bit for bit, the 2-D ``select`` (the five launches of ``rvea_select.hip``) on that run's slices.  On
   fixtures that ``_rvea_reference.qualifies`` accepts, ``arg``, ``next_ind`` and ``empty`` equal the numpy float64 reference and ``apd``
   and γ agree with it within 1e-12 relative, as ``tests/test_rvea_select_gpu.py`` holds the 2-D op to it.  The runs differ in seed,
   vectors and θ; run 0 has θ = 0 and the last run repeats kept rows in its last rows: equal least apd, the lower position wins.
2. A per-run shape just above a cap raises ``NotImplementedError`` under ``vmap``, and so does a batched ``cos_best``.
3. ``BatchedRuns(RVEA)`` equals the solo runs bit for bit, eager and captured, with functorch's run-by-run fallback switched off."""
import functools

import numpy as np
import pytest
import torch

import _rvea_reference as ref
from evoxmi.ops import _ext, batching
from evoxmi.ops import rvea as rvea_ops
from test_batched_rvea import check_runs_equal_solo

pytestmark = pytest.mark.gpu

THETAS = (0.0, 0.49, 1.0)
# (B, n, nv, m): one vector (γ = acos 0); rows no multiple of the 16 waves and vectors one past a 64-lane pass; MC = 8; MC = 16; at
# the cap for MC = 4; at the cap for MC = 16
SHAPES = [(1, 2, 1, 2), (3, 130, 65, 3), (2, 70, 33, 5), (2, 40, 20, 16), (2, 4096, 2048, 3), (2, 1024, 512, 9)]


@functools.lru_cache(maxsize=None)
def _run_fixture(B, n, nv, m, r):
    """``(f, v, theta, want)`` of run r: the first seed whose fixture qualifies and, in the last run, has a vector whose least apd two
    rows hold (host arithmetic only)."""
    for seed in range(100 * r, 100 * r + 20):
        f, v = ref.objectives(n, m, 0.25 if n >= 4 else 0.0, seed), ref.vectors(nv, m, "rand", seed)
        if r == B - 1:  # the rows some vectors keep, again in the last k rows: the least apd of a vector at two positions
            k = max(1, min(8, n // 4))
            first = ref.select(f, v, THETAS[r])
            keep = first["next_ind"][~first["empty"] & (first["next_ind"] < n - k)][:k]
            f[n - len(keep):] = f[keep]
        want = ref.select(f, v, THETAS[r])
        tied = any((want["apd"][want["arg"] == j] == want["apd"][want["next_ind"][j]]).sum() > 1 for j in np.flatnonzero(~want["empty"]))
        if ref.qualifies(want["a"], want["b"]) and (tied or r < B - 1):
            return f, v, THETAS[r], want
    raise AssertionError("no qualifying fixture in 20 seeds")


def _check_runs(fixtures):
    f, v = (torch.from_numpy(np.stack(a)).cuda() for a in zip(*((fx[0], fx[1]) for fx in fixtures)))
    theta = torch.tensor([fx[2] for fx in fixtures], dtype=torch.float32, device="cuda")
    got = rvea_ops.select(f, v, theta, return_info=True)
    B, n, nv = f.shape[0], f.shape[1], v.shape[1]
    assert [t.dtype for t in got] == [torch.int64, torch.bool, torch.int64, torch.float64, torch.float64]
    assert [tuple(t.shape) for t in got] == [(B, nv), (B, nv), (B, n), (B, n), (B, nv)]
    for r, (_, _, _, want) in enumerate(fixtures):
        solo = rvea_ops.select(f[r], v[r], theta[r], return_info=True)
        for name, x, y in zip(("next_ind", "empty", "arg", "apd", "gamma"), got, solo):
            assert x[r].cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"run {r}: {name} differs from the 2-D op"
        next_ind, empty, arg, apd, gamma = (t[r].cpu().numpy() for t in got)
        assert np.array_equal(arg, want["arg"]) and np.array_equal(empty, want["empty"]) and np.array_equal(next_ind, want["next_ind"])
        assert np.allclose(gamma, want["gamma"], rtol=1e-12, atol=0.0)
        assert np.allclose(apd[arg >= 0], want["apd"][arg >= 0], rtol=1e-12, atol=0.0)
    _ext.check_kernel_errors()


@pytest.mark.parametrize("B,n,nv,m", SHAPES)
def test_runs_equal_the_2d_op_and_the_reference(B, n, nv, m):
    fixtures = [_run_fixture(B, n, nv, m, r) for r in range(B)]
    if nv > 1:
        assert any(fx[3]["empty"].any() for fx in fixtures), "no vector without a member"
    _check_runs(fixtures)


@pytest.mark.parametrize("name", list(ref.hand_cases()))
def test_hand_cases_as_one_run(name):
    f, v, theta = ref.hand_cases()[name]
    _check_runs([(f, v, theta, ref.select(f, v, theta))])


@pytest.mark.parametrize("n,nv,m", [(8, 2049, 3), (8, 513, 9), (4097, 4, 3)])
def test_a_run_above_a_cap_raises(n, nv, m):
    batching.register()
    f, v = torch.rand(2, n, m, device="cuda"), torch.rand(2, nv, m, device="cuda")
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda fr, vr: rvea_ops.select(fr, vr, 0.3))(f, v)
    with pytest.raises(NotImplementedError):
        rvea_ops.select(f, v, 0.3)


def test_a_batched_cos_best_raises():
    batching.register()
    a, b = torch.rand(2, 8, 3, device="cuda"), torch.rand(4, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda ar: rvea_ops.cos_best(ar, b))(a)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_rvea_runs_equal_solo_gpu(graph):
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    was = torch._C._functorch._is_vmap_fallback_enabled()
    torch._C._functorch._set_vmap_fallback_enabled(False)
    try:
        check_runs_equal_solo("cuda", graph)
    finally:
        torch._C._functorch._set_vmap_fallback_enabled(was)
    _ext.check_kernel_errors()
