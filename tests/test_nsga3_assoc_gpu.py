"""``nsga3_assoc.hip`` and the run index of ``nsga3_select.hip`` (MI355X, marked gpu) against the float64 host reference of
``_nsga3_reference.py``, and ``BatchedRuns(NSGA3)`` on the device.  Runs of different kinds share the launches: ``front`` (positive rows
on the unit sphere) and ``uniform`` (uniform rows + 1e-3), both with row ⌊j·n/m⌋ overwritten by 0.01 + (0.99 + 0.1j)·e_j so that the
extremes are distinct and cond(E) is small (asserted), and ``degenerate`` (the (1030, 16) uniform rows without planted ones: an extreme
row repeats and the nadir is ``worst``).  Largest observed group_dist error over its bound: 0.163, at (1030, 300, 16) (profiles/NOTES.md)."""
import functools

import numpy as np
import pytest
import torch
from torch.func import vmap

import _nsga3_reference as ref64
from evoxmi import random as rnd
from evoxmi.operators.selection import non_dominated_sort
from evoxmi.ops import nds as nds_ops
from evoxmi.ops import nsga3 as nsga3_ops
from test_batched_ibea_spea2 import same_bits
from test_batched_ibea_spea2_gpu import ext  # noqa: F401  (the fixture: the extension loads, no kernel error afterwards)
from test_batched_mo import D, GENS, M, POP, RUNS
from test_batched_nsga3 import check_runs_equal_solo

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3, 2), (65, 66, 3), (200, 91, 3), (257, 1025, 5), (1030, 300, 16), (8192, 4095, 3)]


def _rows(n, m, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "front":
        f = np.abs(rng.standard_normal((n, m))) + 1e-3
        f = (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)
    else:
        f = rng.random((n, m), dtype=np.float32) + np.float32(1e-3)
    if kind != "degenerate":
        for j in range(m):
            f[j * n // m] = 0.01 + (0.99 + 0.1 * j) * np.eye(m, dtype=np.float32)[j]
    return f


@functools.lru_cache(maxsize=None)
def case(n, K, m):
    """(kinds, f (B, n, m), rank (B, n), ref (K, m), N, the reference of every run), computed once and left unchanged; B = 1 at the cap."""
    seed, N = 100 * n + m, n // 2
    kinds = ["front", "uniform", "degenerate" if (n, m) == (1030, 16) else "front"][: 1 if n == 8192 else 3]
    f = torch.from_numpy(np.stack([_rows(n, m, kind, seed + i) for i, kind in enumerate(kinds)]))
    ref = torch.from_numpy(np.random.default_rng(seed + 3).random((K, m), dtype=np.float32) + np.float32(0.05))
    rank = torch.stack([non_dominated_sort(fb, until=N + 1) for fb in f])
    return kinds, f, rank, ref, N, [ref64.associate(fb.numpy(), rb.numpy(), ref.numpy(), N) for fb, rb in zip(f, rank)]


@pytest.mark.parametrize("n,K,m", SHAPES)
def test_associate_against_reference(ext, n, K, m):
    kinds, f, rank, ref, N, want = case(n, K, m)
    ratio = 0.0
    for B in sorted({1, len(kinds)}):
        out = nsga3_ops.associate(f[:B].cuda(), rank[:B].cuda(), ref.cuda(), N)
        assert all(same_bits(a, b) for a, b in zip(out, nsga3_ops.associate(f[:B].cuda(), rank[:B].cuda(), ref.cuda(), N))), "a second call"
        last_rank, group, gd, scale = (t.cpu().numpy() for t in out)
        assert group.dtype == np.int64 and gd.dtype == np.float32 and scale.shape == (B, 2, m)
        for b, w in enumerate(want[:B]):
            assert last_rank[b] == w["last_rank"] and np.array_equal(scale[b, 0], w["ideal"]), (B, b)
            if kinds[b] == "degenerate":
                assert w["used_worst"] and np.array_equal(scale[b, 1], w["worst"])
            else:
                assert w["cond"] <= 100 and not w["used_worst"], f"the fixture no longer qualifies: cond {w['cond']:.3g}"
                assert np.all(np.abs(scale[b, 1] - w["nadir"]) <= w["cond"] * 8 * m * 2.0**-53 * w["nadir"]), (B, b)
            tol = w["xnorm"] * np.sqrt(m + 3) * 2.0**-25 + 2.0**-23 * w["dmin"]
            err = np.abs(gd[b] - w["dmin"])
            ratio = max(ratio, float((err / tol).max()))
            assert np.all(err <= tol), (B, b, ratio)
            assert np.all(w["dist_to"](group[b]) - w["dmin"] <= tol), (B, b)
    print(f"[nsga3_assoc] ({n}, {K}, {m}): largest group_dist error / bound = {ratio:.3f}")


@pytest.mark.parametrize("n,K,m", [(65, 66, 3), (1030, 300, 16)])
def test_batched_equals_solo_ops(ext, n, K, m):
    _, f, rank, ref, N, _ = case(n, K, m)
    f, rank, ref = f.cuda(), rank.cuda(), ref.cuda()
    keys = rnd.split(rnd.PRNGKey(3, device="cuda"), 3)
    out = nsga3_ops.associate(f, rank, ref, N)
    idx = nds_ops.nsga3_survivors(rank, out[0], out[1], out[2], keys, N, K)
    for b in range(3):
        solo = nsga3_ops.associate(f[b], rank[b], ref, N)
        assert all(same_bits(o[b], s) for o, s in zip(out, solo)), f"run {b}"
        assert torch.equal(idx[b], nds_ops.nsga3_survivors(rank[b], solo[0], solo[1], solo[2], keys[b], N, K)), f"run {b}: survivors"
    assert not torch.equal(idx[0], idx[1])


def test_zero_and_nan_rows(ext):
    _, f, _, ref, N, _ = case(65, 66, 3)
    f = f[1].clone()
    f[5] = f.min(0).values  # the ideal point itself: x = 0
    rank = non_dominated_sort(f, until=N + 1)
    f[9, 1], rank[9] = float("nan"), 65  # outside valid, so ideal and nadir stay finite
    _, group, gd, scale = nsga3_ops.associate(f.cuda(), rank.cuda(), ref.cuda(), N)
    assert bool(torch.isfinite(scale).all())
    assert torch.nonzero(torch.isnan(gd)).flatten().tolist() == [5, 9] and group[5] == 0 and group[9] == 0


def test_batched_runs_equal_solo_and_captured_equals_eager(ext):
    from evoxmi.algorithms.containers.batched import BatchedRuns
    from evoxmi.algorithms.mo.nsga3 import NSGA3
    from evoxmi.problems.numerical import DTLZ2
    from evoxmi.workflows import StdWorkflow

    def final(graph):
        wf = StdWorkflow(BatchedRuns(NSGA3(torch.zeros(D, device="cuda"), torch.ones(D, device="cuda"), M, POP), RUNS), DTLZ2(d=D, m=M), graph=graph)
        st = wf.init(rnd.PRNGKey(9, device="cuda"))
        for _ in range(GENS + 1):  # the initial evaluation, then GENS generations
            st = wf.step(st)
        runs = st.get_child_state("algorithm").runs
        return runs.population.clone(), runs.fitness.clone()

    check_runs_equal_solo("cuda")
    (p0, f0), (p1, f1) = final(False), final(True)
    assert p0.shape == (RUNS, POP, D) and torch.equal(p0, p1) and torch.equal(f0, f1)


def test_caps(ext, monkeypatch):
    from evoxmi.ops import batching

    batching.register()
    for (n, m), K in (((8193, 3), 10), ((16, 9), 10), ((16, 3), 8193)):
        f, ref = torch.rand(2, n, m, device="cuda"), torch.rand(K, m, device="cuda")
        with pytest.raises(NotImplementedError):  # a tell's calls: the sort (n ≤ 8192, m ≤ 8), then the association
            vmap(lambda x: nsga3_ops.associate(x, non_dominated_sort(x, until=9), ref, 8))(f)
    with pytest.raises(NotImplementedError, match="K = 8193"):
        nsga3_ops.associate(f, torch.zeros(2, 16, dtype=torch.int32, device="cuda"), ref, 8)
    rank = non_dominated_sort(f[0], until=9)  # a solo call above a cap still takes the torch path
    monkeypatch.setattr(nsga3_ops._ext, "ops", lambda: pytest.fail("the kernel was called where the torch path is due"))
    _, group, _, scale = nsga3_ops.associate(f[0], rank, ref, 8)
    assert group.is_cuda and group.shape == (16,) and scale.shape == (2, 3)
