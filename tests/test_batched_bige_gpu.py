"""``bige_small.hip`` (MI355X, marked gpu): the bi-goal estimate and its Pareto rank of B runs in one launch, a workgroup per run.

1. ``bi``, ``rank``, ``pr`` and ``cd`` of run r equal, byte for byte, the 2-D ``estimate`` (the three launches of ``bige_select.hip``)
   and ``non_dominated_sort`` of its ``bi`` on that run's slices; ``pr`` equals the numpy float64 reference of the contract
   (``_bige_reference.py``) exactly, with the device's own r word, and ``cd`` is within (n + 2)·2⁻⁵³ relative of it, as
   ``tests/test_bige_select_gpu.py`` holds the 2-D op to it; a second call is bitwise equal.  The runs differ in seed, objectives and
   mask; the last run repeats its first rows in its last rows: equal ``cd``, and neither dominates.
2. A run with a NaN objective: the launch ends, the shapes hold, and the other run has the bytes of its 2-D call.
3. A per-run shape just above a cap raises ``NotImplementedError``, under ``vmap`` and from the 3-D call.
4. ``BatchedRuns(BiGE)`` equals the solo runs bit for bit, eager and captured.
1 and 4 run with functorch's run-by-run fallback switched off."""
import numpy as np
import pytest
import torch

import _bige_reference as ref
from evoxmi.ops import _ext, batching
from evoxmi.ops import bige as bige_ops
from evoxmi.ops import nds as nds_ops
from test_batched_bige import SHAPES, check_runs_equal_solo, runs_of

pytestmark = pytest.mark.gpu


@pytest.fixture
def no_vmap_fallback():
    was = torch._C._functorch._is_vmap_fallback_enabled()
    torch._C._functorch._set_vmap_fallback_enabled(False)
    try:
        yield
    finally:
        torch._C._functorch._set_vmap_fallback_enabled(was)


def _same_bytes_as_2d(got, d_fit, d_mask, r):
    bi, pr, cd = bige_ops.estimate(d_fit[r], d_mask[r], return_parts=True)
    for name, x, y in zip(("bi", "rank", "pr", "cd"), got, (bi, nds_ops.non_dominated_sort(bi), pr, cd)):
        assert x[r].dtype == y.dtype and x[r].cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"run {r}: {name} differs from the 2-D ops"


@pytest.mark.parametrize("shape,mask_names", SHAPES)
def test_runs_equal_the_2d_ops_and_the_reference(shape, mask_names, no_vmap_fallback):
    B, n, m = shape
    fit, mask = runs_of(shape, mask_names)
    d_fit, d_mask = torch.from_numpy(fit).cuda(), torch.from_numpy(mask).cuda()
    got = bige_ops.estimate_rank(d_fit, d_mask, return_parts=True)
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float64, torch.float64]
    assert got[0].shape == (B, n, 2) and all(t.shape == (B, n) for t in got[1:])
    for r in range(B):
        _same_bytes_as_2d(got, d_fit, d_mask, r)
        r_word = np.float32((1 / d_mask[r].sum().to(torch.float32) ** (1 / m)).item())  # the device's own, an input of the contract
        _, pr64, cd64, gap = ref.estimate(fit[r], mask[r], r_word)
        pr, cd, rank = (t[r].cpu().numpy() for t in (got[2], got[3], got[1]))
        assert gap > 1e-9 and np.array_equal(pr.view(np.int64), pr64.view(np.int64)), f"run {r}: pr differs (thr_gap {gap:.3e})"
        want, have = cd64[mask[r]], cd[mask[r]]
        err = float(np.max(np.abs(have - want) / np.where(want > 0, want, 1.0), initial=0.0))
        print(f"[bige small] {shape} run {r} {mask_names[r]}: cd rel {err * 2.0**53:.2f}·2^-53 (bound {n + 2}·2^-53), thr_gap {gap:.3e}, "
              f"{int(rank.max()) + 1} fronts")
        assert err <= (n + 2) * 2.0**-53 and (have[want == 0] == 0).all() and np.isposinf(cd[~mask[r]]).all()
        if not mask[r].any():
            assert (rank == 0).all()
    k = max(1, min(8, n // 4))
    if n > 1 and mask[-1, :k].all() and mask[-1, n - k:].all():  # the repeated rows: equal words, and neither dominates
        assert torch.equal(got[3][-1, :k], got[3][-1, n - k:]) and torch.equal(got[1][-1, :k], got[1][-1, n - k:])
    again = bige_ops.estimate_rank(d_fit, d_mask, return_parts=True)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(got, again))
    _ext.check_kernel_errors()


def test_a_run_with_a_nan_objective():
    fit, mask = runs_of((2, 60, 3), ("all", "every7"))
    fit[1, 8, 1] = np.nan
    d_fit, d_mask = torch.from_numpy(fit).cuda(), torch.from_numpy(mask).cuda()
    got = bige_ops.estimate_rank(d_fit, d_mask, return_parts=True)
    torch.cuda.synchronize()
    _ext.check_kernel_errors()
    assert got[0].shape == (2, 60, 2) and all(t.shape == (2, 60) for t in got[1:])
    _same_bytes_as_2d(got, d_fit, d_mask, 0)


@pytest.mark.parametrize("n,m", [(2049, 3), (1025, 5), (513, 9)])
def test_a_run_above_a_cap_raises(n, m):
    batching.register()
    fit, mask = torch.rand(2, n, m, device="cuda"), torch.ones(2, n, dtype=torch.bool, device="cuda")
    with pytest.raises(NotImplementedError):
        torch.func.vmap(bige_ops.estimate_rank)(fit, mask)
    with pytest.raises(NotImplementedError):
        bige_ops.estimate_rank(fit, mask)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_bige_runs_equal_solo_gpu(graph, no_vmap_fallback):
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    check_runs_equal_solo("cuda", graph)
    _ext.check_kernel_errors()
