"""``tdea_small.hip`` (MI355X, marked gpu): the θ-ranking of B runs in one launch, a workgroup per run.

1. ``t_rank``, ``cls`` and ``val`` of run r equal, byte for byte, the 2-D ``theta_rank`` (the four launches of ``rvea_select.hip`` and
   ``tdea_select.hip``) on that run's slices, and the numpy float64 reference of the contract (``_tdea_reference.py``) exactly, as
   ``tests/test_tdea_select_gpu.py`` holds the 2-D op to it.  The runs differ in seed, objectives and mask; the last run repeats its
   first rows in its last rows: equal val in one cluster ranks by position.
2. A run with a NaN row: the bytes of the 2-D op, and every cluster's masked ranks are 1 … c.
3. A per-run shape just above a cap raises ``NotImplementedError``, under ``vmap`` and from the 3-D call.
4. ``BatchedRuns(TDEA)`` equals the solo runs bit for bit, eager and captured.
1 and 4 run with functorch's run-by-run fallback switched off."""
import numpy as np
import pytest
import torch

import _rvea_reference as rv
import _tdea_reference as ref
from evoxmi.ops import _ext, batching
from evoxmi.ops import tdea as tdea_ops
from test_batched_tdea import check_runs_equal_solo

pytestmark = pytest.mark.gpu

# (B, n, nw, m), the runs' masks: one direction; one cluster of 130, past a thread's first row and past a wave; θ-DEA's own directions
# (axes with θ = 1e6), shared by the runs, rows no multiple of the 16 waves and directions past a 64-lane pass; MC = 8; MC = 16; at the
# cap for MC = 4; at the cap for MC = 16
SHAPES = [((1, 2, 1, 2), ("all",)), ((2, 130, 1, 3), ("every7", "all")), ((3, 182 + 5, 91, 3), ("none", "every7", "all")),
          ((2, 70, 33, 5), ("one", "all")), ((2, 40, 20, 16), ("every7", "all")), ((2, 4096, 2048, 3), ("none", "every7")),
          ((2, 1024, 512, 9), ("one", "all"))]


@pytest.fixture
def no_vmap_fallback():
    was = torch._C._functorch._is_vmap_fallback_enabled()
    torch._C._functorch._set_vmap_fallback_enabled(False)
    try:
        yield
    finally:
        torch._C._functorch._set_vmap_fallback_enabled(was)


def _check_runs(obj, w, mask):
    """obj (B, n, m), w (nw, m) or (B, nw, m) and mask (B, n) as numpy arrays."""
    B, n, nw = obj.shape[0], obj.shape[1], w.shape[-2]
    d_obj, d_w, d_mask = (torch.from_numpy(a).cuda() for a in (obj, w, mask))
    got = tdea_ops.theta_rank(d_obj, d_w, d_mask, return_parts=True)
    assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.float64] and all(t.shape == (B, n) for t in got)
    for r in range(B):
        w_r, dw_r = (w, d_w) if w.ndim == 2 else (w[r], d_w[r])
        solo = tdea_ops.theta_rank(d_obj[r], dw_r, d_mask[r], return_parts=True)
        for name, x, y in zip(("t_rank", "cls", "val"), got, solo):
            assert x[r].cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"run {r}: {name} differs from the 2-D op"
        t_rank, cls, val = (t[r].cpu().numpy() for t in got)
        assert ref.clusters_are_ranked(cls, t_rank, mask[r], nw), f"run {r}"
        if not np.isnan(obj[r]).any():  # the contract's exact words are for finite rows
            want_t, want_cls, want_val = ref.theta_rank(obj[r], w_r, mask[r])
            assert np.array_equal(cls, want_cls) and np.array_equal(val.view(np.int64), want_val.view(np.int64)), f"run {r}"
            assert np.array_equal(t_rank, want_t), f"run {r}: t_rank differs in {int((t_rank != want_t).sum())} rows"
    _ext.check_kernel_errors()


@pytest.mark.parametrize("shape,mask_names", SHAPES)
def test_runs_equal_the_2d_op_and_the_reference(shape, mask_names, no_vmap_fallback):
    B, n, nw, m = shape
    obj = np.stack([ref.objectives(n, m, ("front", "uniform")[r % 2], 7 * r + n) for r in range(B)])
    k = max(1, min(8, n // 4))
    obj[-1, n - k:] = obj[-1, :k]
    w = ref.directions(nw, m) if (nw, m) == (91, 3) else np.stack([rv.vectors(nw, m, "rand", 7 * r + nw) for r in range(B)])
    assert w.shape[-2] == nw
    _check_runs(obj, w, np.stack([ref.masks(n)[name] for name in mask_names]))


def test_a_run_with_a_nan_row():
    obj = np.stack([ref.objectives(60, 3, kind, s) for s, kind in enumerate(("uniform", "front"))])
    obj[1, 8, 1] = np.nan
    w = np.stack([rv.vectors(30, 3, "rand", s) for s in range(2)])
    _check_runs(obj, w, np.stack([ref.masks(60)["all"], ref.masks(60)["every7"]]))


@pytest.mark.parametrize("n,nw,m", [(8, 2049, 3), (8, 513, 9), (4097, 4, 3)])
def test_a_run_above_a_cap_raises(n, nw, m):
    batching.register()
    obj, w, mask = torch.rand(2, n, m, device="cuda"), torch.rand(2, nw, m, device="cuda"), torch.ones(2, n, dtype=torch.bool, device="cuda")
    with pytest.raises(NotImplementedError):
        torch.func.vmap(tdea_ops.theta_rank)(obj, w, mask)
    with pytest.raises(NotImplementedError):
        tdea_ops.theta_rank(obj, w, mask)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_tdea_runs_equal_solo_gpu(graph, no_vmap_fallback):
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    check_runs_equal_solo("cuda", graph)
    _ext.check_kernel_errors()
