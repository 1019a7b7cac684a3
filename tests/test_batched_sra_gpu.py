"""``sra_small.hip`` (MI355X, marked gpu): SRA's selection of B runs in one launch, a workgroup per run.

1. For every run, ``idx``, ``I1`` and ``I2`` equal the 2-D ``select`` (the two launches of ``sra_select.hip``) on that run's slices byte
   for byte; ``idx`` is exactly the sequential host op ``evoxmi::stochastic_ranking`` on the returned indicators; and on the finite
   runs I1 and I2 follow the rule of ``tests/test_sra_rank_gpu.py`` against a float64 torch evaluation of the same float32 objectives,
   ``e_k <= 4·e_t + 2·ulp32(max |ref64|)``, while NaN and inf appear where the dense expressions put them.  The runs of a case differ
   in data and pc; run r of case k is of kind (k + r) mod 4: pc = 0 (I2 only); pc = 1 on objectives whose I1 ascends by position
   (after ⌈n/2⌉ sweeps the result is only half sorted, which shows a wrong sweep count or window edge); repeated rows (ties); a NaN
   and a +inf objective.
2. A per-run shape above a cap raises ``NotImplementedError``, directly and under ``vmap``, and so do batched ``indicators`` and
   ``stochastic_rank``.
3. ``BatchedRuns(SRA)`` equals the solo runs bit for bit, eager and captured, with functorch's run-by-run fallback switched off."""
import pytest
import torch

from evoxmi.ops import _ext, batching
from evoxmi.ops import sra as sra_ops
from test_batched_sra import check_runs_equal_solo
from test_sra_rank_gpu import _rule

pytestmark = pytest.mark.gpu

# (B, n, m): one comparator; odd n; a second lane pass and rows no multiple of the 16 waves; one ranking wave → two; two → three; four
# waves, then five, at both parities of n; the two caps
SHAPES = [(1, 2, 2), (3, 3, 3), (2, 65, 3), (2, 128, 3), (2, 129, 3), (2, 256, 5), (2, 257, 5), (2, 512, 3), (2, 513, 3), (2, 514, 3),
          (2, 1024, 16), (2, 2048, 8)]
KINDS = ["only_I2", "I1_ascending", "ties", "nonfinite"]
PC = {"only_I2": 0.0, "I1_ascending": 1.0, "ties": 0.5, "nonfinite": 0.45}


def _run_objectives(kind, n, m, gen):
    obj = torch.rand(n, m, generator=gen)
    if kind == "I1_ascending":  # row p dominates every row before it by 0.01 · 0.05 per step: Σ_q exp(…) falls with p (at most e^20.5)
        obj = ((n - torch.arange(n, dtype=torch.float32)) * 0.0005)[:, None].expand(n, m).clone()
    elif kind == "ties":
        obj[n // 2:] = obj[:n - n // 2].clone()
    elif kind == "nonfinite":
        obj[0, 0], obj[n - 1, m - 1] = float("nan"), float("inf")
    return obj


@pytest.mark.parametrize("B,n,m", SHAPES)
def test_runs_equal_the_2d_op_the_host_ranking_and_the_float64_indicators(B, n, m):
    gen = torch.Generator().manual_seed(1000 * n + m)
    kinds = [KINDS[(SHAPES.index((B, n, m)) + r) % 4] for r in range(B)]
    obj = torch.stack([_run_objectives(k, n, m, gen) for k in kinds]).cuda()
    u = torch.rand(B, n - 1, generator=gen).cuda()
    pc = torch.tensor([PC[k] for k in kinds], dtype=torch.float32, device="cuda")
    got = sra_ops.select(obj, u, pc, return_info=True)
    assert [t.dtype for t in got] == [torch.int64, torch.float32, torch.float32] and all(t.shape == (B, n) for t in got)
    for r, kind in enumerate(kinds):
        solo = sra_ops.select(obj[r], u[r], pc[r], return_info=True)
        for name, x, y in zip(("idx", "I1", "I2"), got, solo):
            assert x[r].cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f"run {r} ({kind}): {name} differs from the 2-D op"
        idx, I1, I2 = (t[r].cpu() for t in got)
        assert torch.equal(idx, _ext.ops().stochastic_ranking(I1, I2, u[r].cpu(), float(pc[r]))), f"run {r} ({kind}): not the host ranking"
        if kind == "nonfinite":
            for g, w in zip((I1, I2), sra_ops.indicators_dense(obj[r])):
                assert all(torch.equal(f(g), f(w.cpu())) for f in (torch.isnan, torch.isposinf, torch.isneginf)), f"run {r}: NaN / inf pattern"
            continue
        t32, ref64 = sra_ops.indicators_dense(obj[r].cpu()), sra_ops.indicators_dense(obj[r].cpu().double())
        _rule(f"I1 run {r} ({kind})", I1, t32[0], ref64[0])
        _rule(f"I2 run {r} ({kind})", I2, t32[1], ref64[1])
        if kind == "I1_ascending":
            assert bool((I1[1:] > I1[:-1]).all())
            if n >= 4:
                assert not torch.equal(idx, torch.arange(n).flip(0)) and not torch.equal(idx, torch.arange(n))
    _ext.check_kernel_errors()


@pytest.mark.parametrize("B,n,m", [(2, 2049, 3), (2, 1025, 9), (2, 8, 17)])
def test_a_run_above_a_cap_raises(B, n, m):
    batching.register()
    obj, u = torch.rand(B, n, m, device="cuda"), torch.rand(B, n - 1, device="cuda")
    with pytest.raises(NotImplementedError):
        sra_ops.select(obj, u, 0.5)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda o, uu: sra_ops.select(o, uu, 0.5))(obj, u)


def test_batched_indicators_and_rank_raise():
    batching.register()
    obj, u = torch.rand(2, 8, 3, device="cuda"), torch.rand(2, 7, device="cuda")
    with pytest.raises(NotImplementedError):
        torch.func.vmap(sra_ops.indicators)(obj)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda a, uu: sra_ops.stochastic_rank(a, a, uu, 0.5))(obj[:, :, 0], u)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_batched_sra_runs_equal_solo_gpu(graph):
    assert _ext.load(), f"evoxmi extension must load on a GPU box: {_ext._ERROR!r}"
    was = torch._C._functorch._is_vmap_fallback_enabled()
    torch._C._functorch._set_vmap_fallback_enabled(False)
    try:
        check_runs_equal_solo("cuda", graph)
    finally:
        torch._C._functorch._set_vmap_fallback_enabled(was)
    _ext.check_kernel_errors()
