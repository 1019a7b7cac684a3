"""BatchedRuns over IBEA and SPEA2 on the CPU, and the (B, n, m) forms of ``evoxmi.ops.ibea`` and
``evoxmi.ops.spea2``: run r of a batch must equal, bit for bit, the algorithm run alone from
``run_keys(key)[r]``, and row b of every 3-D output the 2-D call on ``obj[b]``.

SPEA2's torch path has data-dependent control flow (the size of the non-dominated set, the length
of the removal loop) and ``torch.cdist`` changes its form with the row count, so under ``vmap`` and
for 3-D input it goes through Python-registered ops that apply the 2-D path run by run
(``evoxmi/ops/spea2.py``): by construction the sequential result, and the oracle the device
kernels are held to in ``tests/test_batched_ibea_spea2_gpu.py``.  IBEA's torch path is traced by
``vmap`` itself."""
import pytest
import torch

from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.ibea import IBEA
from evoxmi.algorithms.mo.spea2 import SPEA2
from evoxmi.ops import ibea as ibea_ops
from evoxmi.ops import spea2 as spea2_ops
from evoxmi.problems.numerical import DTLZ2

from test_batched_mo import D, GENS, M, POP, RUNS, run

assert (D, M, POP, RUNS, GENS) == (12, 3, 20, 3, 6)
ALGOS = {"IBEA": IBEA, "SPEA2": SPEA2}
KAPPA = 0.05


def make(name, dev):
    return ALGOS[name](torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)


def check_runs_equal_solo(name, dev):
    prob = DTLZ2(d=D, m=M)
    pst = prob.init(rnd.PRNGKey(1, device=dev))
    key = rnd.PRNGKey(5, device=dev)
    b = BatchedRuns(make(name, dev), RUNS)
    bst = run(b, key, prob, pst, RUNS)
    assert bst.runs.population.shape == (RUNS, POP, D) and bst.runs.fitness.shape == (RUNS, POP, M)
    for r, k in enumerate(b.run_keys(key)):
        sst = run(make(name, dev), k, prob, pst)
        assert torch.equal(bst.runs.population[r], sst.population), f"{name} run {r}: population differs"
        assert torch.equal(bst.runs.fitness[r], sst.fitness), f"{name} run {r}: fitness differs"
    # the runs are independent: different keys, different populations
    assert not torch.equal(bst.runs.population[0], bst.runs.population[1])
    return bst


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_batched_runs_equal_solo_cpu(name):
    check_runs_equal_solo(name, "cpu")


# ---------------------------------------------------------------- 3-D inputs
def same_bits(a, b):
    """Equal shape, dtype and bits (so that NaNs count)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def four_runs(n=30, m=3):
    """(4, n, m): rows on a front, uniform rows, all rows equal, a run with a NaN row and an inf row."""
    g = torch.Generator().manual_seed(3)
    front = torch.rand(n, m, generator=g) + 1e-3
    front = front / front.norm(dim=1, keepdim=True)  # on the unit sphere: every row non-dominated
    uniform = torch.rand(n, m, generator=g)
    equal = torch.full((n, m), 0.5)
    bad = torch.rand(n, m, generator=g)
    bad[4] = float("nan")
    bad[9] = float("inf")
    return torch.stack([front, uniform, equal, bad])


def test_ibea_3d_cpu():
    obj = four_runs()
    n_keep = 15
    f, C = ibea_ops.fitness(obj, KAPPA)
    idx, order = ibea_ops.select(obj, KAPPA, n_keep, return_order=True)
    assert f.shape == (4, 30) and C.shape == (4, 30) and idx.shape == (4, n_keep) and order.shape == (4, 30 - n_keep)
    assert same_bits(ibea_ops.select(obj, KAPPA, n_keep), idx)
    for b in range(4):
        fb, Cb = ibea_ops.fitness(obj[b], KAPPA)
        ib, ob = ibea_ops.select(obj[b], KAPPA, n_keep, return_order=True)
        assert same_bits(f[b], fb) and same_bits(C[b], Cb), f"run {b}: fitness"
        assert same_bits(idx[b], ib) and same_bits(order[b], ob), f"run {b}: selection"
    assert bool(torch.isfinite(f[:2]).all()) and bool(torch.isnan(f[2:]).all())  # the scalar normalisation is per run
    full = ibea_ops.select(obj, KAPPA, 30, return_order=True)
    assert torch.equal(full[0], torch.arange(30).expand(4, 30)) and full[1].shape == (4, 0)


def test_spea2_3d_cpu():
    obj = four_runs()
    n_keep = 15
    parts = spea2_ops.fitness(obj, return_parts=True)
    assert len(parts) == 5 and all(p.shape == (4, 30) for p in parts)
    assert same_bits(spea2_ops.fitness(obj), parts[0])
    masks = {"nd": parts[0] < 1, "all": torch.ones(4, 30, dtype=torch.bool)}
    assert masks["nd"].sum(1).tolist()[0] == 30 and int(masks["nd"][1].sum()) < n_keep  # one run truncates, one does not
    for b in range(4):
        for got, want in zip(parts, spea2_ops.fitness(obj[b], return_parts=True)):
            assert same_bits(got[b], want), f"run {b}: fitness parts"
        assert same_bits(parts[0][b], spea2_ops.fitness(obj[b]))
    for name, mask in masks.items():
        keep, order, rescans = spea2_ops.truncate(obj, mask, n_keep, return_order=True)
        assert keep.shape == (4, 30) and order.shape == (4, 30 - n_keep) and rescans.shape == (4,)
        assert same_bits(spea2_ops.truncate(obj, mask, n_keep), keep)
        for b in range(4):
            kb, ob, rb = spea2_ops.truncate(obj[b], mask[b], n_keep, return_order=True)
            assert same_bits(keep[b], kb) and same_bits(order[b], ob) and same_bits(rescans[b], rb), f"run {b}, mask {name}"
            assert same_bits(keep[b], spea2_ops.truncate(obj[b], mask[b], n_keep))
    idx = spea2_ops.select(obj, n_keep)
    assert idx.shape == (4, n_keep) and idx.dtype == torch.int64
    for b in range(4):
        assert same_bits(idx[b], spea2_ops.select(obj[b], n_keep)), f"run {b}: select"
