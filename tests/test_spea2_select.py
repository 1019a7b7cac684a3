"""``evoxmi.ops.spea2`` on the CPU: the torch path is bit for bit what SPEA2 computed before the ops module,
and the float64 references of ``_spea2_reference.py`` (used by the GPU tests) state the same rule as
``truncation``."""
import numpy as np
import pytest
import torch

import _spea2_reference as ref
from evoxmi.ops import spea2 as spea2_ops


def _frozen_tell_selection(merged_fit, pop_size):
    """SPEA2.tell's eager selection as it was written out before ``evoxmi.ops.spea2`` (a frozen copy)."""
    sig = spea2_ops.cal_fitness(merged_fit)
    mask = sig < 1
    num_valid = int(mask.sum())
    if num_valid <= pop_size:
        order = torch.argsort(sig, stable=True)
    else:
        keep = spea2_ops.truncation(merged_fit, num_valid - pop_size, mask)
        order = torch.argsort((~keep).to(torch.int64), stable=True)
    return order[:pop_size], num_valid


CASES = [(200, 3, "uniform", 100), (200, 3, "front", 100), (130, 5, "front", 64), (257, 2, "uniform", 20), (64, 2, "front", 63)]


@pytest.mark.parametrize("n,m,kind,n_keep", CASES)
def test_cpu_entries_are_the_torch_path_bit_for_bit(n, m, kind, n_keep):
    obj = torch.from_numpy(ref.objectives(n, m, kind, seed=3))
    sig = spea2_ops.fitness(obj)
    assert torch.equal(sig.view(torch.int32), spea2_ops.cal_fitness(obj).view(torch.int32))
    want, num_valid = _frozen_tell_selection(obj, n_keep)
    assert (num_valid > n_keep) == (kind == "front"), "the case no longer covers the branch it is here for"
    got = spea2_ops.select(obj, n_keep)
    assert got.dtype == torch.int64 and torch.equal(got, want)


def test_parts_add_up_and_equal_the_reference():
    obj = torch.from_numpy(ref.objectives(200, 3, "uniform", seed=5))
    sig, S, R, D, nd = spea2_ops.fitness(obj, return_parts=True)
    assert torch.equal(sig, spea2_ops.cal_fitness(obj)) and torch.equal(sig, D + R)
    S64, nd64, R64, D64 = ref.fitness_parts(obj.numpy())
    assert np.array_equal(S.numpy(), S64) and np.array_equal(nd.numpy(), nd64) and np.array_equal(R.numpy(), R64.astype(np.float32))
    assert np.allclose(D.numpy(), D64, rtol=1e-4, atol=0)  # cdist's float32 against float64
    assert torch.equal(sig < 1, nd)


def test_truncate_entry_is_truncation():
    obj = torch.from_numpy(ref.objectives(100, 3, "front", seed=1))
    mask = torch.ones(100, dtype=torch.bool)
    mask[::7] = False
    count = int(mask.sum())
    keep, order, n_rescans = spea2_ops.truncate(obj, mask, 40, return_order=True)
    assert torch.equal(keep, spea2_ops.truncation(obj, count - 40, mask)) and torch.equal(keep, spea2_ops.truncate(obj, mask, 40))
    assert order.shape == (60,) and int(n_rescans) == 0
    removed = order[: count - 40]
    assert bool((order[count - 40:] == -1).all()) and bool(mask[removed].all()) and not bool(keep[removed].any())
    assert int(keep.sum()) == 40
    # count ≤ n_keep: nothing leaves
    assert torch.equal(spea2_ops.truncate(obj, mask, count), mask)


GRID = [(17, 2, 0), (64, 2, 1), (100, 3, 2), (257, 3, 3)]


@pytest.mark.parametrize("n,m,seed", GRID)
def test_dense_reference_agrees_with_truncation_on_exact_inputs(n, m, seed):
    """On a coarse dyadic grid every d2 is exact in float32 (and in cdist's matrix-product form), so the float32
    torch loop and the float64 rule must remove the same rows in the same order."""
    obj = np.unique(ref.objectives(n, m, "grid", seed), axis=0)  # distinct points: the sqrt in cdist keeps their order
    rng = np.random.default_rng(seed)
    obj = obj[rng.permutation(obj.shape[0])]
    n = obj.shape[0]
    mask = rng.random(n) < 0.8
    k = int(mask.sum()) // 2
    want = ref.dense_truncation(obj, mask, k)
    keep, order, _ = spea2_ops.truncate(torch.from_numpy(obj), torch.from_numpy(mask), int(mask.sum()) - k, return_order=True)
    assert np.array_equal(order[:k].numpy(), want)
    expect = mask.copy()
    expect[want] = False
    assert np.array_equal(keep.numpy(), expect)


@pytest.mark.parametrize("n,m,kind", [(64, 2, "front"), (200, 3, "front"), (257, 3, "uniform"), (257, 5, "front"), (100, 3, "grid")])
def test_incremental_reference_equals_the_dense_one(n, m, kind):
    obj = ref.objectives(n, m, kind, seed=7)
    mask = np.ones(n, dtype=bool)
    if kind != "uniform":
        mask[3::11] = False
    k = int(mask.sum()) - max(1, n // 3)
    dense = ref.dense_truncation(obj, mask, k)
    inc, gap, pairs, rescans = ref.incremental_truncation(obj, mask, k)
    assert np.array_equal(inc, dense)
    assert rescans >= 1 and gap >= 0
    assert ref.replay_slack(obj, mask, dense) == 1.0


def test_incremental_reference_on_duplicates_and_nonfinite():
    obj = ref.objectives(40, 3, "front", seed=9).copy()
    obj[10:20] = obj[5]  # a block of duplicates
    obj[30, 1] = np.inf
    obj[31, 0] = np.nan
    mask = np.ones(40, dtype=bool)
    mask[31] = False
    dense = ref.dense_truncation(obj, mask, 30)
    inc = ref.incremental_truncation(obj, mask, 30)[0]
    assert np.array_equal(inc, dense)
    assert dense[:10].tolist() == [5] + list(range(10, 19))  # duplicates leave lowest index first, one stays


def test_earlier_names_still_import_from_the_algorithm_module():
    from evoxmi.algorithms.mo import spea2 as algo

    assert algo.cal_fitness is spea2_ops.cal_fitness
    assert algo.truncation is spea2_ops.truncation
    assert algo.truncation_predicated is spea2_ops.truncation_predicated
    assert spea2_ops.N_CAP == 8192 and spea2_ops.M_CAP == 16
    assert not spea2_ops.on_device(100, 3, "cpu")
