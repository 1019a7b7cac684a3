"""BatchedRuns over NSGA-III on the CPU: every run equals the solo run from ``run_keys(key)[r]`` bit for bit (under ``vmap`` the tell's
selection goes run by run through ``evoxmi_py::nsga3_survivors_run``), and the float32 torch path of ``ops.nsga3.associate`` against
the float64 host reference of ``_nsga3_reference.py``."""
import numpy as np
import torch

import _nsga3_reference as ref64
from evoxmi import random as rnd
from evoxmi.algorithms.containers.batched import BatchedRuns
from evoxmi.algorithms.mo.nsga3 import NSGA3
from evoxmi.operators.selection import non_dominated_sort
from evoxmi.ops import nsga3 as nsga3_ops
from evoxmi.problems.numerical import DTLZ2
from test_batched_mo import D, M, POP, RUNS, run


def check_runs_equal_solo(dev):
    make = lambda: NSGA3(torch.zeros(D, device=dev), torch.ones(D, device=dev), M, POP)
    prob, key = DTLZ2(d=D, m=M), rnd.PRNGKey(5, device=dev)
    pst, b = prob.init(rnd.PRNGKey(1, device=dev)), BatchedRuns(make(), RUNS)
    bst = run(b, key, prob, pst, RUNS)
    assert bst.runs.population.shape == (RUNS, POP, D) and bst.runs.fitness.shape == (RUNS, POP, M)
    for r, k in enumerate(b.run_keys(key)):
        sst = run(make(), k, prob, pst)
        assert torch.equal(bst.runs.population[r], sst.population), f"run {r}: population differs"
        assert torch.equal(bst.runs.fitness[r], sst.fitness), f"run {r}: fitness differs"
    assert not torch.equal(bst.runs.population[0], bst.runs.population[1])


def test_batched_nsga3_runs_equal_solo_cpu():
    check_runs_equal_solo("cpu")


def test_torch_path_against_reference():
    """float32 bounds: cos carries ε = 2(m + 3)·2⁻²⁴, so sqrt(1 − cos²) is off by min(ε / sinθ, √ε); the nadir by cond(E)·8m·2⁻²⁴."""
    n, K, m, N = 65, 66, 3, 32
    g = torch.Generator().manual_seed(7)
    f = torch.rand(n, m, generator=g) + 1e-3
    for j in range(m):
        f[j * n // m] = 0.01 + (0.99 + 0.1 * j) * torch.eye(m)[j]
    ref = torch.rand(K, m, generator=g) + 0.05
    rank = non_dominated_sort(f, until=N + 1)
    last_rank, group, group_dist, scale = nsga3_ops.associate(f, rank, ref, N)
    want = ref64.associate(f.numpy(), rank.numpy(), ref.numpy(), N)
    assert want["cond"] <= 100 and not want["used_worst"]
    assert int(last_rank) == want["last_rank"] and np.array_equal(scale[0].numpy(), want["ideal"])
    rel = want["cond"] * 8 * m * 2.0**-24
    assert np.all(np.abs(scale[1].numpy() - want["nadir"]) <= rel * want["nadir"])
    eps, xn = 2 * (m + 3) * 2.0**-24, want["xnorm"]
    sin = np.maximum(want["dmin"] / xn, 1e-30)
    tol = xn * (np.minimum(eps / sin, np.sqrt(eps)) + rel + 2.0**-23)
    assert np.all(np.abs(group_dist.numpy() - want["dmin"]) <= tol)
    assert np.all(want["dist_to"](group.numpy()) - want["dmin"] <= 2 * tol)
    # (B, n, m) is the 2-D call run by run
    for got, one in zip(nsga3_ops.associate(torch.stack([f, f]), torch.stack([rank, rank]), ref, N), (last_rank, group, group_dist, scale)):
        assert torch.equal(got[1], one)
