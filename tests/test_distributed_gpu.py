"""Multi-process SPMD paths with the HIP kernels in the loop (MI355X, marked gpu).

The pool's boxes have one GPU, and RCCL refuses two ranks on one device, so these
tests run 2 ranks on ``cuda:0`` with the gloo backend (gloo stages CUDA tensors through
the host).  They exercise exactly the sharded code that the 8-GPU RCCL runs use —
rank-local Philox rows, the fused kernels, the all-gathers / all-reduces — and compare
with the single-process result.  The RCCL collectives themselves, captured in the
hipGraph, are covered by ``bench.py --force-dist`` under torchrun on one GPU.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make(kind):
    from evoxmi.algorithms import CMAES, OpenES
    from evoxmi.problems.numerical import CEC2022TestSuit, Sphere
    from evoxmi.workflows import StdWorkflow

    if kind == "cmaes":
        d = 64
        alg = CMAES(torch.linspace(-3, 3, d, device="cuda"), init_stdev=2.0, pop_size=512)
        return StdWorkflow(alg, CEC2022TestSuit.create(1))
    if kind == "flagship":  # bench.py's config: each of 2 ranks samples / evaluates 5000 rows (192-row f16x3 tiles)
        center = (torch.rand(1000, generator=torch.Generator().manual_seed(1)) * 160 - 80).cuda()
        return StdWorkflow(CMAES(center_init=center, init_stdev=20.0, pop_size=10000), CEC2022TestSuit.create(1))
    alg = OpenES(torch.full((40,), 1.0, device="cuda"), 256, learning_rate=0.05, noise_stdev=0.2, optimizer="adam")
    return StdWorkflow(alg, Sphere())


def _field(kind):
    return "mean" if kind in ("cmaes", "flagship") else "center"


def _worker(rank, world, port, kind, gens, out, seed=3):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from evoxmi import random as rnd
    from evoxmi.parallel import destroy, init_distributed

    init_distributed(backend="gloo")
    torch.cuda.set_device(0)
    wf = _make(kind)
    st = wf.init(rnd.PRNGKey(seed, device="cuda"))
    st = wf.enable_distributed(st)
    for _ in range(gens):
        st = wf.step(st)
    torch.cuda.synchronize()
    alg = st.get_child_state("algorithm")
    out[rank] = alg[_field(kind)].cpu()
    if kind in ("cmaes", "flagship"):
        out[("sigma", rank)] = alg["sigma"].cpu()
        out[("C", rank)] = alg["C"].cpu()
    destroy()


# CMA-ES: one generation (afterwards the Jacobi eigenbasis of the clustered spectrum
# amplifies rounding-level differences of the all-reduced statistics into different
# — equally valid — sample rotations, so longer runs are compared replica-to-replica only)
@pytest.mark.parametrize("kind,gens", [("cmaes", 1), ("cmaes", 5), ("openes", 8), ("flagship", 1)])
def test_sharded_two_ranks_on_gpu_match_single_process(kind, gens):
    from evoxmi import random as rnd

    wf = _make(kind)
    st = wf.init(rnd.PRNGKey(3, device="cuda"))
    for _ in range(gens):
        st = wf.step(st)
    ref = st.get_child_state("algorithm")[_field(kind)].cpu()
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), kind, gens, out), nprocs=2, join=True)
    assert torch.equal(out[0], out[1])  # replicas stay bit-identical
    if kind in ("cmaes", "flagship"):
        # the covariance too: a wrong element of the packed all-reduce reaches the mean only a generation later
        assert torch.equal(out[("C", 0)], out[("C", 1)])
    if kind == "cmaes" and gens > 1:
        return
    if kind == "flagship":
        # the shard's 5000-row sampling / rotation products on the shorter f16x3 tiles, the packed
        # rank-μ all-reduce: the same population rows (Philox row offsets), sums in another order
        assert torch.equal(out[("sigma", 0)], out[("sigma", 1)])
        assert torch.allclose(out[0], ref, rtol=1e-4, atol=1e-4), float((out[0] - ref).abs().max())
        return
    # reduction order differs from the single process (rank partial sums + all-reduce)
    assert torch.allclose(out[0], ref, rtol=1e-3, atol=1e-3)


def test_sharded_cmaes_tracks_single_process_over_many_generations():
    """Longer CMA-ES runs (30 generations): the 2-rank replicas stay bit-identical, and the
    sharded run follows the single process statistically — over three seeds, the median step
    size within 20 % and the median progress on f(mean) in decades within 15 % (the eigenbasis of
    a clustered spectrum turns rounding-level differences of the all-reduced statistics into
    different, equally valid sample rotations, so the runs are not compared bit for bit, and one
    seed alone swings by ≈20 %: 10.2 vs 8.6 decades on seed 3 in round 6)."""
    import math
    import statistics

    from evoxmi import random as rnd

    gens = 30
    sig_ratio, dec_ratio = [], []
    for seed in (3, 4, 5):
        wf = _make("cmaes")
        st = wf.init(rnd.PRNGKey(seed, device="cuda"))
        f0 = float(wf.problem.evaluate(None, st.get_child_state("algorithm")["mean"][None, :])[0][0])
        for _ in range(gens):
            st = wf.step(st)
        alg = st.get_child_state("algorithm")
        ref_mean, ref_sigma = alg["mean"], float(alg["sigma"])
        mgr = mp.get_context("spawn").Manager()
        out = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), "cmaes", gens, out, seed), nprocs=2, join=True)
        assert torch.equal(out[0], out[1]) and torch.equal(out[("sigma", 0)], out[("sigma", 1)])
        assert torch.equal(out[("C", 0)], out[("C", 1)])
        f_ref = float(wf.problem.evaluate(None, ref_mean[None, :])[0][0])
        f_sh = float(wf.problem.evaluate(None, out[0].cuda()[None, :])[0][0])
        assert f_ref < f0 and f_sh < f0
        sig_ratio.append(float(out[("sigma", 0)]) / ref_sigma)
        dec_ratio.append(math.log10(f0 / f_sh) / math.log10(f0 / f_ref))
    assert abs(statistics.median(sig_ratio) - 1.0) < 0.2, sig_ratio
    assert abs(statistics.median(dec_ratio) - 1.0) < 0.15, dec_ratio
