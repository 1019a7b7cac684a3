"""The fused planar rollout kernel (``ops.neuro.planar_rollout``) against the torch engine.

Reference for every return comparison: ``PlanarChain`` + the batched MLP evaluated in
**float64** on the CPU from the same weights and initial state (never the kernel).  The bound on
a return is the larger of the Ant test's ``rtol 2e-3, atol 2e-3·cap`` and 4× the largest error of
the **float32** CPU loop against that float64 reference on the same inputs (an independent
evaluation at the kernel's precision; the factor 4 allows for a different summation order).
"""
import functools

import pytest
import torch

from evoxmi import random as rnd
from evoxmi.models import MLPPolicy
from evoxmi.problems.neuroevolution import Brax
from evoxmi.problems.neuroevolution.reinforcement_learning.envs import get_environment
from evoxmi.utils import TreeAndVector

pytestmark = pytest.mark.gpu

MODELS = ("hopper", "walker2d", "halfcheetah", "swimmer")


def _population(env, hidden, n, seed, scale=0.3):
    policy = MLPPolicy([env.obs_dim, hidden, hidden, env.act_dim])
    params = policy.init(rnd.PRNGKey(0))
    tv = TreeAndVector(params)
    v = tv.to_vector(params)
    pop = v + scale * torch.randn(n, v.numel(), generator=torch.Generator().manual_seed(seed))
    return policy, tv, pop


def _cpu_rollout(env, policy, tree, s0, cap, dtype):
    """Sticky-done returns, lengths and the smallest health margin seen up to the deciding step
    (distance of z or |θ| from its threshold), with the torch engine in ``dtype`` on the CPU."""
    tree = torch.utils._pytree.tree_map(lambda x: x.to(dtype), tree)
    n = next(iter(tree.values()))["w"].shape[0]
    s = s0.to(dtype).expand(n, -1).clone()
    t = env.spec["task"]
    total = torch.zeros(n, dtype=dtype)
    steps = torch.full((n,), cap, dtype=torch.int32)
    margin = torch.full((n,), float("inf"), dtype=dtype)
    alive = torch.ones(n, dtype=torch.bool)
    for i in range(cap):
        s, _, r, done = env.step(s, policy(tree, env.obs(s)))
        m = torch.stack([(s[:, 1] - t["z_lo"]).abs(), (s[:, 1] - t["z_hi"]).abs(), (s[:, 2].abs() - t["pitch_max"]).abs()]).amin(0)
        margin = torch.where(alive, torch.minimum(margin, m), margin)
        steps = torch.where(alive & done, torch.full_like(steps, i), steps)
        alive = alive & ~done
        total = total + alive.to(dtype) * r
    return total, steps, margin


@functools.lru_cache(maxsize=None)
def _case(name, cap, hidden):
    env = get_environment(name)
    policy, tv, pop = _population(env, hidden, 96, cap)
    tree = tv.batched_to_tree(pop)
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0]
    ref, steps, _ = _cpu_rollout(env, policy, tree, s0, cap, torch.float64)
    f32, _, _ = _cpu_rollout(env, policy, tree, s0, cap, torch.float32)
    return env, policy, pop, s0, ref, steps, float((f32.double() - ref).abs().max())


def _bound(ref, cap, e32):
    return torch.maximum(2e-3 * ref.abs() + 2e-3 * cap, torch.full_like(ref, 4 * e32))


# Observed on an MI355X, largest |return − float64 reference| at n = 96: kernel / float32 CPU loop
#   (cap, hidden)   hopper              walker2d            halfcheetah         swimmer
#   (1, 64)         1.9e-07 / 1.6e-07   2.1e-07 / 3.3e-07   1.7e-07 / 1.9e-07   1.6e-07 / 2.2e-07
#   (5, 64)         6.3e-06 / 5.8e-06   6.8e-06 / 1.3e-05   1.4e-05 / 2.0e-05   3.7e-06 / 1.1e-05
#   (20, 40)        5.9e-05 / 7.0e-05   3.4e-03 / 3.8e-04   4.7e-03 / 1.6e-03   1.7e-03 / 3.9e-03
#   (20, 96)        2.5e-03 / 1.4e-03   7.9e-04 / 1.0e-03   1.8e-01 / 2.7e-01   7.8e-04 / 3.0e-03
# (n = 1 and n = 5 are subsets of the same rows and never larger); termination test, compared rows:
# hopper 1.8e-04 / 4.0e-04, walker2d 1.8e+00 / 1.3e+00 (contact-rich falls amplify rounding: there, as in
# halfcheetah (20, 96), the 4 × float32 clause sets the bound and the lengths carry the comparison);
# long episodes: population mean −78.51 against the reference's −75.21 (bound 0.05·mean|ref| + 1 = 4.8).
@pytest.mark.parametrize("n", [1, 5, 96])
@pytest.mark.parametrize("cap,hidden", [(1, 64), (5, 64), (20, 40), (20, 96)])
@pytest.mark.parametrize("name", MODELS)
def test_returns_and_lengths_match_float64_reference(name, cap, hidden, n):
    from evoxmi.ops import neuro

    env, policy, pop, s0, ref, steps, e32 = _case(name, cap, hidden)
    out, length = neuro.planar_rollout(pop[:n].cuda(), hidden, hidden, env.model_table(), s0.cuda(), cap)
    assert out.shape == (n,) and out.dtype == torch.float32 and length.shape == (n,) and length.dtype == torch.int32
    err = (out.cpu().double() - ref[:n]).abs()
    print(f"{name} cap={cap} hidden={hidden} n={n}: kernel {float(err.max()):.3e} float32-torch {e32:.3e}")
    assert torch.equal(length.cpu(), steps[:n])
    assert bool((err <= _bound(ref[:n], cap, e32)).all()), (float(err.max()), e32)


# initial states of the termination test: root pitched towards its limit with a pitch rate, chosen on
# the CPU so that the float64 reference ends episodes at many different steps (hopper 2 … 29, walker2d
# 7 … 27, some rows surviving) and excludes 1 row of 64 for each model by the 1e-3 health margin
TERMINATION = {"hopper": dict(pitch=0.14, rate=0.2), "walker2d": dict(pitch=0.4, rate=0.8)}


@pytest.mark.parametrize("name", ["hopper", "walker2d"])
def test_termination_inside_the_episode(name):
    from evoxmi.ops import neuro

    cap, hidden, n = 30, 64, 64
    env = get_environment(name)
    policy, tv, pop = _population(env, hidden, n, 7, scale=0.5)
    tree = tv.batched_to_tree(pop)
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0].clone()
    s0[2] = TERMINATION[name]["pitch"]
    s0[env.nd + 2] = TERMINATION[name]["rate"]
    ref, steps, margin = _cpu_rollout(env, policy, tree, s0, cap, torch.float64)
    f32, _, _ = _cpu_rollout(env, policy, tree, s0, cap, torch.float32)
    keep = margin >= 1e-3
    print(f"{name}: excluded {int((~keep).sum())} of {n}, reference lengths {sorted(set(steps.tolist()))}")
    assert int((~keep).sum()) <= n // 10
    assert bool((steps < cap).any()) and bool((steps == cap).any())
    assert int(steps.min()) >= 2
    out, length = neuro.planar_rollout(pop.cuda(), hidden, hidden, env.model_table(), s0.cuda(), cap)
    assert torch.equal(length.cpu()[keep], steps[keep])
    e32 = float((f32.double() - ref)[keep].abs().max())
    err = (out.cpu().double() - ref).abs()[keep]
    print(f"{name}: kernel {float(err.max()):.3e} float32-torch {e32:.3e}")
    assert bool((err <= _bound(ref[keep], cap, e32)).all()), (float(err.max()), e32)


def test_fallback_outside_the_fused_case():
    env = get_environment("hopper")

    def run(policy, dtype=torch.float32):
        params = policy.init(rnd.PRNGKey(0))
        tree = torch.utils._pytree.tree_map(lambda x: x[None].expand(4, *x.shape).to(device="cuda", dtype=dtype).contiguous(), params)
        prob = Brax(policy, "hopper", 5)
        out, _ = prob.evaluate(prob.init(rnd.PRNGKey(5)), tree)
        return prob._fused_ok(tree), out

    ok, out = run(MLPPolicy([env.obs_dim, 64, 64, env.act_dim]))
    assert ok and torch.isfinite(out).all()
    for policy, dtype in ((MLPPolicy([env.obs_dim, 64, env.act_dim]), torch.float32),
                          (MLPPolicy([env.obs_dim, 64, 64, env.act_dim], activation="relu"), torch.float32),
                          (MLPPolicy([env.obs_dim, 600, 600, env.act_dim]), torch.float32),
                          (MLPPolicy([env.obs_dim, 256, 256, env.act_dim]), torch.float32),  # within hidden ≤ 512, over one wave's LDS
                          (MLPPolicy([env.obs_dim, 64, 64, env.act_dim]), torch.float64)):
        ok, out = run(policy, dtype)
        assert not ok and out.is_cuda and out.shape == (4,) and torch.isfinite(out).all()


def test_binding_rejects_what_is_outside_the_caps():
    from evoxmi.ops import neuro

    env = get_environment("hopper")
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0].cuda()
    tab = env.model_table()
    P = neuro.planar_param_count(env.obs_dim, 64, 64, env.act_dim)
    with pytest.raises(RuntimeError, match="hidden sizes"):
        neuro.planar_rollout(torch.zeros(2, P, device="cuda"), 600, 64, tab, s0, 3)
    with pytest.raises(RuntimeError, match="columns"):
        neuro.planar_rollout(torch.zeros(2, P + 1, device="cuda"), 64, 64, tab, s0, 3)
    bad = tab.clone()
    bad[24 + 16 * 2] = 0.0  # body 2 hangs on the root: a tree shape with no instantiated kernel
    with pytest.raises(RuntimeError, match="tree shape"):
        neuro.planar_rollout(torch.zeros(2, P, device="cuda"), 64, 64, bad, s0, 3)
    out, length = neuro.planar_rollout(torch.zeros(0, P, device="cuda"), 64, 64, tab, s0, 3)
    assert out.shape == (0,) and length.shape == (0,) and length.dtype == torch.int32


def test_capture_and_determinism():
    from evoxmi.algorithms import OpenES
    from evoxmi.ops import neuro
    from evoxmi.utils import rank_based_fitness
    from evoxmi.workflows import StdWorkflow

    env = get_environment("hopper")
    outs = []
    for graph in (False, True):
        policy = MLPPolicy([env.obs_dim, 32, 32, env.act_dim])
        params = policy.init(rnd.PRNGKey(1), device="cuda")
        tv = TreeAndVector(params)
        prob = Brax(policy, "hopper", 40)
        wf = StdWorkflow(OpenES(tv.to_vector(params), 64, learning_rate=0.05, noise_stdev=0.1, optimizer="adam"), prob,
                         sol_transforms=[tv.batched_to_tree], fit_transforms=[rank_based_fitness], opt_direction="max", graph=graph)
        st = wf.init(rnd.PRNGKey(3, device="cuda"))
        for _ in range(4):
            st = wf.step(st)
        assert (wf._graph is not None) == graph
        assert prob.last_episode_lengths.shape == (64,)
        outs.append(st.get_child_state("algorithm").center.clone())
    assert torch.allclose(outs[0], outs[1], rtol=1e-5, atol=1e-6)
    _, _, pop = _population(env, 32, 64, 3)
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0].cuda()
    a = neuro.planar_rollout(pop.cuda(), 32, 32, env.model_table(), s0, 40)
    b = neuro.planar_rollout(pop.cuda(), 32, 32, env.model_table(), s0, 40)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_long_episode_statistics():
    from evoxmi.ops import neuro

    env = get_environment("halfcheetah")
    policy, tv, pop = _population(env, 32, 256, 0, scale=0.2)
    s0 = env.reset(rnd.PRNGKey(2), 1)[0][0]
    ref, _, _ = _cpu_rollout(env, policy, tv.batched_to_tree(pop), s0, 300, torch.float64)
    out, _ = neuro.planar_rollout(pop.cuda(), 32, 32, env.model_table(), s0.cuda(), 300)
    # chaotic dynamics: individual returns may diverge late in the episode, the population statistics must not
    print(f"halfcheetah cap 300: kernel mean {float(out.mean()):.4f} reference mean {float(ref.mean()):.4f}")
    assert torch.isfinite(out).all()
    assert abs(float(out.mean()) - float(ref.mean())) < 0.05 * float(ref.abs().mean()) + 1.0
