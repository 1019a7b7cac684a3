"""The fused planar rollout kernel on the constrained-root models (inverted_pendulum,
inverted_double_pendulum, reacher) against the torch engine.

Reference for every return comparison: ``PlanarChain`` + the batched MLP evaluated in **float64** on the
CPU from the same weights and initial state (never the kernel).  The bound on a return is that of
``test_planar_rollout_gpu.py``: the larger of ``rtol 2e-3, atol 2e-3·cap`` and 4× the largest error of the
**float32** CPU loop against that float64 reference on the same inputs.
"""
import functools

import pytest
import torch

from evoxmi import random as rnd
from evoxmi.models import MLPPolicy
from evoxmi.problems.neuroevolution import Brax
from evoxmi.problems.neuroevolution.reinforcement_learning import planar
from evoxmi.problems.neuroevolution.reinforcement_learning.envs import get_environment
from evoxmi.utils import TreeAndVector

pytestmark = pytest.mark.gpu

MODELS = ("inverted_pendulum", "inverted_double_pendulum", "reacher")


def _population(env, hidden, n, seed, scale=0.3):
    policy = MLPPolicy([env.obs_dim, hidden, hidden, env.act_dim])
    params = policy.init(rnd.PRNGKey(0))
    tv = TreeAndVector(params)
    v = tv.to_vector(params)
    pop = v + scale * torch.randn(n, v.numel(), generator=torch.Generator().manual_seed(seed))
    return policy, tv, pop


def _margin(env, s):
    """Distance of the quantity that decides health from its threshold (infinite where nothing but a
    non-finite state ends the episode)."""
    t = env.task
    if env.kind == "balance":
        return ((s[:, 2] + s[:, 3]).abs() - t["pitch_max"]).abs()
    if env.kind == "balance_tip":
        return (env.tip(s[:, :env.nd])[:, 1] - t["z_lo"]).abs()
    return torch.full_like(s[:, 0], float("inf"))


def _cpu_rollout(env, policy, tree, s0, cap, dtype):
    """Sticky-done returns, lengths and the smallest health margin seen up to the deciding step, with the
    torch engine in ``dtype`` on the CPU."""
    tree = torch.utils._pytree.tree_map(lambda x: x.to(dtype), tree)
    n = next(iter(tree.values()))["w"].shape[0]
    s = s0.to(dtype).expand(n, -1).clone()
    total = torch.zeros(n, dtype=dtype)
    steps = torch.full((n,), cap, dtype=torch.int32)
    margin = torch.full((n,), float("inf"), dtype=dtype)
    alive = torch.ones(n, dtype=torch.bool)
    for i in range(cap):
        s, _, r, done = env.step(s, policy(tree, env.obs(s)))
        margin = torch.where(alive, torch.minimum(margin, _margin(env, s)), margin)
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
#   (cap, hidden)   inverted_pendulum   inverted_double_pendulum   reacher
#   (1, 64)         0 / 0               8.9e-07 / 1.2e-06          7.8e-07 / 7.4e-07
#   (5, 64)         0 / 0               8.0e-06 / 8.2e-06          2.4e-05 / 9.7e-06
#   (20, 40)        0 / 0               3.1e-05 / 3.1e-05          8.8e-03 / 4.8e-03
#   (20, 96)        0 / 0               3.6e-05 / 9.5e-05          2.1e-03 / 1.6e-02
#   (5, 160)        0 / 0               7.0e-06 / 7.4e-06          9.2e-05 / 2.0e-04
# (the inverted pendulum's return counts healthy steps, so equal lengths make it exact; n = 1 and n = 5 are
# subsets of the same rows and never larger); termination test, compared rows: inverted_pendulum 0 / 0,
# inverted_double_pendulum 5.6e-03 / 1.3e-02; reacher targets 5.3e-06 / 4.2e-06 and 2.4e-05 / 2.5e-05;
# fused / generic / float32 CPU loop at cap 8: inverted_double_pendulum 2.2e-05 / 9.8e-06 / 9.3e-06, reacher
# 9.8e-06 / 2.0e-05 / 6.9e-06.
@pytest.mark.parametrize("n", [1, 5, 96])
@pytest.mark.parametrize("cap,hidden", [(1, 64), (5, 64), (20, 40), (20, 96), (5, 160)])
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


# initial states of the termination test: the first pole tilted and turning, chosen on the CPU so that the
# float64 reference ends episodes at several different steps and some rows survive
# (inverted_pendulum 4 … 29 with 12 of 64 rows surviving, inverted_double_pendulum 6 … 26 with 3 surviving) and
# excludes 3 and 0 rows of 64 by the 1e-3 health margin
TERMINATION = {"inverted_pendulum": dict(tilt=0.06, rate=0.3), "inverted_double_pendulum": dict(tilt=0.15, rate=0.5)}


@pytest.mark.parametrize("name", ["inverted_pendulum", "inverted_double_pendulum"])
def test_termination_inside_the_episode(name):
    from evoxmi.ops import neuro

    cap, hidden, n = 30, 64, 64
    env = get_environment(name)
    policy, tv, pop = _population(env, hidden, n, 7, scale=0.5)
    tree = tv.batched_to_tree(pop)
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0].clone()
    s0[3] = TERMINATION[name]["tilt"]
    s0[env.nd + 3] = TERMINATION[name]["rate"]
    ref, steps, margin = _cpu_rollout(env, policy, tree, s0, cap, torch.float64)
    f32, _, _ = _cpu_rollout(env, policy, tree, s0, cap, torch.float32)
    keep = margin >= 1e-3
    print(f"{name}: excluded {int((~keep).sum())} of {n}, reference lengths {sorted(set(steps.tolist()))}")
    assert int((~keep).sum()) <= n // 10
    assert bool((steps < cap).any()) and bool((steps == cap).any())
    assert int(steps.min()) >= 2 and len(set(steps.tolist())) >= 4
    out, length = neuro.planar_rollout(pop.cuda(), hidden, hidden, env.model_table(), s0.cuda(), cap)
    assert torch.equal(length.cpu()[keep], steps[keep])
    e32 = float((f32.double() - ref)[keep].abs().max())
    err = (out.cpu().double() - ref).abs()[keep]
    print(f"{name}: kernel {float(err.max()):.3e} float32-torch {e32:.3e}")
    assert bool((err <= _bound(ref[keep], cap, e32)).all()), (float(err.max()), e32)


def test_reacher_target_reaches_the_kernel():
    """The same weights and start pose with two different targets: different returns, each within the bound
    of its own reference."""
    from evoxmi.ops import neuro

    cap, hidden, n = 10, 64, 32
    env = get_environment("reacher")
    policy, tv, pop = _population(env, hidden, n, 11)
    tree = tv.batched_to_tree(pop)
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0]
    outs = []
    for target in ((0.15, -0.05), (-0.1, 0.12)):
        s = s0.clone()
        s[2 * env.nd:] = torch.tensor(target)
        ref, steps, _ = _cpu_rollout(env, policy, tree, s, cap, torch.float64)
        f32, _, _ = _cpu_rollout(env, policy, tree, s, cap, torch.float32)
        e32 = float((f32.double() - ref).abs().max())
        out, length = neuro.planar_rollout(pop.cuda(), hidden, hidden, env.model_table(), s.cuda(), cap)
        err = (out.cpu().double() - ref).abs()
        print(f"reacher target {target}: kernel {float(err.max()):.3e} float32-torch {e32:.3e}")
        assert torch.equal(length.cpu(), steps) and bool((err <= _bound(ref, cap, e32)).all()), (float(err.max()), e32)
        outs.append((out.cpu().double(), ref, _bound(ref, cap, e32)))
    # the targets lie 0.3 apart, so over 10 steps the distance term moves a return by up to 3, against a bound of
    # about 0.05: most returns under one target are outside the bound of the other target's reference
    (out_a, ref_a, bound_a), (out_b, ref_b, bound_b) = outs
    crossed = ((out_a - ref_b).abs() > bound_b) & ((out_b - ref_a).abs() > bound_a)
    print(f"reacher: {int(crossed.sum())} of {n} returns outside the other target's bound")
    assert int(crossed.sum()) > n // 2


@pytest.mark.parametrize("name", MODELS)
def test_fused_against_generic_capture_and_determinism(name):
    from evoxmi.algorithms import OpenES
    from evoxmi.ops import neuro
    from evoxmi.utils import rank_based_fitness
    from evoxmi.workflows import StdWorkflow

    env = get_environment(name)
    cap = 8
    policy, tv, pop = _population(env, 32, 64, 3)
    tree = torch.utils._pytree.tree_map(lambda x: x.cuda(), tv.batched_to_tree(pop))
    fits = []
    for fused in (True, False):
        prob = Brax(policy, name, cap, fused=fused)
        assert prob._fused_ok(tree) == fused
        fit, _ = prob.evaluate(prob.init(rnd.PRNGKey(5)), tree)
        fits.append(fit.cpu().double())
        if fused:
            lengths = prob.last_episode_lengths.cpu()
    # both are float32 evaluations of the same episodes: they differ by each one's own error
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0]
    ref, steps, margin = _cpu_rollout(env, policy, tv.batched_to_tree(pop), s0, cap, torch.float64)
    f32, _, _ = _cpu_rollout(env, policy, tv.batched_to_tree(pop), s0, cap, torch.float32)
    keep = margin >= 1e-3
    e32 = float((f32.double() - ref)[keep].abs().max())
    print(f"{name}: fused {float((fits[0] - ref)[keep].abs().max()):.3e} generic {float((fits[1] - ref)[keep].abs().max()):.3e} float32-torch {e32:.3e}")
    assert int((~keep).sum()) <= 64 // 10 and torch.equal(lengths[keep], steps[keep])
    for fit in fits:
        assert bool(((fit - ref).abs()[keep] <= _bound(ref[keep], cap, e32)).all())
    outs = []
    for graph in (False, True):
        pol = MLPPolicy([env.obs_dim, 32, 32, env.act_dim])
        params = pol.init(rnd.PRNGKey(1), device="cuda")
        tvg = TreeAndVector(params)
        prob = Brax(pol, name, 20)
        wf = StdWorkflow(OpenES(tvg.to_vector(params), 64, learning_rate=0.05, noise_stdev=0.1, optimizer="adam"), prob,
                         sol_transforms=[tvg.batched_to_tree], fit_transforms=[rank_based_fitness], opt_direction="max", graph=graph)
        st = wf.init(rnd.PRNGKey(3, device="cuda"))
        for _ in range(4):
            st = wf.step(st)
        assert (wf._graph is not None) == graph
        assert prob.last_episode_lengths.shape == (64,)
        outs.append(st.get_child_state("algorithm").center.clone())
    assert torch.allclose(outs[0], outs[1], rtol=1e-5, atol=1e-6)
    s0 = s0.cuda()
    a = neuro.planar_rollout(pop.cuda(), 32, 32, env.model_table(), s0, 20)
    b = neuro.planar_rollout(pop.cuda(), 32, 32, env.model_table(), s0, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_binding_rejects_a_wrong_init_and_an_uninstantiated_combination():
    from evoxmi.ops import neuro

    env = get_environment("reacher")
    s0 = env.reset(rnd.PRNGKey(5), 1)[0][0].cuda()
    tab = env.model_table()
    P = neuro.planar_param_count(env.obs_dim, 64, 64, env.act_dim)
    W = torch.zeros(2, P, device="cuda")
    with pytest.raises(RuntimeError, match="init state must have 12"):
        neuro.planar_rollout(W, 64, 64, tab, s0[:10], 3)  # q ++ u without the target
    with pytest.raises(RuntimeError, match="columns"):
        neuro.planar_rollout(torch.zeros(2, P + 1, device="cuda"), 64, 64, tab, s0, 3)
    # hopper's chain of 4 on an x-only root, a reach arm on an x-only root, a cart with a driven pole, and a
    # running model with a driven slider: no kernel is instantiated for any of them
    hopper_tab = get_environment("hopper").model_table()
    bad = [planar.PlanarChain(dict(planar.HOPPER, root_free=(1, 0, 0))).model_table(),
           planar.PlanarChain(dict(planar.REACHER, root_free=(1, 0, 0))).model_table(),
           planar.PlanarChain(dict(planar.INVERTED_PENDULUM, hinges=(dict(planar.INVERTED_PENDULUM["hinges"][0], gear=10.0),))).model_table(),
           planar.PlanarChain(dict(planar.HOPPER, root_gear=(5.0, 0.0, 0.0))).model_table()]
    assert not torch.equal(bad[3], hopper_tab)
    for t in bad:
        with pytest.raises(RuntimeError, match="combination"):
            neuro.planar_rollout(W, 64, 64, t, s0, 3)
    out, length = neuro.planar_rollout(torch.zeros(0, P, device="cuda"), 64, 64, tab, s0, 3)
    assert out.shape == (0,) and length.shape == (0,) and length.dtype == torch.int32
