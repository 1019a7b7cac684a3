"""The planar engine with a constrained root (``PlanarChain`` with ``root_free``, a driven root slider,
passive hinges, task kinds and auxiliary state) and the inverted_pendulum, inverted_double_pendulum and
reacher environments on it: resolution, the reduced mass matrix against autograd, the constraints, energy
and momentum, behaviour, the reacher's target, actions, the kernel's model table, learning and the
fused case."""
import math
import os

import numpy as np
import pytest
import torch

from evoxmi import random as rnd
from evoxmi.algorithms import OpenES
from evoxmi.models import MLPPolicy
from evoxmi.problems.neuroevolution import Brax
from evoxmi.problems.neuroevolution.reinforcement_learning import planar
from evoxmi.problems.neuroevolution.reinforcement_learning.envs import get_environment
from evoxmi.utils import TreeAndVector, rank_based_fitness
from evoxmi.workflows import StdWorkflow

MODELS = ("inverted_pendulum", "inverted_double_pendulum", "reacher")
GYM = ("InvertedPendulum-v4", "InvertedDoublePendulum-v4", "Reacher-v4")
DIMS = {"inverted_pendulum": (4, 1), "inverted_double_pendulum": (8, 1), "reacher": (11, 2)}
OLD = ("hopper", "walker2d", "halfcheetah", "swimmer")


@pytest.mark.parametrize("name,spelling", [(n, s) for n, g in zip(MODELS, GYM) for s in (n, g)])
def test_names_resolve_through_brax(name, spelling):
    obs_dim, act_dim = DIMS[name]
    prob = Brax(MLPPolicy([obs_dim, 8, 8, act_dim]), spelling, 10)
    env = prob.env
    assert type(env) is type(get_environment(spelling)) and isinstance(env, planar.PlanarChain)
    assert (env.obs_dim, env.act_dim) == (obs_dim, act_dim)
    assert env.state_dim == 2 * env.nd + (2 if name == "reacher" else 0)
    s, o = env.reset(rnd.PRNGKey(0), 3)
    assert s.shape == (3, env.state_dim) and o.shape == (3, obs_dim) and torch.equal(s[0], s[1]) and torch.equal(s[0], s[2])
    s2, o2, r, d = env.step(s, torch.zeros(3, act_dim))
    assert s2.shape == s.shape and o2.shape == o.shape and r.shape == (3,) and d.shape == (3,) and d.dtype == torch.bool
    assert torch.isfinite(s2).all() and torch.isfinite(o2).all() and torch.isfinite(r).all()
    tree = torch.utils._pytree.tree_map(lambda x: x[None].expand(3, *x.shape), prob.policy.init(rnd.PRNGKey(1)))
    fit, _ = prob.evaluate(prob.init(rnd.PRNGKey(2)), tree)  # the generic loop carries the auxiliary words
    assert fit.shape == (3,) and torch.isfinite(fit).all()


def _random_state(env, n, seed):
    """q, u in float64 with the locked coordinates at root_init and at rest."""
    g = torch.Generator().manual_seed(seed)
    q = 0.5 * torch.randn(n, env.nd, generator=g, dtype=torch.float64)
    u = torch.randn(n, env.nd, generator=g, dtype=torch.float64)
    for i in range(3):
        if not env.root_free[i]:
            q[:, i] = env.spec["root_init"][i]
            u[:, i] = 0.0
    return q, u


@pytest.mark.parametrize("name", MODELS)
def test_reduced_mass_matrix_and_velocity_products_match_autograd(name):
    """M[F, F] is the Hessian in u_F of the kinetic energy with the locked velocities at 0, and the closed-form
    ∂T/∂q equals autograd's on the free coordinates (T assembled independently from the link velocities)."""
    env = get_environment(name)
    F = list(env.free)
    q, u = _random_state(env, 4, 0)
    M = env.mass_matrix(q)[:, F][:, :, F]
    for n in range(4):
        def T(uf):
            full = torch.zeros(env.nd, dtype=torch.float64).index_copy(0, torch.tensor(F), uf)
            return env.kinetic_energy(q[n:n + 1], full[None])[0]

        hess = torch.autograd.functional.hessian(T, u[n, F].clone())
        torch.testing.assert_close(M[n], hess, rtol=1e-10, atol=1e-12)
    qg = q.clone().requires_grad_(True)
    gq, = torch.autograd.grad(env.kinetic_energy(qg, u).sum(), [qg])
    torch.testing.assert_close(env.dTdq(q, u)[:, F], gq[:, F], rtol=1e-10, atol=1e-10)
    # the momenta of the free coordinates: M[F, F] u_F
    torch.testing.assert_close(env.momenta(q, u)[:, F], (M @ u[:, F, None])[..., 0], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", MODELS)
def test_locked_coordinates_hold_exactly(name, dtype):
    env = get_environment(name)
    s, _ = env.reset(rnd.PRNGKey(0), 4)
    s = s.to(dtype)
    locked = [i for i in range(3) if not env.root_free[i]]
    assert locked and all(float(s[0, i]) == env.spec["root_init"][i] and float(s[0, env.nd + i]) == 0.0 for i in locked)
    q0 = s[:, locked].clone()
    g = torch.Generator().manual_seed(2)
    moved = s[:, list(env.free)].clone()
    for _ in range(200):
        s, _, _, _ = env.step(s, (torch.rand(4, env.act_dim, generator=g) * 2 - 1).to(dtype))
        assert torch.equal(s[:, locked], q0)  # bit for bit
        assert bool((s[:, [env.nd + i for i in locked]] == 0).all())
    assert float((s[:, list(env.free)] - moved).abs().max()) > 0.1  # the free ones did move


def _energy(env, s):
    """Kinetic plus gravitational energy."""
    q, u = s[:, :env.nd], s[:, env.nd:2 * env.nd]
    return env.kinetic_energy(q, u) + env.spec["gravity"] * (env._c(q)["mass"] * env._kin(q)["cm"][..., 1]).sum(1)


def _conservative(name, dt, substeps):
    """The model unforced: no joint or slider damping, no limit springs, no stiffness."""
    hinges = tuple(dict(h, damping=0.0, limit_k=0.0, stiffness=0.0) for h in get_environment(name).spec["hinges"])
    return get_environment(name, dt=dt, substeps=substeps, hinges=hinges, lin_damp=0.0, root_slider=None)


# observed: ratio 4.02 / 4.96 / 4.00 (first order), cart momentum drift 2e-14 / 6e-14 of 6.3 / 7.1
@pytest.mark.parametrize("name", MODELS)
def test_energy_error_is_first_order_and_cart_momentum_is_conserved(name):
    worst = []
    for dt, substeps in ((1e-3, 10), (0.25e-3, 40)):  # the same physical time: 100 control steps of 10 ms
        env = _conservative(name, dt, substeps)
        s = torch.zeros(1, env.state_dim, dtype=torch.float64)
        s[0, 3:env.nd] = torch.tensor([0.3, -0.2][:env.nj], dtype=torch.float64)
        s[0, env.nd + 3:2 * env.nd] = torch.tensor([1.0, -2.0][:env.nj], dtype=torch.float64)
        if env.root_free[0]:
            s[0, env.nd] = 0.5
        e0, p0 = float(_energy(env, s)), float(env.momentum(s)[0][0, 0])
        de = dp = 0.0
        for _ in range(100):
            s, _, _, _ = env.step(s, torch.zeros(1, env.act_dim, dtype=torch.float64))
            de = max(de, abs(float(_energy(env, s)) - e0))
            dp = max(dp, abs(float(env.momentum(s)[0][0, 0]) - p0))
        worst.append(de)
        print(f"{name} dt={dt}: E0 {e0:.6f} max|E-E0| {de:.3e}  P0 {p0:.6f} max|P-P0| {dp:.3e}")
        if env.root_free[0]:
            assert abs(p0) > 1.0 and dp <= 1e-9 * abs(p0)
    assert 3.0 <= worst[0] / worst[1] <= 5.5, worst


@pytest.mark.parametrize("name", ["inverted_pendulum", "inverted_double_pendulum"])
def test_pendulums_fall_with_zero_action(name):
    env = get_environment(name)
    s, _ = env.reset(rnd.PRNGKey(0), 1)
    done = False
    for _ in range(200):
        s, _, r, d = env.step(s, torch.zeros(1, 1))
        assert torch.isfinite(s).all()
        if bool(d[0]):
            done = True
            assert float(r[0]) == 0.0
            break
    assert done


# discrete LQR gains (Q = diag(1, 10, 0.1, 0.1), R = 1) of the 20 ms control step linearised about the upright pole
FEEDBACK = (0.829, -6.733, 0.985, -1.201)


def test_linear_feedback_balances_the_inverted_pendulum():
    env = get_environment("inverted_pendulum")
    s, o = env.reset(rnd.PRNGKey(0), 1)
    k = torch.tensor(FEEDBACK)
    total = 0.0
    for _ in range(500):
        s, o, r, d = env.step(s, (o * k).sum(1, keepdim=True))
        assert not bool(d[0])
        total += float(r[0])
    assert total == 500.0 and abs(float(s[0, 0])) < 0.5 and abs(float(s[0, 3])) < 0.05


def test_reacher_target_observation_and_reward():
    env = get_environment("reacher")
    radius = env.spec["task"]["target_radius"]
    targets = [env.reset(rnd.PRNGKey(k), 1)[0][0, 2 * env.nd:] for k in range(8)]
    assert all(t.shape == (2,) and float(t.norm()) <= radius for t in targets)
    assert len({tuple(t.tolist()) for t in targets}) == 8
    s, o = env.reset(rnd.PRNGKey(3), 2)
    target = s[:, 2 * env.nd:].clone()
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        a = torch.rand(2, 2, generator=g) * 2 - 1
        s, o, r, d = env.step(s, a)
        assert torch.equal(s[:, 2 * env.nd:], target) and not d.any()
        q = s[:, :env.nd]
        k, c = env._kin(q), env._c(q)
        tip = k["hp"][:, -1] + planar._rot(k["ca"][:, -1], k["sa"][:, -1], torch.tensor(env.spec["bodies"][-1]["caps"][1][:2]))
        torch.testing.assert_close(o[:, 8:10], tip - target, rtol=0, atol=1e-7)
        torch.testing.assert_close(o[:, :2], torch.cos(q[:, 3:]))
        torch.testing.assert_close(o[:, 2:4], torch.sin(q[:, 3:]))
        assert torch.equal(o[:, 4:6], target) and torch.equal(o[:, 6:8], s[:, env.nd + 3:2 * env.nd]) and bool((o[:, 10] == 0).all())
        torch.testing.assert_close(r, -(tip - target).norm(dim=1) - (a * a).sum(1), rtol=1e-6, atol=1e-7)
    # the arm is 0.21 long: the tip stays within reach of the root
    assert float(tip.norm(dim=1).max()) <= 0.21 + 1e-6


@pytest.mark.parametrize("name", MODELS)
def test_actions_are_clamped_and_passive_hinges_take_no_column(name):
    env = get_environment(name)
    passive = sum(1 for h in env.spec["hinges"] if h["gear"] == 0)
    assert env.act_dim == (1 if env.root_gear[0] else 0) + env.nj - passive
    s, _ = env.reset(rnd.PRNGKey(0), 2)
    sign = torch.sign(torch.randn(2, env.act_dim, generator=torch.Generator().manual_seed(0)))
    for x, y in zip(env.step(s, 3.0 * sign), env.step(s, sign)):
        assert torch.equal(x, y)
    moved = env.step(s, sign)[0]
    still = env.step(s, torch.zeros(2, env.act_dim))[0]
    assert not torch.equal(moved, still)


def test_passive_hinge_in_a_driven_chain():
    """The swimmer with its first hinge passive: one action column, and it drives the second hinge."""
    h = list(planar.SWIMMER["hinges"])
    h[0] = dict(h[0], gear=0.0)
    env = planar.PlanarChain(dict(planar.SWIMMER, hinges=tuple(h)))
    full = get_environment("swimmer")
    assert env.act_dim == 1 and full.act_dim == 2 and env.obs_dim == full.obs_dim
    s, _ = env.reset(rnd.PRNGKey(0), 1)
    a = torch.tensor([[0.7]])
    for x, y in zip(env.step(s, a), full.step(s, torch.tensor([[0.0, 0.7]]))):
        torch.testing.assert_close(x, y, rtol=1e-6, atol=1e-7)


def _close(a, b):
    return a == b or abs(a - b) <= 1e-6 * max(abs(a), abs(b))  # float32 storage


@pytest.mark.parametrize("name", MODELS)
def test_model_table_round_trip_with_the_new_fields(name):
    env = get_environment(name)
    tab = env.model_table()
    assert tab.dtype == torch.float32 and tab.shape == (planar.TABLE_WORDS,) and planar.TABLE_WORDS == 232
    got = planar.PlanarChain.unpack_table(tab)
    spec, task = env.spec, env.spec["task"]
    for f in ("dt", "gravity", "contact_k", "lin_damp"):
        assert _close(got[f], spec[f]), f
    assert got["substeps"] == spec["substeps"] and got["n_bodies"] == len(spec["bodies"])
    assert got["root_free"] == tuple(spec["root_free"]) and got["kind"] == task["kind"]
    for f in ("healthy_reward", "ctrl_cost", "pitch_max", "z_lo", "tip_x_cost", "tip_goal"):
        if f in task:
            assert _close(got[f], task[f]), f
    if "vel_cost" in task:
        assert all(_close(x, y) for x, y in zip(got["vel_cost"], task["vel_cost"]))
    if "root_gear" in spec:
        assert all(_close(x, y) for x, y in zip(got["root_gear"], spec["root_gear"]))
        assert all(_close(got["root_slider"][f], v) for f, v in spec["root_slider"].items())
    else:
        assert "root_gear" not in got and "root_slider" not in got
    for gh, sh in zip(got["hinges"], spec["hinges"]):
        assert set(gh) == set(sh) and all(_close(gh[f], sh[f]) for f in sh)
    for gb, sb in zip(got["bodies"], spec["bodies"]):
        assert gb["parent"] == sb["parent"] and _close(gb["mass"], sb["mass"]) and _close(gb["inertia"], sb["inertia"])
        assert all(_close(x, y) for gc, sc in zip(gb["caps"], sb["caps"]) for x, y in zip(gc, sc))


def test_tables_of_the_four_running_models_are_unchanged():
    """Word for word the tables of the commit before constrained roots (recorded from it): the kernel-argument
    segment of every existing launch is what it was."""
    golden = np.load(os.path.join(os.path.dirname(__file__), "golden", "planar_tables_parent.npy"))
    assert golden.shape == (4, 232) and golden.dtype == np.float32
    now = np.stack([get_environment(n).model_table().numpy() for n in OLD])
    assert np.array_equal(now.view(np.uint32), golden.view(np.uint32))
    for n in OLD:
        got = planar.PlanarChain.unpack_table(get_environment(n).model_table())
        assert not {"root_free", "kind", "root_gear", "root_slider", "vel_cost"} & set(got)


def test_openes_inverted_pendulum_improves():
    """The centre policy's return after OpenES generations exceeds its return before by more than
    the standard deviation of the first generation's 64 returns."""
    policy = MLPPolicy([4, 16, 16, 1])
    params = policy.init(rnd.PRNGKey(1))
    adapter = TreeAndVector(params)
    problem = Brax(policy, "inverted_pendulum", cap_episode=100)
    algo = OpenES(adapter.to_vector(params), 64, learning_rate=0.02, noise_stdev=0.05, optimizer="adam")
    wf = StdWorkflow(algo, problem, sol_transforms=[adapter.batched_to_tree], fit_transforms=[rank_based_fitness], opt_direction="max")
    st = wf.init(rnd.PRNGKey(3))

    def centre_return(st):
        centre = st.get_child_state("algorithm").center
        ret, _ = problem.evaluate(st.get_child_state("problem"), adapter.batched_to_tree(centre[None, :]))
        return float(ret[0])

    before = centre_return(st)
    st = wf.step(st)
    pop = st.get_child_state("algorithm").population  # after the first step: the first generation
    first, _ = problem.evaluate(st.get_child_state("problem"), adapter.batched_to_tree(pop))
    spread = float(first.std())
    for _ in range(29):
        st = wf.step(st)
    after = centre_return(st)
    assert math.isfinite(before) and after > before + spread, f"before {before} after {after} first-generation std {spread}"


def test_fused_case_is_the_six_combinations():
    for name in MODELS + OLD:
        assert get_environment(name).within_caps(), name
    # hopper's chain of 4 with a locked root, a two-link reach arm on a free root, a cart whose pole is driven:
    # combinations with no instantiated kernel, so outside the fused case
    outside = [planar.PlanarChain(dict(planar.HOPPER, root_free=(1, 0, 0))),
               planar.PlanarChain(dict(planar.REACHER, root_free=(1, 1, 1))),
               planar.PlanarChain(dict(planar.INVERTED_PENDULUM, hinges=(dict(planar.INVERTED_PENDULUM["hinges"][0], gear=10.0),))),
               planar.PlanarChain(dict(planar.SWIMMER, root_gear=(5.0, 0.0, 0.0)))]
    for env in outside:
        assert not env.within_caps()
        s, _ = env.reset(rnd.PRNGKey(0), 2)
        assert torch.isfinite(env.step(s, torch.zeros(2, env.act_dim))[0]).all()  # the torch engine runs them
        policy = MLPPolicy([env.obs_dim, 8, 8, env.act_dim])
        prob = Brax(policy, "hopper", 3)
        prob.env = env
        assert not prob._fused_ok(torch.utils._pytree.tree_map(lambda x: x[None], policy.init(rnd.PRNGKey(0))))


def test_render_draws_the_target_and_no_ground():
    env = get_environment("reacher")
    s, _ = env.reset(rnd.PRNGKey(1), 1)
    img = env.render(s[0], width=96, height=64, span=0.6)
    assert img.shape == (64, 96, 3) and img.dtype == torch.uint8
    assert bool((img == torch.tensor([40, 160, 60], dtype=torch.uint8)).all(-1).any())  # the target
    assert not bool((img == torch.tensor([120, 100, 80], dtype=torch.uint8)).all(-1).any())  # no ground
    frames = Brax(MLPPolicy([4, 8, 8, 1]), "inverted_pendulum", 3).visualize(rnd.PRNGKey(1), MLPPolicy([4, 8, 8, 1]).init(rnd.PRNGKey(0)),
                                                                             output_type="rgb_array", width=96, height=64)
    assert len(frames) == 4 and not any(bool((f == torch.tensor([120, 100, 80], dtype=torch.uint8)).all(-1).any()) for f in frames)
