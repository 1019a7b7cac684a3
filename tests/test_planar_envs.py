"""The planar articulated-tree engine (``PlanarChain``) and the hopper, walker2d, halfcheetah and
swimmer environments on it: resolution, mass matrix and velocity-product terms against autograd,
momentum invariants, behaviour at rest, learning, the kernel's model table and rendering."""
import math

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

MODELS = ("hopper", "walker2d", "halfcheetah", "swimmer")
DIMS = {"hopper": (11, 3), "walker2d": (17, 6), "halfcheetah": (17, 6), "swimmer": (8, 2)}
# no external force: gravity, contacts, root-body damping and fluid drag off (what stays is internal)
FREE = dict(gravity=0.0, contact_k=0.0, contact_c=0.0, lin_damp=0.0, ang_damp=0.0, fluid_cn=0.0, fluid_ct=0.0, fluid_cw=0.0)


@pytest.mark.parametrize("name,spelling", [(n, s) for n, g in zip(MODELS, ("Hopper-v4", "Walker2d-v4", "HalfCheetah-v4", "Swimmer-v4")) for s in (n, g)])
def test_names_resolve_through_brax(name, spelling):
    obs_dim, act_dim = DIMS[name]
    prob = Brax(MLPPolicy([obs_dim, 8, 8, act_dim]), spelling, 10)
    env = prob.env
    assert isinstance(env, planar.PlanarChain) and (env.obs_dim, env.act_dim) == (obs_dim, act_dim)
    s, o = env.reset(rnd.PRNGKey(0), 3)
    assert s.shape == (3, 2 * env.nd) and o.shape == (3, obs_dim) and torch.equal(s[0], s[1]) and torch.equal(s[0], s[2])
    s2, o2, r, d = env.step(s, torch.zeros(3, act_dim))
    assert s2.shape == s.shape and o2.shape == o.shape and r.shape == (3,) and d.shape == (3,) and d.dtype == torch.bool
    assert torch.isfinite(s2).all() and torch.isfinite(o2).all() and torch.isfinite(r).all()


def test_unknown_name_still_raises():
    with pytest.raises(ValueError):
        Brax(MLPPolicy([4, 8, 8, 2]), "humanoid", 10)


@pytest.mark.parametrize("name", MODELS)
def test_mass_matrix_momenta_and_velocity_products_match_autograd(name):
    """π = M(q)u equals ∂T/∂u and the closed-form ∂T/∂q equals autograd's, with T assembled
    independently from the link velocities."""
    env = get_environment(name)
    g = torch.Generator().manual_seed(0)
    q = (0.5 * torch.randn(5, env.nd, generator=g, dtype=torch.float64)).requires_grad_(True)
    u = torch.randn(5, env.nd, generator=g, dtype=torch.float64).requires_grad_(True)
    T = env.kinetic_energy(q, u)
    gq, gu = torch.autograd.grad(T.sum(), [q, u])
    torch.testing.assert_close(env.momenta(q.detach(), u.detach()), gu, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(env.dTdq(q.detach(), u.detach()), gq, rtol=1e-10, atol=1e-10)
    assert bool((T > 0).all())


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 1e-4)])
@pytest.mark.parametrize("name", MODELS)
def test_momentum_conserved_without_external_forces(name, dtype, tol):
    """Random joint torques with joint damping, stiffness and limit springs on (all internal): linear
    momentum and angular momentum about the world origin are conserved over 200 control steps."""
    env = get_environment(name, **FREE)
    s, _ = env.reset(rnd.PRNGKey(0), 4)
    s = s.to(dtype)
    s[:, 1] += 5.0
    s[:, env.nd:env.nd + 3] += torch.randn(4, 3, generator=torch.Generator().manual_seed(1)).to(dtype)
    q0 = s[:, 3:env.nd].clone()
    P0, L0 = env.momentum(s)
    g = torch.Generator().manual_seed(2)
    for _ in range(200):
        s, _, _, _ = env.step(s, (torch.rand(4, env.act_dim, generator=g) * 2 - 1).to(dtype))
    P1, L1 = env.momentum(s)
    assert torch.isfinite(s).all()
    assert float((P1 - P0).norm(dim=1).max()) <= tol * float(P0.norm(dim=1).max())
    assert float((L1 - L0).abs().max()) <= tol * float(L0.abs().max())
    assert float((s[:, 3:env.nd] - q0).abs().max()) > 0.1  # the joints did move


@pytest.mark.parametrize("name", MODELS)
def test_gravity_enters_the_momenta_exactly(name):
    """Free fall from height with random torques: vertical momentum = P0 − m_tot·g·t, horizontal unchanged."""
    g_acc = 9.81
    env = get_environment(name, **dict(FREE, gravity=g_acc))
    s, _ = env.reset(rnd.PRNGKey(0), 4)
    s = s.double()
    s[:, 1] += 1000.0
    s[:, env.nd:env.nd + 3] += torch.randn(4, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    P0, _ = env.momentum(s)
    g = torch.Generator().manual_seed(2)
    for _ in range(100):
        s, _, _, _ = env.step(s, torch.rand(4, env.act_dim, generator=g, dtype=torch.float64) * 2 - 1)
    P1, _ = env.momentum(s)
    m_tot = sum(b["mass"] for b in env.spec["bodies"])
    t = 100 * env.spec["dt"] * env.spec["substeps"]
    expect = P0[:, 1] - m_tot * g_acc * t
    assert float((P1[:, 1] - expect).abs().max()) <= 1e-9 * float(expect.abs().max())
    assert float((P1[:, 0] - P0[:, 0]).abs().max()) <= 1e-9 * float(expect.abs().max())


def test_halfcheetah_stands_with_zero_action():
    env = get_environment("halfcheetah")
    s, _ = env.reset(rnd.PRNGKey(0), 2)
    for _ in range(100):
        s, _, _, d = env.step(s, torch.zeros(2, 6))
    assert torch.isfinite(s).all() and not d.any()
    lo, hi = env.spec["standing_band"]
    assert lo < float(s[0, 1]) < hi
    c, k = env._c(s), env._kin(s[:, :env.nd])
    z = (k["hp"][:, c["cap_body"]] + planar._rot(k["ca"][:, c["cap_body"]], k["sa"][:, c["cap_body"]], c["cap_pt"]))[..., 1]
    on = c["cap_on"] > 0
    assert bool((z[:, on] > 0).all())  # no contact sphere is deeper than its radius (its centre stays above the ground)


@pytest.mark.parametrize("name,cap", [("hopper", 400), ("walker2d", 400)])
def test_hopper_and_walker_fall_with_zero_action(name, cap):
    env = get_environment(name)
    s, _ = env.reset(rnd.PRNGKey(0), 1)
    done = False
    for _ in range(cap):
        s, _, _, d = env.step(s, torch.zeros(1, env.act_dim))
        assert torch.isfinite(s).all()
        if bool(d[0]):
            done = True
            break
    assert done


def test_swimmer_drag_dissipates_kinetic_energy():
    env = get_environment("swimmer")
    s, _ = env.reset(rnd.PRNGKey(0), 1)
    s = s.double()
    s[:, env.nd:] += torch.randn(1, env.nd, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    T = [float(env.kinetic_energy(s[:, :env.nd], s[:, env.nd:]))]
    for _ in range(60):
        s, _, _, d = env.step(s, torch.zeros(1, 2, dtype=torch.float64))
        T.append(float(env.kinetic_energy(s[:, :env.nd], s[:, env.nd:])))
    assert not bool(d[0]) and T[0] > 0
    assert all(b <= a * (1 + 1e-12) for a, b in zip(T[:-1], T[1:])), T
    assert T[-1] < 0.5 * T[0]


@pytest.mark.parametrize("name", MODELS)
def test_actions_are_clamped(name):
    env = get_environment(name)
    s, _ = env.reset(rnd.PRNGKey(0), 2)
    sign = torch.sign(torch.randn(2, env.act_dim, generator=torch.Generator().manual_seed(0)))
    a = env.step(s, 3.0 * sign)
    b = env.step(s, sign)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_non_finite_state_is_unhealthy():
    env = get_environment("halfcheetah")
    s, _ = env.reset(rnd.PRNGKey(0), 2)
    s[1, 4] = float("nan")
    _, _, r, d = env.step(s, torch.zeros(2, 6))
    assert d.tolist() == [False, True] and torch.isfinite(r).all()


def test_openes_hopper_improves():
    """The centre policy's return after OpenES generations exceeds its return before by more than
    the standard deviation of the first generation's 64 returns."""
    policy = MLPPolicy([11, 16, 16, 3])
    params = policy.init(rnd.PRNGKey(1))
    adapter = TreeAndVector(params)
    problem = Brax(policy, "hopper", cap_episode=60)
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


def _close(a, b):
    return a == b or abs(a - b) <= 1e-6 * max(abs(a), abs(b))  # float32 storage


@pytest.mark.parametrize("name", MODELS)
def test_model_table_round_trip(name):
    env = get_environment(name)
    tab = env.model_table()
    assert tab.dtype == torch.float32 and tab.shape == (planar.TABLE_WORDS,)
    got = planar.PlanarChain.unpack_table(tab)
    spec = env.spec
    for f in ("dt", "gravity", "contact_k", "contact_c", "mu", "eps_v", "lin_damp", "ang_damp", "fluid_cn", "fluid_ct", "fluid_cw"):
        assert _close(got[f], spec[f]), f
    assert got["substeps"] == spec["substeps"] and got["n_bodies"] == len(spec["bodies"])
    for f, v in spec["task"].items():
        assert _close(got[f], v), f
    assert len(got["bodies"]) == len(spec["bodies"]) and len(got["hinges"]) == len(spec["hinges"])
    for gb, sb in zip(got["bodies"], spec["bodies"]):
        assert gb["parent"] == sb["parent"]
        for f in ("anchor", "com"):
            assert all(_close(x, y) for x, y in zip(gb[f], sb[f])), f
        assert _close(gb["mass"], sb["mass"]) and _close(gb["inertia"], sb["inertia"])
        assert all(_close(x, y) for gc, sc in zip(gb["caps"], sb["caps"]) for x, y in zip(gc, sc))
    for gh, sh in zip(got["hinges"], spec["hinges"]):
        assert set(gh) == set(sh) and all(_close(gh[f], sh[f]) for f in sh)


def test_model_over_a_cap_is_rejected():
    spec = dict(planar.HOPPER)
    bodies, hinges = list(spec["bodies"]), list(spec["hinges"])
    while len(bodies) < 9:  # 9 bodies: over the 8-body cap
        bodies.append(planar.capsule(len(bodies) - 1, (0.26, 0), (0, 0), (0.1, 0), 0.03, 0.5))
        hinges.append(planar.hinge(10.0, -1.0, 1.0, 0.1, 0.1, limit_k=100.0))
    env = planar.PlanarChain(dict(spec, bodies=tuple(bodies), hinges=tuple(hinges)))
    assert not env.within_caps()
    with pytest.raises(ValueError, match="caps"):
        env.model_table()
    s, _ = env.reset(rnd.PRNGKey(0), 2)
    assert torch.isfinite(env.step(s, torch.zeros(2, env.act_dim))[0]).all()  # the torch engine has no cap
    policy = MLPPolicy([env.obs_dim, 8, 8, env.act_dim])
    prob = Brax(policy, "hopper", 3)
    prob.env = env
    tree = torch.utils._pytree.tree_map(lambda x: x[None], policy.init(rnd.PRNGKey(0)))
    assert not prob._fused_ok(tree)
    # within the hidden cap but over one wave's LDS: outside the fused case (checked without a GPU)
    from evoxmi.ops import neuro

    assert neuro.planar_lds_bytes(11, 256, 256, 3) > neuro.PLANAR_LDS_LIMIT >= neuro.planar_lds_bytes(11, 128, 128, 3)
    # a tree shape with no instantiated kernel is outside the fused case too
    b2 = list(planar.HOPPER["bodies"])
    b2[2] = dict(b2[2], parent=0)
    assert not planar.PlanarChain(dict(planar.HOPPER, bodies=tuple(b2))).within_caps()
    assert get_environment("hopper").within_caps()


def test_visualize_rgb_array_and_default_trajectory():
    policy = MLPPolicy([11, 8, 8, 3])
    params = policy.init(rnd.PRNGKey(0))
    prob = Brax(policy, "hopper", 6)
    frames = prob.visualize(rnd.PRNGKey(1), params, output_type="rgb_array", width=96, height=64)
    assert len(frames) == 7
    assert all(f.shape == (64, 96, 3) and f.dtype == torch.uint8 for f in frames)
    assert any(not torch.equal(frames[0], f) for f in frames[1:])
    traj = prob.visualize(rnd.PRNGKey(1), params)
    assert len(traj) == 7 and all(x.shape == (12,) and x.dtype == torch.float32 for x in traj)
    # the default output is the state trajectory of the same rollout
    s, _ = prob.env.reset(rnd.PRNGKey(1), 1)
    assert torch.equal(traj[0], s[0])
    with pytest.raises(ValueError):
        Brax(MLPPolicy([4, 8, 8, 2], discrete=True), "cartpole", 3).visualize(rnd.PRNGKey(1), None, output_type="rgb_array")
