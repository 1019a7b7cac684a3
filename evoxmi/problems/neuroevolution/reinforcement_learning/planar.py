"""Planar articulated-tree engine and the planar Brax-style tasks: four that run (hopper, walker2d,
halfcheetah, swimmer), two that balance (inverted_pendulum, inverted_double_pendulum) and the reacher.

``PlanarChain`` integrates a tree of rigid links that moves in one plane (vertical for
hopper / walker2d / halfcheetah, horizontal for the swimmer) from a declarative model spec,
a plain dict of numbers and tuples.  The spec is the single source of truth: the fused
rollout kernel (``csrc/kernels/planar_rollout.hip``, ``ops.neuro.planar_rollout``) reads the
float32 table that :meth:`PlanarChain.model_table` packs from it, so no constant is written
twice.  The torch code here is the CPU path and the numerics oracle of that kernel.

The environments are **Brax-style**: the interface, observation layout, reward and
termination rule of the Brax / MuJoCo tasks of the same names, on this engine's own
dynamics (penalty contacts, this file's geometry).  They are not bit-compatible with Brax or
MuJoCo and no parity with their numbers is claimed.

Model
-----
Body ``b`` hangs on hinge ``b`` of its parent (body 0 is the free root); every body frame is
world-aligned at zero angles.  Per body: parent index, hinge anchor in the parent frame
(origin = the parent's hinge point), CoM offset from the hinge, mass, pitch inertia about
the CoM and the two capsule end caps ``(x, z, radius, contact)`` (body-frame point, radius,
1 if the cap is a ground-contact sphere).  Per hinge: gear, armature, damping, stiffness with
rest angle, range with a limit-spring constant, initial angle.  Global: gravity, sub-step
``dt``, sub-steps per control step, contact ``k`` / ``c`` / ``mu`` / ``eps_v``, root-body
damping and the fluid coefficients (swimmer).

Coordinates ``q = (x, z, θ_root, φ_1 … φ_nj)``, ``u = q̇``, state ``(N, 2·nd) = q ++ u`` with
``nd = 3 + nj``.  Angles are counter-clockwise in the (x, z) plane.

One sub-step is symplectic Euler in momentum form, the scheme of ``envs.Ant._substep``:

1. ``q ← q + dt·u``;
2. ``π ← π + dt·(τ + Q_ext + ∂T/∂q)`` at the new pose, where the root's three momenta are the
   system's linear momentum and its angular momentum about the world origin (they take the
   external wrench only, so gravity and contacts enter them exactly) and a hinge's momentum
   is ``∂T/∂φ̇``; ``∂T/∂φ_k = v_hinge,z·P_x − v_hinge,x·P_z`` with ``P`` the linear
   momentum of the hinge's subtree (planar angular velocities do not depend on ``q``);
3. ``u = M(q)⁻¹ π``, ``M = Σ_b J_bᵀ diag(m_b, m_b, I_b) J_b + diag(armature)``, by a Cholesky
   solve of the dense ``nd × nd`` matrix.

Constrained root, slider, passive hinges, task kinds (all optional; the defaults are the above)
-------------------------------------------------------------------------------------------------
``root_free=(fx, fz, fθ)`` locks root coordinates: a locked one keeps its ``root_init`` value exactly, has
velocity exactly 0 and gets no reset noise.  The sub-step then advances the generalized momenta of the free
coordinates ``F`` directly (``π_θ`` about the root point, ``∂T/∂φ_k`` in the same closed form) and solves the
reduced system ``M[F, F] u_F = π_F``; the momentum rows of locked coordinates are never read.
``root_gear=(gx, 0, 0)`` and ``root_slider=dict(lo, hi, limit_k)`` drive root x: its force is
``gx·a − lin_damp·ẋ + limit_k·(clamp(lo − x, 0) − clamp(x − hi, 0))``.  A hinge with gear 0 is passive and takes no
action: ``act_dim`` counts the non-zero gears, the slider's column first, then the hinges in body order.
``task["kind"]`` is ``"run"`` (forward velocity, health on root height and pitch, observation ``q ++ u``),
``"balance"`` (observation ``q_F ++ u_F``, reward ``healthy_reward − ctrl_cost·‖a‖²``, unhealthy when the first
link's absolute angle reaches ``pitch_max``), ``"balance_tip"`` (observation free root coordinates, ``sin φ``,
``cos φ``, ``u_F``; reward ``healthy_reward − (tip_x_cost·x_tip² + (z_tip − tip_goal)²) − Σ_j vel_cost_j·φ̇_j²``;
unhealthy when ``z_tip ≤ z_lo``; the tip is the far end cap of the last body) or ``"reach"`` (two hinges;
observation ``cos φ, sin φ, target, φ̇, tip − target, 0``; reward ``−‖tip − target‖ − ctrl_cost·‖a‖²``).  A
non-finite state is unhealthy in every kind.  The state is ``q ++ u ++ aux`` with ``state_dim = 2·nd + n_aux``:
``aux`` is the reach task's target (2 words, uniform in a disc of ``target_radius``, drawn at reset from
``fold_in(key, 1)``) and empty otherwise; ``step`` carries it through unchanged.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ....ops import random as rnd
from .envs import register

INF = float("inf")

# caps of the fused kernel (ops.neuro.planar_rollout)
MAX_BODIES, MAX_DOF, MAX_OBS, MAX_ACT, MAX_HIDDEN = 8, 10, 32, 8, 512
# model table layout (float32 words; integers are stored as exact floats)
TABLE_HEADER, TABLE_BODY, TABLE_HINGE = 24, 16, 10
TABLE_WORDS = TABLE_HEADER + MAX_BODIES * (TABLE_BODY + TABLE_HINGE)
_HEADER_FIELDS = ("n_bodies", "obs_skip", "substeps", "dt", "gravity", "contact_k", "contact_c", "mu", "eps_v", "lin_damp", "ang_damp",
                  "fluid_cn", "fluid_ct", "fluid_cw", "vel_clip", "healthy_reward", "ctrl_cost", "z_lo", "z_hi", "pitch_max")
_HINGE_FIELDS = ("gear", "armature", "damping", "stiffness", "rest", "lo", "hi", "limit_k", "init")
# words added for constrained roots and task kinds; every one is 0 for a free-root "run" model, so those tables are unchanged:
# header 20 … 23, hinge row 0 (the root slider, at the hinge fields' own offsets) and word 9 of every hinge row (vel_cost)
_HEADER_EXTRA = ("root_lock", "kind", "tip_x_cost", "tip_goal")
_SLIDER_FIELDS = ("gear", "lo", "hi", "limit_k")
VEL_COST_WORD = len(_HINGE_FIELDS)
KINDS = ("run", "balance", "balance_tip", "reach")
_TASK_DEFAULTS = dict(kind="run", obs_skip=0, vel_clip=0.0, healthy_reward=0.0, ctrl_cost=0.0, z_lo=-INF, z_hi=INF, pitch_max=INF,
                      tip_x_cost=0.0, tip_goal=0.0, vel_cost=None, target_radius=0.0)
# what the kernel is instantiated for: (parent list, mask of locked root coordinates (1 x, 2 z, 4 θ), task kind)
FUSED_COMBINATIONS = (((-1, 0, 1), 0, "run"), ((-1, 0, 1, 2), 0, "run"), ((-1, 0, 1, 2, 0, 4, 5), 0, "run"),
                      ((-1, 0), 6, "balance"), ((-1, 0, 1), 6, "balance_tip"), ((-1, 0, 1), 7, "reach"))
FUSED_TOPOLOGIES = tuple(c[0] for c in FUSED_COMBINATIONS[:3])


def capsule(parent, anchor, p0, p1, radius, mass, contact=(1, 1)):
    """A capsule link from ``p0`` to ``p1`` (body frame, origin at the hinge): CoM at the
    middle, pitch inertia of a solid cylinder ``m·(L²/12 + r²/4)``, end caps at both ends."""
    length = math.hypot(p1[0] - p0[0], p1[1] - p0[1])
    return dict(parent=parent, anchor=tuple(map(float, anchor)), com=(0.5 * (p0[0] + p1[0]), 0.5 * (p0[1] + p1[1])), mass=float(mass),
                inertia=mass * (length * length / 12 + radius * radius / 4),
                caps=((float(p0[0]), float(p0[1]), float(radius), float(contact[0])), (float(p1[0]), float(p1[1]), float(radius), float(contact[1]))))


def hinge(gear, lo, hi, armature=0.0, damping=0.0, stiffness=0.0, rest=0.0, limit_k=0.0, init=0.0):
    return dict(gear=float(gear), armature=float(armature), damping=float(damping), stiffness=float(stiffness), rest=float(rest),
                lo=float(lo), hi=float(hi), limit_k=float(limit_k), init=float(init))


_D = math.pi / 180


def _leg(parent0, first, foot_heel, foot_toe, masses, gear, armature, damping, limit_k):
    """thigh 0.45 / leg 0.5 / foot of the hopper and the walker, hanging from the torso's lower end."""
    bodies = [capsule(parent0, (0, -0.2), (0, 0), (0, -0.45), 0.05, masses[0], contact=(0, 1)),
              capsule(first, (0, -0.45), (0, 0), (0, -0.5), 0.04, masses[1], contact=(0, 0)),
              capsule(first + 1, (0, -0.5), (foot_heel, 0), (foot_toe, 0), 0.06, masses[2])]
    hinges = [hinge(gear, -150 * _D, 0, armature, damping, limit_k=limit_k), hinge(gear, -150 * _D, 0, armature, damping, limit_k=limit_k),
              hinge(gear, -45 * _D, 45 * _D, armature, damping, limit_k=limit_k)]
    return bodies, hinges


def _hopper():
    b, h = _leg(0, 1, -0.13, 0.26, (3.93, 2.71, 5.09), 200.0, 1.0, 1.0, 2000.0)
    return dict(name="hopper", bodies=tuple([capsule(-1, (0, 0), (0, 0.2), (0, -0.2), 0.05, 3.53)] + b), hinges=tuple(h),
                gravity=9.81, dt=0.002, substeps=4, contact_k=20000.0, contact_c=300.0, mu=1.0, eps_v=0.1, lin_damp=0.0, ang_damp=0.0,
                fluid_cn=0.0, fluid_ct=0.0, fluid_cw=0.0,
                task=dict(obs_skip=1, vel_clip=10.0, healthy_reward=1.0, ctrl_cost=1e-3, z_lo=0.7, z_hi=INF, pitch_max=0.2),
                root_init=(0.0, 1.25, 0.0), reset_noise=5e-3, standing_band=None)


def _walker2d():
    b1, h1 = _leg(0, 1, 0.0, 0.2, (3.93, 2.71, 2.94), 100.0, 0.3, 1.0, 1000.0)
    b2, h2 = _leg(0, 4, 0.0, 0.2, (3.93, 2.71, 2.94), 100.0, 0.3, 1.0, 1000.0)
    return dict(name="walker2d", bodies=tuple([capsule(-1, (0, 0), (0, 0.2), (0, -0.2), 0.05, 3.53)] + b1 + b2), hinges=tuple(h1 + h2),
                gravity=9.81, dt=0.002, substeps=4, contact_k=20000.0, contact_c=300.0, mu=1.0, eps_v=0.1, lin_damp=0.0, ang_damp=0.0,
                fluid_cn=0.0, fluid_ct=0.0, fluid_cw=0.0,
                task=dict(obs_skip=1, vel_clip=10.0, healthy_reward=1.0, ctrl_cost=1e-3, z_lo=0.8, z_hi=2.0, pitch_max=1.0),
                root_init=(0.0, 1.25, 0.0), reset_noise=5e-3, standing_band=None)


def _halfcheetah():
    r = 0.046
    links = (((-0.5, 0), (0.16, -0.25), 1.54), ((0.16, -0.25), (-0.28, -0.14), 1.58), ((-0.28, -0.14), (0.06, -0.19), 1.07),
             ((0.5, 0), (-0.14, -0.24), 1.43), ((-0.14, -0.24), (0.13, -0.18), 1.18), ((0.13, -0.18), (0.09, -0.14), 0.85))
    parents = (0, 1, 2, 0, 4, 5)
    bodies = [capsule(-1, (0, 0), (-0.5, 0), (0.5, 0), r, 6.36)]
    for p, (anchor, tip, m) in zip(parents, links):
        bodies.append(capsule(p, anchor, (0, 0), tip, r, m, contact=(0, 1)))
    gear = (120, 90, 60, 120, 60, 30)
    stiff = (240, 180, 120, 180, 120, 60)
    damp = (6, 4.5, 3, 4.5, 3, 1.5)
    rng = ((-1.05, 0.52), (-0.785, 0.785), (-0.785, 0.4), (-0.7, 1.0), (-0.87, 1.2), (-0.5, 0.5))
    hinges = [hinge(g, lo, hi, 1.0, d, s, 0.0, 200.0) for g, s, d, (lo, hi) in zip(gear, stiff, damp, rng)]
    return dict(name="halfcheetah", bodies=tuple(bodies), hinges=tuple(hinges),
                gravity=9.81, dt=0.01, substeps=5, contact_k=5000.0, contact_c=100.0, mu=1.0, eps_v=0.3, lin_damp=0.0, ang_damp=0.0,
                fluid_cn=0.0, fluid_ct=0.0, fluid_cw=0.0,
                task=dict(obs_skip=1, vel_clip=0.0, healthy_reward=0.0, ctrl_cost=0.1, z_lo=-INF, z_hi=INF, pitch_max=INF),
                root_init=(0.0, 0.7, 0.0), reset_noise=0.1, standing_band=(0.4, 0.8))


def _swimmer():
    bodies = [capsule(-1, (0, 0), (0, 0), (-1, 0), 0.1, 30.0, contact=(0, 0)), capsule(0, (-1, 0), (0, 0), (-1, 0), 0.1, 30.0, contact=(0, 0)),
              capsule(1, (-1, 0), (0, 0), (-1, 0), 0.1, 30.0, contact=(0, 0))]
    hinges = [hinge(150.0, -100 * _D, 100 * _D, 1.0, 30.0, limit_k=2000.0) for _ in range(2)]
    return dict(name="swimmer", bodies=tuple(bodies), hinges=tuple(hinges),
                gravity=0.0, dt=0.01, substeps=4, contact_k=0.0, contact_c=0.0, mu=0.0, eps_v=0.05, lin_damp=0.0, ang_damp=0.0,
                fluid_cn=300.0, fluid_ct=30.0, fluid_cw=30.0,
                task=dict(obs_skip=2, vel_clip=0.0, healthy_reward=0.0, ctrl_cost=1e-4, z_lo=-INF, z_hi=INF, pitch_max=INF),
                root_init=(0.0, 0.0, 0.0), reset_noise=0.1, standing_band=None)


def _no_ground():
    return dict(contact_k=0.0, contact_c=0.0, mu=0.0, eps_v=0.05, ang_damp=0.0, fluid_cn=0.0, fluid_ct=0.0, fluid_cw=0.0, standing_band=None)


def _cart():
    return capsule(-1, (0, 0), (-0.1, 0), (0.1, 0), 0.1, 10.5, contact=(0, 0))


def _inverted_pendulum():
    pole = capsule(0, (0, 0), (0, 0), (0, 0.6), 0.049, 5.0, contact=(0, 0))
    return dict(name="inverted_pendulum", bodies=(_cart(), pole), hinges=(hinge(0.0, -INF, INF, damping=0.05),),
                gravity=9.81, dt=0.002, substeps=10, lin_damp=1.0, root_free=(1, 0, 0), root_gear=(100.0, 0.0, 0.0),
                root_slider=dict(lo=-1.0, hi=1.0, limit_k=5000.0),
                task=dict(kind="balance", healthy_reward=1.0, ctrl_cost=0.0, pitch_max=0.2),
                root_init=(0.0, 0.0, 0.0), reset_noise=0.01, **_no_ground())


def _inverted_double_pendulum():
    poles = (capsule(0, (0, 0), (0, 0), (0, 0.6), 0.045, 4.2, contact=(0, 0)), capsule(1, (0, 0.6), (0, 0), (0, 0.6), 0.045, 4.2, contact=(0, 0)))
    return dict(name="inverted_double_pendulum", bodies=(_cart(),) + poles, hinges=(hinge(0.0, -INF, INF, damping=0.05), hinge(0.0, -INF, INF, damping=0.05)),
                gravity=9.81, dt=0.001, substeps=20, lin_damp=1.0, root_free=(1, 0, 0), root_gear=(500.0, 0.0, 0.0),
                root_slider=dict(lo=-1.0, hi=1.0, limit_k=5000.0),
                task=dict(kind="balance_tip", healthy_reward=10.0, tip_x_cost=0.01, tip_goal=2.0, vel_cost=(1e-3, 5e-3), z_lo=1.0),
                root_init=(0.0, 0.0, 0.0), reset_noise=0.05, **_no_ground())


def _reacher():
    bodies = (capsule(-1, (0, 0), (-0.01, 0), (0.01, 0), 0.02, 1.0, contact=(0, 0)), capsule(0, (0, 0), (0, 0), (0.1, 0), 0.01, 0.0356, contact=(0, 0)),
              capsule(1, (0.1, 0), (0, 0), (0.11, 0), 0.01, 0.0387, contact=(0, 0)))
    hinges = (hinge(200.0, -INF, INF, armature=1.0, damping=1.0), hinge(200.0, -3.0, 3.0, armature=1.0, damping=1.0, limit_k=1000.0))
    return dict(name="reacher", bodies=bodies, hinges=hinges, gravity=0.0, dt=0.01, substeps=2, lin_damp=0.0, root_free=(0, 0, 0),
                task=dict(kind="reach", ctrl_cost=1.0, target_radius=0.2),
                root_init=(0.0, 0.0, 0.0), reset_noise=0.1, **_no_ground())


HOPPER, WALKER2D, HALFCHEETAH, SWIMMER = _hopper(), _walker2d(), _halfcheetah(), _swimmer()
INVERTED_PENDULUM, INVERTED_DOUBLE_PENDULUM, REACHER = _inverted_pendulum(), _inverted_double_pendulum(), _reacher()


def _rot(c, s, v):
    """Rotate v (…, 2) counter-clockwise by the angle whose cosine / sine are c / s (…)."""
    return torch.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1]], -1)


def _perp(v):
    return torch.stack([-v[..., 1], v[..., 0]], -1)


class PlanarChain:
    """Planar articulated tree integrated in momentum form (see the module docstring).

    ``spec``: the model dict (``HOPPER`` … ``SWIMMER`` are the registered ones).  Works in
    float32 and float64 on any device; the dtype and device follow the state tensor."""

    discrete = False

    def __init__(self, spec=None, **overrides):
        spec = dict(self.SPEC if spec is None else spec)
        spec.update(overrides)
        self.spec = spec
        self.nb = len(spec["bodies"])
        self.nj = self.nb - 1
        self.nd = self.nb + 2
        if len(spec["hinges"]) != self.nj:
            raise ValueError("PlanarChain: one hinge per non-root body")
        self.parents = tuple(int(b["parent"]) for b in spec["bodies"])
        if self.parents[0] != -1 or any(not 0 <= p < i for i, p in enumerate(self.parents) if i > 0):
            raise ValueError("PlanarChain: body 0 is the root and every parent index precedes its child")
        t = self.task = dict(_TASK_DEFAULTS, **spec["task"])
        self.kind = t["kind"]
        if self.kind not in KINDS:
            raise ValueError(f"PlanarChain: task kind {self.kind!r} is not one of {KINDS}")
        self.obs_skip = int(t["obs_skip"])
        self.root_free = tuple(bool(f) for f in spec.get("root_free", (1, 1, 1)))
        self.root_lock = sum(1 << i for i, f in enumerate(self.root_free) if not f)
        self.free = tuple(i for i in range(3) if self.root_free[i]) + tuple(range(3, self.nd))
        self.n_free_root = len(self.free) - self.nj
        self.root_gear = tuple(float(g) for g in spec.get("root_gear", (0.0, 0.0, 0.0)))
        if self.root_gear[1] or self.root_gear[2] or (self.root_gear[0] and not self.root_free[0]):
            raise ValueError("PlanarChain: only a free root x can be driven (root_gear = (gx, 0, 0))")
        self.slider = spec.get("root_slider")
        self.act_hinges = tuple(j for j, h in enumerate(spec["hinges"]) if h["gear"] != 0)
        self.act_dim = (1 if self.root_gear[0] else 0) + len(self.act_hinges)
        self.vel_cost = tuple(float(v) for v in (t["vel_cost"] or (0.0,) * self.nj))
        if len(self.vel_cost) != self.nj:
            raise ValueError("PlanarChain: one vel_cost per hinge")
        if self.kind == "reach" and self.nj != 2:
            raise ValueError("PlanarChain: the reach task is a two-hinge arm")
        nf = len(self.free)
        self.n_aux = 2 if self.kind == "reach" else 0
        self.obs_dim = {"run": 2 * nf - self.obs_skip, "balance": 2 * nf, "balance_tip": self.n_free_root + 2 * self.nj + nf, "reach": 11}[self.kind]
        self.state_dim = 2 * self.nd + self.n_aux
        self._consts = {}

    # -- caps of the fused kernel -------------------------------------------------------
    def _fused_combination(self):
        """The kernel is instantiated for this tree shape, root constraint, task kind and actuation: the slider driven
        and every hinge passive for the two balance kinds, no slider and every hinge driven for the others."""
        if (self.parents, self.root_lock, self.kind) not in FUSED_COMBINATIONS:
            return False
        slider = bool(self.root_gear[0]) or bool(self.slider and self.slider["limit_k"])
        if self.kind in ("balance", "balance_tip"):
            return bool(self.root_gear[0]) and not self.act_hinges and self.obs_skip == 0
        return not slider and len(self.act_hinges) == self.nj and (self.kind == "run" or self.obs_skip == 0)

    def within_caps(self):
        return (self.nb <= MAX_BODIES and self.nd <= MAX_DOF and self.obs_dim <= MAX_OBS and self.act_dim <= MAX_ACT
                and self._fused_combination())

    def model_table(self):
        """The float32 table (``TABLE_WORDS``) the fused kernel reads: header, 8 body rows, 8 hinge
        rows (row ``j`` = the hinge of body ``j``; row 0 holds the root slider's gear, range and limit spring).
        Raises for a model over the caps."""
        if self.nb > MAX_BODIES or self.nd > MAX_DOF or self.obs_dim > MAX_OBS or self.act_dim > MAX_ACT:
            raise ValueError(f"PlanarChain: model {self.spec.get('name')!r} exceeds the fused-kernel caps "
                             f"({MAX_BODIES} bodies, {MAX_DOF} DOF, {MAX_OBS} observations, {MAX_ACT} actions)")
        s, t = self.spec, self.task
        tab = torch.zeros(TABLE_WORDS, dtype=torch.float64)
        vals = {**s, **t, "n_bodies": self.nb, "root_lock": self.root_lock, "kind": KINDS.index(self.kind)}
        for i, f in enumerate(_HEADER_FIELDS + _HEADER_EXTRA):
            tab[i] = float(vals[f])
        ho = TABLE_HEADER + MAX_BODIES * TABLE_BODY
        slider = dict(self.slider or dict(lo=0.0, hi=0.0, limit_k=0.0), gear=self.root_gear[0])
        for f in _SLIDER_FIELDS:
            tab[ho + _HINGE_FIELDS.index(f)] = float(slider[f])
        for j, v in enumerate(self.vel_cost):
            tab[ho + (j + 1) * TABLE_HINGE + VEL_COST_WORD] = v
        for b, body in enumerate(s["bodies"]):
            o = TABLE_HEADER + b * TABLE_BODY
            row = [body["parent"], *body["anchor"], *body["com"], body["mass"], body["inertia"], *body["caps"][0], *body["caps"][1]]
            tab[o:o + len(row)] = torch.tensor(row, dtype=torch.float64)
        for j, h in enumerate(s["hinges"]):
            o = TABLE_HEADER + MAX_BODIES * TABLE_BODY + (j + 1) * TABLE_HINGE
            tab[o:o + len(_HINGE_FIELDS)] = torch.tensor([h[f] for f in _HINGE_FIELDS], dtype=torch.float64)
        return tab.to(torch.float32)

    @staticmethod
    def unpack_table(tab):
        """The spec numbers held by a model table (the inverse of :meth:`model_table`)."""
        tab = [float(x) for x in tab.cpu()]
        out = {f: tab[i] for i, f in enumerate(_HEADER_FIELDS)}
        nb = int(out["n_bodies"])
        bodies, hinges = [], []
        for b in range(nb):
            r = tab[TABLE_HEADER + b * TABLE_BODY:TABLE_HEADER + (b + 1) * TABLE_BODY]
            bodies.append(dict(parent=int(r[0]), anchor=(r[1], r[2]), com=(r[3], r[4]), mass=r[5], inertia=r[6], caps=(tuple(r[7:11]), tuple(r[11:15]))))
        for j in range(1, nb):
            o = TABLE_HEADER + MAX_BODIES * TABLE_BODY + j * TABLE_HINGE
            hinges.append(dict(zip(_HINGE_FIELDS, tab[o:o + len(_HINGE_FIELDS)])))
        out["bodies"], out["hinges"] = tuple(bodies), tuple(hinges)
        # what a constrained root or another task kind adds (absent for a free-root "run" model)
        ho = TABLE_HEADER + MAX_BODIES * TABLE_BODY
        extra = {f: tab[len(_HEADER_FIELDS) + i] for i, f in enumerate(_HEADER_EXTRA)}
        slider = {f: tab[ho + _HINGE_FIELDS.index(f)] for f in _SLIDER_FIELDS}
        vel_cost = tuple(tab[ho + j * TABLE_HINGE + VEL_COST_WORD] for j in range(1, nb))
        if extra["root_lock"]:
            out["root_free"] = tuple(0 if int(extra["root_lock"]) >> i & 1 else 1 for i in range(3))
        if extra["kind"]:
            out["kind"] = KINDS[int(extra["kind"])]
        if out.get("kind") == "balance_tip":
            out.update(tip_x_cost=extra["tip_x_cost"], tip_goal=extra["tip_goal"], vel_cost=vel_cost)
        if slider["gear"]:
            out["root_gear"] = (slider["gear"], 0.0, 0.0)
        if slider["limit_k"]:
            out["root_slider"] = dict(lo=slider["lo"], hi=slider["hi"], limit_k=slider["limit_k"])
        return out

    # -- constants of the model as tensors ----------------------------------------------
    def _c(self, ref):
        key = (ref.dtype, ref.device)
        c = self._consts.get(key)
        if c is not None:
            return c
        o = dict(dtype=ref.dtype, device=ref.device)
        s, nb = self.spec, self.nb
        A = torch.zeros(nb, nb, **o)  # A[b, k] = 1 when body k is b or an ancestor of b
        for b in range(nb):
            k = b
            while k >= 0:
                A[b, k] = 1
                k = self.parents[k]
        caps = [(b, cap) for b, body in enumerate(s["bodies"]) for cap in body["caps"]]
        c = dict(
            A=A, Aang=torch.cat([torch.zeros(nb, 2, **o), A], 1),
            par=torch.tensor([max(p, 0) for p in self.parents], device=ref.device),
            anchor=torch.tensor([b["anchor"] if i else (0.0, 0.0) for i, b in enumerate(s["bodies"])], **o),
            com=torch.tensor([b["com"] for b in s["bodies"]], **o), mass=torch.tensor([b["mass"] for b in s["bodies"]], **o),
            inertia=torch.tensor([b["inertia"] for b in s["bodies"]], **o),
            cap_body=torch.tensor([b for b, _ in caps], device=ref.device), cap_pt=torch.tensor([cp[:2] for _, cp in caps], **o),
            cap_r=torch.tensor([cp[2] for _, cp in caps], **o), cap_on=torch.tensor([cp[3] for _, cp in caps], **o),
            body_ids=torch.arange(nb, device=ref.device),
        )
        ax = c["cap_pt"][1::2] - c["cap_pt"][0::2]
        c["axis"] = ax / ax.norm(dim=1, keepdim=True).clamp_min(1e-12)
        for f in _HINGE_FIELDS:
            c[f] = torch.tensor([h[f] for h in s["hinges"]], **o)
        c["arm_diag"] = torch.diag(torch.cat([torch.zeros(3, **o), c["armature"]]))
        c["free"] = torch.tensor(self.free, device=ref.device)
        c["free_mask"] = torch.zeros(self.nd, **o).index_fill_(0, c["free"], 1.0)
        c["act_hinges"] = torch.tensor(self.act_hinges, dtype=torch.long, device=ref.device)
        c["vel_cost"] = torch.tensor(self.vel_cost, **o)
        c["tip_pt"] = torch.tensor(s["bodies"][-1]["caps"][1][:2], **o)
        self._consts[key] = c
        return c

    # -- kinematics ---------------------------------------------------------------------
    def _kin(self, q):
        """Absolute angles (cos, sin), hinge points and CoMs of all bodies, world frame."""
        c = self._c(q)
        al = q[:, 2:] @ c["A"].T
        ca, sa = torch.cos(al), torch.sin(al)
        e = _rot(ca[:, c["par"]], sa[:, c["par"]], c["anchor"])
        hp = q[:, None, :2] + torch.einsum("bk,nkd->nbd", c["A"], e)
        cm = hp + _rot(ca, sa, c["com"])
        return dict(ca=ca, sa=sa, hp=hp, cm=cm)

    def _jac(self, k, X, body, ref):
        """Jacobian (N, np, 2, nd) of world points X (N, np, 2) fixed to the bodies ``body``."""
        c = self._c(ref)
        d = X[:, :, None, :] - k["hp"][:, None, :, :]
        ang = _perp(d) * c["A"][body][None, :, :, None]  # (N, np, nb, 2)
        n, npt = X.shape[0], X.shape[1]
        lin = torch.eye(2, dtype=ref.dtype, device=ref.device).expand(n, npt, 2, 2)
        return torch.cat([lin, ang.transpose(2, 3)], 3)

    def _mass_matrix(self, k, Jc, ref):
        c = self._c(ref)
        M = torch.einsum("nbdi,b,nbdj->nij", Jc, c["mass"], Jc)
        return M + torch.einsum("bi,b,bj->ij", c["Aang"], c["inertia"], c["Aang"]) + c["arm_diag"]

    def mass_matrix(self, q):
        k = self._kin(q)
        return self._mass_matrix(k, self._jac(k, k["cm"], self._c(q)["body_ids"], q), q)

    def momenta(self, q, u):
        """Generalized momenta ``π = M(q) u = ∂T/∂u`` (the root's angular one about the root point)."""
        return (self.mass_matrix(q) @ u[..., None])[..., 0]

    def _dTdq_from(self, k, Jc, u, ref):
        c = self._c(ref)
        vc = torch.einsum("nbdi,ni->nbd", Jc, u)
        vh = torch.einsum("nbdi,ni->nbd", self._jac(k, k["hp"], c["body_ids"], ref), u)
        Ps = torch.einsum("bk,b,nbd->nkd", c["A"], c["mass"], vc)  # linear momentum of every subtree
        return torch.cat([torch.zeros_like(u[:, :2]), vh[..., 1] * Ps[..., 0] - vh[..., 0] * Ps[..., 1]], 1)

    def dTdq(self, q, u):
        """``∂T/∂q`` at fixed ``u`` (N, nd), closed form: 0 for the translations and
        ``v_hinge,z·P_x − v_hinge,x·P_z`` of the subtree for every angle."""
        k = self._kin(q)
        return self._dTdq_from(k, self._jac(k, k["cm"], self._c(q)["body_ids"], q), u, q)

    def kinetic_energy(self, q, u):
        """T of the whole system from the link velocities, propagated down the tree (independent of
        the Jacobian / mass-matrix assembly; the tests differentiate it to check M, π and ∂T/∂q)."""
        c, k = self._c(q), self._kin(q)
        w, vh = [u[:, 2]], [u[:, :2]]
        T = 0.5 * (c["armature"] * u[:, 3:] ** 2).sum(1)
        for b in range(self.nb):
            if b > 0:
                p = self.parents[b]
                w.append(w[p] + u[:, 2 + b])
                vh.append(vh[p] + w[p][:, None] * _perp(k["hp"][:, b] - k["hp"][:, p]))
            vc = vh[b] + w[b][:, None] * _perp(k["cm"][:, b] - k["hp"][:, b])
            T = T + 0.5 * c["mass"][b] * (vc * vc).sum(1) + 0.5 * c["inertia"][b] * w[b] ** 2
        return T

    def momentum(self, s):
        """Total linear momentum (N, 2) and angular momentum about the world origin (N,)."""
        q, u = s[:, :self.nd], s[:, self.nd:2 * self.nd]
        pi = self.momenta(q, u)
        return pi[:, :2], pi[:, 2] + q[:, 0] * pi[:, 1] - q[:, 1] * pi[:, 0]

    def initial_momenta(self, s):
        P, L = self.momentum(s)
        return P, L, self.momenta(s[:, :self.nd], s[:, self.nd:2 * self.nd])[:, 3:]

    # -- dynamics -----------------------------------------------------------------------
    def _substep(self, q, u, mom, tau, root_force=0.0):
        c, S = self._c(q), self.spec
        dt, nb = S["dt"], self.nb
        q = q + dt * u
        k = self._kin(q)
        Jc = self._jac(k, k["cm"], c["body_ids"], q)
        # generalized external force Q (N, nd); Q[:, 2] is the torque about the root point
        Fg = torch.zeros_like(k["cm"])
        Fg[..., 1] = -S["gravity"] * c["mass"]
        Q = torch.einsum("nbdi,nbd->ni", Jc, Fg)
        if S["fluid_cn"] or S["fluid_ct"] or S["fluid_cw"]:
            vc = torch.einsum("nbdi,ni->nbd", Jc, u)
            t = _rot(k["ca"], k["sa"], c["axis"])
            n = _perp(t)
            F = -S["fluid_cn"] * (vc * n).sum(-1, keepdim=True) * n - S["fluid_ct"] * (vc * t).sum(-1, keepdim=True) * t
            w = u[:, 2:] @ c["A"].T
            Q = Q + torch.einsum("nbdi,nbd->ni", Jc, F) - S["fluid_cw"] * (w @ c["Aang"])
        if S["lin_damp"] or S["ang_damp"]:
            Q = Q + torch.cat([-S["lin_damp"] * u[:, :2], -S["ang_damp"] * u[:, 2:3], torch.zeros_like(u[:, 3:])], 1)
        if S["contact_k"]:
            X = k["hp"][:, c["cap_body"]] + _rot(k["ca"][:, c["cap_body"]], k["sa"][:, c["cap_body"]], c["cap_pt"])
            Jx = self._jac(k, X, c["cap_body"], q)
            vx = torch.einsum("npdi,ni->npd", Jx, u)
            pen = torch.clamp(c["cap_r"] - X[..., 1], min=0) * c["cap_on"]
            fn = torch.clamp(S["contact_k"] * pen - S["contact_c"] * vx[..., 1] * (pen > 0), min=0)
            ft = -S["mu"] * fn * vx[..., 0] / torch.sqrt(vx[..., 0] ** 2 + S["eps_v"] ** 2)
            Q = Q + torch.einsum("npdi,npd->ni", Jx, torch.stack([ft, fn], -1))
        phi, phid = q[:, 3:], u[:, 3:]
        lim = torch.clamp(c["lo"] - phi, min=0) - torch.clamp(phi - c["hi"], min=0)
        tj = tau - c["damping"] * phid - c["stiffness"] * (phi - c["rest"]) + c["limit_k"] * lim
        dT = self._dTdq_from(k, Jc, u, q)
        if self.root_gear[0] or self.slider:  # the driven slider of root x, with its limit spring
            fx = self.root_gear[0] * root_force
            if self.slider:
                sl = self.slider
                fx = fx + sl["limit_k"] * (torch.clamp(sl["lo"] - q[:, 0], min=0) - torch.clamp(q[:, 0] - sl["hi"], min=0))
            Q = torch.cat([(Q[:, 0] + fx)[:, None], Q[:, 1:]], 1)
        if self.root_lock:
            # generalized momenta of the free coordinates, advanced directly (π_θ about the root point); a locked
            # coordinate's row takes a constraint force that is never computed, and the row is never read
            pi = mom + dt * (torch.cat([Q[:, :3], Q[:, 3:] + tj], 1) + dT)
            F = c["free"]
            M = self._mass_matrix(k, Jc, q)[:, F][:, :, F]
            uf = torch.cholesky_solve(pi[:, F, None], torch.linalg.cholesky_ex(M).L)[..., 0]
            return q, torch.zeros_like(u).index_copy_(1, F, uf), pi
        P, L, pj = mom
        P = P + dt * Q[:, :2]
        L = L + dt * (Q[:, 2] + q[:, 0] * Q[:, 1] - q[:, 1] * Q[:, 0])
        pj = pj + dt * (tj + Q[:, 3:] + dT[:, 3:])
        pi = torch.cat([P, (L - (q[:, 0] * P[:, 1] - q[:, 1] * P[:, 0]))[:, None], pj], 1)
        M = self._mass_matrix(k, Jc, q)
        u = torch.cholesky_solve(pi[..., None], torch.linalg.cholesky_ex(M).L)[..., 0]  # a non-finite state stays non-finite (unhealthy)
        return q, u, (P, L, pj)

    def tip(self, q):
        """World position (N, 2) of the far end cap of the last body."""
        c, k = self._c(q), self._kin(q)
        return k["hp"][:, -1] + _rot(k["ca"][:, -1], k["sa"][:, -1], c["tip_pt"])

    def healthy(self, s):
        t = self.task
        finite = torch.isfinite(s).all(1)
        if self.kind == "balance":
            return ((s[:, 2] + s[:, 3]).abs() < t["pitch_max"]) & finite
        if self.kind == "balance_tip":
            return (self.tip(s[:, :self.nd])[:, 1] > t["z_lo"]) & finite
        if self.kind == "reach":
            return finite
        z, th = s[:, 1], s[:, 2]
        return (z > t["z_lo"]) & (z < t["z_hi"]) & (th.abs() < t["pitch_max"]) & finite

    def obs(self, s):
        nd = self.nd
        q, u = s[:, :nd], s[:, nd:2 * nd]
        if self.kind == "run":
            clip = self.task["vel_clip"]
            if clip:
                u = torch.clamp(u, -clip, clip)
            if not self.root_lock:
                return torch.cat([q[:, self.obs_skip:], u], 1)
        F = self._c(s)["free"]
        if self.kind in ("run", "balance"):
            return torch.cat([q[:, F][:, self.obs_skip:], u[:, F]], 1)
        phi = q[:, 3:]
        if self.kind == "balance_tip":
            return torch.cat([q[:, F[:self.n_free_root]], torch.sin(phi), torch.cos(phi), u[:, F]], 1)
        target = s[:, 2 * nd:]
        return torch.cat([torch.cos(phi), torch.sin(phi), target, u[:, 3:], self.tip(q) - target, torch.zeros_like(q[:, :1])], 1)

    def reset(self, key, n):
        S = self.spec
        k1, k2 = rnd.split(key)
        q = torch.tensor(list(S["root_init"]) + [h["init"] for h in S["hinges"]], dtype=torch.float32)
        dq = S["reset_noise"] * (rnd.uniform(k1, (self.nd,)).to(torch.float32) * 2 - 1)
        u = S["reset_noise"] * rnd.normal(k2, (self.nd,)).to(torch.float32)
        if self.root_lock:  # a locked coordinate starts at root_init exactly, at rest
            free = self._c(q)["free_mask"]
            dq, u = dq * free, u * free
        parts = [q + dq, u]
        if self.kind == "reach":  # the target: uniform in a disc, from a key of its own
            r, ang = rnd.uniform(rnd.fold_in(key, 1), (2,)).to(torch.float32)
            rad = self.task["target_radius"] * torch.sqrt(r)
            parts.append(torch.stack([rad * torch.cos(2 * math.pi * ang), rad * torch.sin(2 * math.pi * ang)]))
        s = torch.cat(parts).expand(n, self.state_dim).clone()
        return s, self.obs(s)

    def step(self, s, action):
        S, t = self.spec, self.task
        c = self._c(s)
        nd = self.nd
        a = torch.clamp(action.to(s.dtype), -1.0, 1.0)
        root_force = 0.0
        if not self.root_gear[0] and len(self.act_hinges) == self.nj:  # every hinge is driven and nothing else
            tau = c["gear"] * a
        else:  # the root slider's column first, then the driven hinges in body order; a passive hinge takes none
            na_root = 1 if self.root_gear[0] else 0
            if na_root:
                root_force = a[:, 0]
            tau = torch.zeros_like(s[:, :self.nj]).index_copy_(1, c["act_hinges"], c["gear"][c["act_hinges"]] * a[:, na_root:])
        q, u, aux = s[:, :nd], s[:, nd:2 * nd], s[:, 2 * nd:]
        x0 = q[:, 0]
        mom = self.momenta(q, u) if self.root_lock else self.initial_momenta(s)
        for _ in range(S["substeps"]):
            q, u, mom = self._substep(q, u, mom, tau, root_force)
        s = torch.cat([q, u, aux], 1) if self.n_aux else torch.cat([q, u], 1)
        healthy = self.healthy(s)
        ctrl = t["ctrl_cost"] * (a * a).sum(1)
        if self.kind == "run":
            reward = (q[:, 0] - x0) / (S["dt"] * S["substeps"]) + t["healthy_reward"] - ctrl
        elif self.kind == "balance":
            reward = t["healthy_reward"] - ctrl
        elif self.kind == "balance_tip":
            tip = self.tip(q)
            reward = t["healthy_reward"] - (t["tip_x_cost"] * tip[:, 0] ** 2 + (tip[:, 1] - t["tip_goal"]) ** 2) - (c["vel_cost"] * u[:, 3:] ** 2).sum(1)
        else:
            reward = -(self.tip(q) - aux).norm(dim=1) - ctrl
        reward = torch.where(healthy, reward, torch.zeros_like(reward))
        return s, self.obs(s), reward, ~healthy

    # -- rendering ----------------------------------------------------------------------
    def render(self, state, width=320, height=240, span=None):
        """``(H, W, 3) uint8`` side view of one state ``(state_dim,)``: links as thick segments, the ground
        line at ``z = 0`` (models with contacts only), the reach task's target as a dot, the camera centred on the root."""
        s = state.detach().to("cpu", torch.float64).reshape(1, -1)
        c, k = self._c(s), self._kin(s[:, :self.nd])
        X = (k["hp"][:, c["cap_body"]] + _rot(k["ca"][:, c["cap_body"]], k["sa"][:, c["cap_body"]], c["cap_pt"]))[0].numpy()
        r = c["cap_r"].numpy()
        span = span or 2.5 * max(1.0, float(np.abs(c["cap_pt"].numpy()).max()) * 2)
        cx, cz = float(s[0, 0]), (float(s[0, 1]) if not self.spec["contact_k"] else 0.35 * span)
        px = cx + (np.arange(width) + 0.5 - width / 2) * span / width
        pz = cz - (np.arange(height) + 0.5 - height / 2) * span / width
        gx, gz = np.meshgrid(px, pz)
        img = np.full((height, width, 3), 235, np.uint8)
        if self.spec["contact_k"]:
            img[gz < 0] = (120, 100, 80)
            tick = (np.floor(gx) % 2 == 0) & (gz < 0) & (gz > -0.05 * span)
            img[tick] = (70, 60, 50)
        for b in range(self.nb):
            p0, p1, rad = X[2 * b], X[2 * b + 1], max(float(r[2 * b]), 1.5 * span / width)
            d = p1 - p0
            tpar = np.clip(((gx - p0[0]) * d[0] + (gz - p0[1]) * d[1]) / max(float(d @ d), 1e-12), 0, 1)
            dist = np.hypot(gx - (p0[0] + tpar * d[0]), gz - (p0[1] + tpar * d[1]))
            img[dist <= rad] = (200, 60, 40) if b == 0 else (40, 90 + 20 * (b % 3), 200)
        if self.kind == "reach":  # the target
            tx, tz = (float(v) for v in s[0, 2 * self.nd:])
            img[np.hypot(gx - tx, gz - tz) <= max(0.009, 2.0 * span / width)] = (40, 160, 60)
        return torch.from_numpy(img)


@register("hopper")
class Hopper(PlanarChain):
    """Brax-style Hopper (11 observations / 3 actions), not bit-compatible with Brax / MuJoCo.

    Torso 0.4 (root at its centre, start height 1.25), thigh 0.45, leg 0.5, foot 0.39 (heel −0.13 …
    toe 0.26); radii 0.05 / 0.05 / 0.04 / 0.06; masses 3.53 / 3.93 / 2.71 / 5.09; gear 200, armature 1,
    damping 1, ranges [−150°, 0], [−150°, 0], [−45°, 45°] with limit springs of 2000 N·m/rad; contacts
    k = 20000, c = 300, μ = 1, ε_v = 0.1 at the torso ends, the knee and the foot's heel and toe; 4 sub-steps
    of 2 ms per 8 ms control step.  Observation ``q[1:] ++ clip(u, ±10)``; reward = forward velocity
    + 1 − 1e-3‖a‖²; ends when root z ≤ 0.7, |θ| ≥ 0.2 or the state is non-finite."""

    SPEC = HOPPER


@register("walker2d")
class Walker2d(PlanarChain):
    """Brax-style Walker2d (17 / 6), not bit-compatible with Brax / MuJoCo.

    The hopper's torso with the hopper's leg twice, feet 0.2 (heel at the ankle), foot mass 2.94;
    gear 100, armature 0.3, damping 1 (explicit integration at 2 ms needs them), limit springs 1000; contacts and stepping as the hopper.
    Observation ``q[1:] ++ clip(u, ±10)``; reward = forward velocity + 1 − 1e-3‖a‖²; ends when root z
    leaves (0.8, 2.0), |θ| ≥ 1 or the state is non-finite."""

    SPEC = WALKER2D


@register("halfcheetah")
class HalfCheetah(PlanarChain):
    """Brax-style HalfCheetah (17 / 6), not bit-compatible with Brax / MuJoCo.

    Torso 1.0 (root at its centre, start height 0.7, radius 0.046 everywhere); back leg from the rear
    end: thigh (0.16, −0.25), shin (−0.28, −0.14), foot (0.06, −0.19); front leg from the front end:
    thigh (−0.14, −0.24), shin (0.13, −0.18), foot (0.09, −0.14); masses 6.36 / 1.54 / 1.58 / 1.07 / 1.43 /
    1.18 / 0.85 (total 14.01); gears 120 / 90 / 60 / 120 / 60 / 30, stiffness 240 / 180 / 120 / 180 / 120 / 60,
    damping 6 / 4.5 / 3 / 4.5 / 3 / 1.5, armature 1 (at 0.1 the 10 ms explicit step amplifies float32 rounding to O(1) within 20 control steps), limit springs 200; contacts k = 5000, c = 100, μ = 1, ε_v = 0.3
    at the torso ends and every link's far end; 5 sub-steps of 10 ms per 50 ms control step.
    Observation ``q[1:] ++ u``; reward = forward velocity − 0.1‖a‖²; never ends (non-finite only)."""

    SPEC = HALFCHEETAH


@register("swimmer")
class Swimmer(PlanarChain):
    """Brax-style Swimmer (8 / 2), not bit-compatible with Brax / MuJoCo.

    Three links of 1.0 (mass 30 each, radius 0.1) in a horizontal plane, the root point at the head
    tip; gear 150, armature 1, joint damping 30, range ±100° with limit springs 2000; no gravity and no contacts;
    anisotropic viscous drag per link ``−c_n (v·n) n − c_t (v·t) t`` at the CoM with c_n = 300,
    c_t = 30 and ``−c_ω ω`` with c_ω = 30; 4 sub-steps of 10 ms per 40 ms control step.
    Observation ``q[2:] ++ u``; reward = forward velocity − 1e-4‖a‖²; never ends (non-finite only)."""

    SPEC = SWIMMER


@register("inverted_pendulum")
class InvertedPendulum(PlanarChain):
    """Brax-style InvertedPendulum (4 observations / 1 action), not bit-compatible with Brax / MuJoCo.

    A cart (capsule 0.2 long, radius 0.1, mass 10.5) on a rail: the root is free in x only (z and θ locked at 0).
    The pole (0.6 long, radius 0.049, mass 5) stands upright at φ = 0 on a passive hinge (gear 0, damping 0.05, no
    armature, no range).  The one action drives the slider with gear 100; slider damping 1, range ±1 with a limit
    spring of 5000 N/m.  Gravity 9.81, no contacts; 10 sub-steps of 2 ms per 20 ms control step (the explicit step
    gains energy once the pole whirls; that lies behind the termination rule).  Observation ``(x, φ, ẋ, φ̇)``;
    reward = 1 while healthy; ends when |φ| ≥ 0.2 or the state is non-finite.  Reset noise 0.01."""

    SPEC = INVERTED_PENDULUM


@register("inverted_double_pendulum")
class InvertedDoublePendulum(PlanarChain):
    """Brax-style InvertedDoublePendulum (8 / 1), not bit-compatible with Brax / MuJoCo.

    The inverted pendulum's cart (mass 10.5, root free in x only) with two poles of 0.6 (radius 0.045, mass 4.2
    each) on passive hinges (damping 0.05, no armature, no range).  Slider gear 500, damping 1, range ±1 with a
    limit spring of 5000 N/m.  Gravity 9.81, no contacts; 20 sub-steps of 1 ms per 20 ms control step: released
    from 0.01 rad the explicit step multiplies the energy by 200 within 75 control steps at 10 ms and only drifts
    at 1 ms, and the tip is below 1 long before the poles whirl.  Observation ``(x, sin φ₁, sin φ₂, cos φ₁,
    cos φ₂, ẋ, φ̇₁, φ̇₂)``; reward = 10 − (0.01·x_tip² + (z_tip − 2)²) − 1e-3·φ̇₁² − 5e-3·φ̇₂², the tip being the
    far end of the second pole; ends when z_tip ≤ 1 or the state is non-finite.  Reset noise 0.05."""

    SPEC = INVERTED_DOUBLE_PENDULUM


@register("reacher")
class Reacher(PlanarChain):
    """Brax-style Reacher (11 / 2), not bit-compatible with Brax / MuJoCo.

    A two-link arm in a horizontal plane (gravity 0, no contacts) on a fully locked root (a base of mass 1 that
    never moves).  Links 0.1 and 0.11 (radius 0.01, masses 0.0356 / 0.0387); both hinges gear 200, armature 1,
    damping 1; the second has range ±3 with a limit spring of 1000 N·m/rad.  The link inertia of about 1e-4 is
    dominated by the armature (with armature 0 the step diverges).  2 sub-steps of 10 ms per 20 ms control step.
    The target is drawn at reset, uniform in a disc of radius 0.2, and rides in the state's two last words.
    Observation ``cos φ (2), sin φ (2), target (2), φ̇ (2), tip − target (2), 0``; reward = −‖tip − target‖ −
    ‖a‖²; never ends (non-finite only).  Reset noise 0.1."""

    SPEC = REACHER
