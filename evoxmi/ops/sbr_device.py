"""Device-controlled sorted-block refinement: the converged eigensolver as one capturable schedule.

The host-driven solver (:func:`evoxmi.ops.sbr.eigh_warm`) chooses every refinement
iteration's variant from statistics it reads back, so a CMA-ES generation was split into
graph segments around a host phase (``runtime.host_phase``) with a device→host read per
generation.  The reference decomposes C inside its one jitted step
(``/root/reference/src/evox/algorithms/so/es_variants/cma_es.py:155-160,193-198`` under
``std_workflow.py:203-216``); this module restores that property on MI355X:

* the solve is a FIXED schedule of ``K`` iterations (``EVOXMI_SBR_DEVICE_ITERS``), each
  the same kernel sequence as the host driver's iteration (block solves, far generator,
  X², damping, Taylor exponential, Bq·V, Newton–Schulz, Bᵀ C B) —
  ``csrc/kernels/eigh_sbr_dev.hip`` + ``gemm_ks.hip``;
* every kernel reads a device control word and returns at once when its variant is off
  for this iteration or the solve has already converged (a skipped kernel costs one
  launch boundary, ≈1.5 µs);
* the Bᵀ C B GEMM writes the convergence statistics' partials in its epilogue and one
  single-workgroup kernel per iteration reduces them and writes the next iteration's
  control words with :func:`evoxmi.ops.sbr.decide`'s rules (tolerance stop, Newton–Schulz
  while κ is large or after a damped step, damping at iteration 0 / large κ, near-only
  close to the tolerance, Taylor order 4 once κ is small, the sticky local threshold, and
  the divergence stop — which restores the warm-start basis).  The control step of slot j
  runs inside slot j + 1's rank launch (its own workgroup, ``sbr_dev_ctrl_rank``); only the
  last one is a launch of its own.

No host read, no iteration plan, no state outside the algorithm's ``State``: a solve
depends only on (C, B_prev), so a checkpoint-resumed run is bitwise identical
(``tests/test_sbr_device_gpu.py``).  The per-solve [off_rel, 0, iterations, fallback]
also go to a device ring (:meth:`DeviceSBR.history`) that benches read after timing.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Optional

import torch

from . import _ext
from .linalg import mm
from .sbr import SBRConfig, _probe_vectors

LOG_LEN = 4096

# ---------------------------------------------------------------------------- tuned constants
# (round 6: fixed here instead of ~20 EVOXMI_SBR_* knobs; each value is the round-3..5
# measurement recorded in profiles/NOTES.md)
#
# decision rules of the device control kernel (eigh_sbr_dev.hip):
#   near_only 1.5   — a near-only step at 1.5-3e-5 often left far pairs: 1.5 saved 0.25 iterations
#   theta0 1.0 / theta_kappa 0.05 — the local far threshold once κ ≤ 0.05 keeps settled solves at
#                     4 iterations (without it they stall at ≈1.3e-5)
#   thr_fac 0.3     — global far-pair threshold (0.2 / 0.5 measured slower)
#   block_sweeps 2  — one sweep per block: 7 iterations per solve instead of 4.4
#   damp_tau / damp_kappa 1.0, ns_kappa 0.3, ns_iters 2 — the damping / Newton–Schulz rules of
#                     the round-2 solver (τ 1.5 / 2 fell back)
DEVICE_CFG = dict(near_only=1.5, theta0=1.0, theta_kappa=0.05, thr_fac=0.3, block_sweeps=2, damp_tau=1.0, damp_kappa=1.0,
                  ns_kappa=0.3, ns_iters=2)
RECOVER = 2          # divergences answered by a forced damped + re-orthonormalised step
LEAN_GUARD = 1       # a lean slot whose step needs damping / NS / order 6 stops the solve (capped)
FULL_SLOTS = 5       # warm schedule: slots ≥ 5 are lean (no damping / NS / X³ kernels)
LATE_FULL_SLOTS = 3  # late schedule: damping / NS / order-6 kernels in slots 0-2 only
LATE_DAMP_SLOTS = 1  # late schedule: the damping power steps in slot 0 only (89 launches / generation)
LATE_NS_ITERS = 1    # forced Newton–Schulz steps per late solve: 1 since the end of round 6 (with x3late: 50 steps
                     # 1.3325 vs 1.3499 ms, ‖BᵀB − I‖ bounded over 600 generations, 10-seed trajectory parity
                     # passes; round 5 had kept 2 after the 5-seed parity statistic read 5.8 % > 5 %)
LEAN_MAX_N = 1024    # larger matrices keep every slot full (d = 2000 capped in a lean slot)
CW = 8               # control words per slot (eigh_sbr_dev.hip kCW)
LARGE_N_ITERS = 8    # ... and get at least 8 slots (7 capped one d = 2000 solve)


@dataclass(frozen=True)
class Schedule:
    """A fixed device schedule: ``iters`` refinement slots; slots ≥ ``lean_from`` carry no
    damping / Newton–Schulz / X³ kernels, slots ≥ ``damp_from`` no damping power steps;
    ``ns_iters`` forced Newton–Schulz iterations; ``xgate``: the damping also follows the
    generator's free bounds (cold starts)."""

    iters: int
    lean_from: Optional[int] = None
    damp_from: Optional[int] = None
    ns_iters: int = 2
    xgate: bool = False
    basis_x3: bool = False  # basis update and Newton–Schulz correction as bf16x3 (sbr_corr_prec "x3late", late level)


def schedule(level: str, n: int) -> Schedule:
    """The schedule of a CMA-ES graph variant: ``"cold"`` (every slot full, bounds-gated
    damping), ``"warm"``, ``"warm6"`` (one slot fewer) or ``"late"`` (lean tail slots) at matrix
    order ``n``; ``"deep"`` is the cold schedule with twice the slots, for decompositions that
    run only every few generations (``CMAES._decomposition_C``: the basis is several updates
    old, a divergence recovery's damped steps are slow, and the cost is amortised)."""
    from .. import config

    if level in ("cold", "deep"):
        return Schedule(int(config.get("sbr_cold_iters")) * (2 if level == "deep" else 1), None, None, DEVICE_CFG["ns_iters"],
                        True)
    late = level == "late"
    iters = int(config.get("sbr_late_iters" if late else "sbr_device_iters"))
    if level == "warm6":  # the warm schedule with one slot fewer
        iters = max(iters - 1, int(config.get("sbr_late_iters")))
    if n > LEAN_MAX_N:
        return Schedule(max(iters, LARGE_N_ITERS), None, None, DEVICE_CFG["ns_iters"], False)
    if iters >= int(config.get("sbr_cold_iters")):  # a schedule as long as the cold one keeps every slot full
        return Schedule(iters, None, None, DEVICE_CFG["ns_iters"], False)
    if late:
        # settled solves: generators ≤ ≈1 in 2-norm falling to ≈0.02 (tools/xnorm_probe.py), the basis
        # correction small against the exactly held basis — "x3late" takes it at bf16x3 here only
        return Schedule(iters, LATE_FULL_SLOTS, LATE_DAMP_SLOTS, LATE_NS_ITERS, False,
                        config.get("sbr_corr_prec") == "x3late")
    return Schedule(iters, FULL_SLOTS, None, DEVICE_CFG["ns_iters"], False)


_LEVEL = ["warm"]


@contextlib.contextmanager
def use_schedule(level: str):
    """Solves inside this context use :func:`schedule` (``level``) — the CMA-ES graph variants
    (``CMAES.graph_variant_context``)."""
    prev = _LEVEL[0]
    _LEVEL[0] = level
    try:
        yield
    finally:
        _LEVEL[0] = prev


class DeviceSBR:
    """Persistent buffers + the fixed iteration schedule for one (n, device, config)."""

    def __init__(self, n: int, device, cfg: SBRConfig, iters: int, lean_from: int = None, xgate: bool = None,
                 damp_from: int = None, basis_x3: bool = False, fold: bool = True):
        if cfg.block not in (16, 32):
            raise ValueError("the device schedule uses the shifted-layout blocks (16 / 32)")
        self.n, self.cfg, self.K = n, cfg, int(iters)
        # fold: the control step after slot j runs inside slot j + 1's rank launch (one launch per
        # slot fewer); False keeps the separate control / rank launches (bit-identical results:
        # tests/test_sbr_fold_gpu.py, and the A/B of profiles/NOTES.md)
        self.fold = bool(fold)
        # slots ≥ lean_from launch no damping / Newton–Schulz / X³ kernels (their variants are
        # only chosen in the first iterations of a warm-started solve): a skipped lean slot
        # costs 7 launch boundaries fewer
        self.lean_from = self.K if lean_from is None else min(int(lean_from), self.K)
        # slots ≥ damp_from launch no damping power steps (the late schedule keeps them in slot 0:
        # in settled solves they return at once, ≈6 launches per generation); the control kernel
        # stops the solve (capped, escalated by the host) where the κ rule would damp there
        self.damp_from = self.lean_from if damp_from is None else min(int(damp_from), self.lean_from)
        dev = torch.device(device)
        ops = _ext.ops()

        def mat():
            return torch.zeros(n, n, device=dev)

        (self.A, self.B, self.T, self.W, self.X, self.X2, self.X3, self.P, self.VT, self.Bq,
         self.G) = (mat() for _ in range(11))
        from .. import config

        sb = cfg.block
        nb = -(-n // sb)
        self.perm = torch.zeros(n, dtype=torch.int32, device=dev)
        self.Q = torch.zeros(nb * sb * sb, device=dev)
        self.dq = torch.zeros(n, device=dev)
        self.nparts = int(ops.gemm_ks_grid(n, n, 1))
        self.part = torch.zeros(4 * self.nparts, dtype=torch.float64, device=dev)
        # stats partials of X² = −X·Xᵀ (its diagonal): free bounds of ‖X‖₂ that gate the damping's
        # power iteration in the cold schedule (xgate).  (Round 6 also tried them to choose order-2
        # steps — exp(αX) − I ≈ αX + ½α²X² below ‖αX‖₂ ≤ 2e-3 — but settled solves' generators are
        # 0.02-1.2 in 2-norm (tools/xnorm_probe.py): it never fired; removed.)
        self.xgate = bool(xgate)
        self.part2 = torch.zeros(4 * self.nparts, dtype=torch.float64, device=dev) if self.xgate else None
        K = self.K
        self.hist = torch.zeros(4 * (K + 1), dtype=torch.float64, device=dev)
        self.alpha = torch.ones(K + 1, device=dev)
        self.theta = torch.zeros(max(K, 1), device=dev)
        self.ctrl = torch.ones(CW * max(K, 1), dtype=torch.int32, device=dev)
        self.st = torch.zeros(8, dtype=torch.int32, device=dev)
        self.never = torch.zeros(1, dtype=torch.int32, device=dev)
        self.V = _probe_vectors(n, str(dev))
        self.work = torch.zeros(24 * n, device=dev)
        self.w = torch.zeros(n, device=dev)
        self.w_init = torch.zeros(n, device=dev)
        self.eig_stats = torch.zeros(4, dtype=torch.float64, device=dev)
        self.log = torch.zeros(LOG_LEN, 4, dtype=torch.float64, device=dev)
        self.log_count = torch.zeros(1, dtype=torch.int32, device=dev)
        # precision tiers (round 6): the residual products (Bᵀ C B, BᵀB) stay f32-accurate
        # (bf16x6); the products that only form a correction of an exactly held matrix —
        # X², X³ and the Taylor terms of exp(αX) − I, the basis update Bq + Bq·(V − I), and
        # Newton–Schulz's T − ½T·(TᵀT − I) — run at bf16x3 (≈1e-5 of the correction's own size)
        cp = config.get("sbr_corr_prec")
        # "x3": the Taylor terms of exp(αX) − I only (X², X³, Vᵀ); "x3all": all of them; "x3late" (default): see below.
        # Trajectory parity against rocSOLVER (tests/test_eigh_sbr.py's statistic) is seed noise at
        # the 5-seed level — a 5-seed set once put x3all at 5.2 % against the 5 % bound, other sets at
        # 0.4-2.6 % — and over 15 seeds x3all +0.6 %, x3 −1.4 %, x6 +1.1 % (profiles/r6_parity_seed_sets.jsonl,
        # r6_parity_15_seeds.txt; the test now takes 10 seeds).  x3all stays opt-in: in the
        # degenerate-spectrum stress test (rank 0's rows tiled ×8, generators of norm ≈ 1, where the
        # basis correction is not small) one of 14 solves fell back to its warm start
        # "x3late": as "x3", and the basis update / Newton–Schulz correction at bf16x3 in the late
        # level's settled solves only (cold / warm solves, where generators reach norm ≈ 1 in
        # near-degenerate spectra, keep them bf16x6)
        self.corr = "x3" if cp in ("x3", "x3all", "x3late") else None
        self.corr_basis = "x3" if cp == "x3all" or (cp == "x3late" and basis_x3) else None
        self.prm = [float(cfg.tol), float(cfg.ns_kappa), float(cfg.damp_kappa), float(cfg.t4_kappa), float(cfg.near_only),
                    float(cfg.theta0), float(cfg.theta_kappa), float(self.lean_from), float(RECOVER),
                    float(LEAN_GUARD), float(self.xgate), float(self.damp_from)]

    # ------------------------------------------------------------------ pieces
    def _btcb(self, C, skip, B=None):
        """A = Bᵀ C B (symmetric output, stats partials in the epilogue)."""
        B = self.B if B is None else B
        mm(B, C, ta=True, tb=True, out=self.W, skip=skip)
        mm(self.W, B, mode=1, out=self.A, skip=skip, stat_part=self.part)

    def _ctrl(self, j, C, report=None):
        from ..core import in_capture_warmup

        # a graph capture's warm-up step (on a copy of the state) is not a solve of the run: unlogged
        warm = in_capture_warmup()
        log = self.log[:0] if warm else self.log  # log_len 0: the ctrl kernel writes no row
        seq, ring = (None, None) if (report is None or warm) else report
        _ext.ops().sbr_dev_ctrl(self.part, self.nparts, j, self.K, self.hist, self.alpha, self.theta, self.ctrl, self.st, self.prm,
                                int(self.cfg.ns_iters), self.A, self.w, self.eig_stats, self.w_init, log, self.log_count, seq, ring)

    def _ctrl_rank(self, j, shift):
        """Control step after slot ``j`` (−1: after the initial Bᵀ C B) and the ranking of slot j + 1, one launch."""
        _ext.ops().sbr_dev_ctrl_rank(self.part, self.nparts, j, self.K, self.hist, self.alpha, self.theta, self.ctrl, self.st, self.prm,
                                     int(self.cfg.ns_iters), self.A, self.w_init, shift, self.perm)

    def _iteration(self, j, C, B_in=None, report=None):
        ops = _ext.ops()
        cfg = self.cfg
        sb = cfg.block
        c = self.ctrl[CW * j : CW * j + CW]
        sk_all, sk_far, sk_damp, sk_x3, sel6, sk_ns, sel_ns, sk_copy = (c[i : i + 1] for i in range(8))
        # (mod n: with n ≤ sb/2 the half-block shift is no position of the sorted order — the rank kernels take
        # shift in [0, n), and an unreduced one sent their perm writes in front of the buffer)
        shift = ((j % 2) * (sb // 2)) % self.n
        full = j < self.lean_from
        damp_slot = j < self.damp_from
        if self.fold:
            # the previous slot's control step (it writes this slot's control words) and this slot's
            # ranking in one launch; the ranking runs whether or not the slot is skipped
            self._ctrl_rank(j - 1, shift)
            ops.sbr16_block_only_out(self.A, shift, int(cfg.block_sweeps), sb, self.perm, self.Q, self.dq, sk_all, 0.0)
        else:
            ops.sbr16_block_out(self.A, shift, int(cfg.block_sweeps), sb, self.perm, self.Q, self.dq, sk_all, 0.0)
        # far generator X and Bq = B[:, perm]·blockdiag(Q) in one launch
        # (iteration 0 reads the warm-start basis itself: no copy of it into the workspace)
        ops.sbr16_far_bq_out(self.A, self.perm, self.Q, self.dq, self.hist[4 * j : 4 * j + 4], float(cfg.thr_fac),
                             self.theta[j : j + 1], self.X, self.B if B_in is None else B_in, self.Bq, sb, sk_far, sk_all)
        corr = self.corr
        # X skew ⇒ X² = −X·Xᵀ, symmetric (upper tiles only)
        mm(self.X, self.X, tb=True, mode=1, alpha=-1.0, out=self.X2, skip=sk_far, stat_part=self.part2, stat_diag_only=True,
           prec=corr)
        if cfg.damp_tau > 0 and damp_slot:
            # three power-step launches (they return at once when the free Frobenius bound already
            # gives α = 1); α itself is formed by the prep kernel below (no_final)
            ops.sbr_damping_out(self.X2, self.V, float(cfg.damp_tau), self.alpha[j + 1 : j + 2], self.work, sk_damp, None, True,
                                self.part2)
        if full:
            # order 6 only: X³ = X²·X = −X²·Xᵀ (skew)
            mm(self.X2, self.X, tb=True, mode=2, alpha=-1.0, out=self.X3, skip=sk_x3, prec=corr)
        damp_here = cfg.damp_tau > 0 and damp_slot
        # near-only iterations (no far step): the block-rotated basis is the new basis — Bq → B
        # copied by this launch (it returns at once otherwise), no copy launch of its own
        ops.sbr_dev_prep(self.X, self.X2, self.X3, self.alpha[j + 1 : j + 2], self.P, self.VT, c, self.work if damp_here else None,
                         float(cfg.damp_tau), self.part2, self.Bq, self.B, int(corr is not None))
        # Vᵀ = M(−α) + X²·Pᵀ (order 4) or M(−α) − X³·Pᵀ (order 6): the control word selects
        # (with the tiered precision the prep wrote M − I, so this is Vᵀ − I)
        mm(self.X2, self.P, tb=True, alpha=1.0, beta=1.0, Cin=self.VT, out=self.VT, skip=sk_far, sel=sel6, A2=self.X3, alpha2=-1.0,
           prec=corr)
        # B·V → B, or into T when Newton–Schulz follows
        if corr is not None:
            # Bq + Bq·(V − I): the exact basis plus a correction product
            mm(self.Bq, self.VT, tb=True, beta=1.0, Cin=self.Bq, out=self.B, skip=sk_far, sel=sel_ns, C2=self.T, prec=self.corr_basis)
        else:
            mm(self.Bq, self.VT, tb=True, out=self.B, skip=sk_far, sel=sel_ns, C2=self.T)
        if full:
            if corr is not None:
                # E = TᵀT − I at full precision (the orthogonality residual), then T − ½T·E
                mm(self.T, self.T, ta=True, mode=1, out=self.G, skip=sk_ns, diag_add=-1.0)
                mm(self.T, self.G, tb=True, alpha=-0.5, beta=1.0, Cin=self.T, out=self.B, skip=sk_ns, prec=self.corr_basis)
            else:
                mm(self.T, self.T, ta=True, mode=1, out=self.G, skip=sk_ns)
                mm(self.T, self.G, tb=True, alpha=-0.5, beta=1.5, Cin=self.T, out=self.B, skip=sk_ns)
        self._btcb(C, sk_all)
        if not self.fold or j == self.K - 1:
            # the last slot's control step stays a launch of its own: the log, the report ring, w_out, the keep word
            self._ctrl(j, C, report)

    # ------------------------------------------------------------------ solve
    def solve(self, C: torch.Tensor, B_prev: torch.Tensor, report=None, restore: bool = True):
        """(w, B, eig_stats) with C ≈ B diag(w) Bᵀ — device buffers of this workspace, valid
        until the next solve.  Nothing is read back; capturable into a hipGraph.  ``report``:
        (int32 device counter, pinned host float64 [R, 5] ring) — the last slot's control kernel
        writes the solve's [off_rel, status, iterations, fallback, seq] there (CMAES's schedule)."""
        ops = _ext.ops()
        n = self.n
        assert C.shape == (n, n) and B_prev.shape == (n, n)
        B_prev = B_prev if B_prev.is_contiguous() else B_prev.contiguous()
        self._btcb(C, self.never, B_prev)
        if not self.fold or self.K == 0:
            self._ctrl(-1, C, report if self.K == 0 else None)
        for j in range(self.K):
            self._iteration(j, C, B_prev if j == 0 else None, report if j == self.K - 1 else None)
        # the refinement diverged, or no iteration ran (st[5] = 0): the warm-start basis is the result
        # (restore=False: the caller selects it itself from keep_word — CMA-ES's cma_eig_out)
        if restore:
            ops.sbr_dev_copy(B_prev, self.B, self.st[5:6])
        return self.w, self.B, self.eig_stats

    @property
    def keep_word(self) -> torch.Tensor:
        """int32 device word: 0 ⇒ the last solve's basis is its warm start (not written to B)."""
        return self.st[5:6]

    def history(self, last: int = None):
        """[off_rel, 0, refinement iterations, fallback] of the most recent solves (one
        device→host read — call it outside timed loops)."""
        cnt = int(self.log_count.item())
        k = min(cnt, LOG_LEN) if last is None else min(cnt, LOG_LEN, int(last))
        if k == 0:
            return torch.zeros(0, 4, dtype=torch.float64)
        idx = [(cnt - k + i) % LOG_LEN for i in range(k)]
        return self.log.cpu()[idx]


_WS = {}


def workspace(n: int, device, cfg: SBRConfig, iters: int, lean_from: int = None, xgate: bool = False,
              damp_from: int = None, basis_x3: bool = False) -> DeviceSBR:
    from .. import config

    key = (n, str(device), cfg.block, cfg.block_sweeps, cfg.thr_fac, cfg.ns_iters, cfg.damp_tau, cfg.tol, cfg.ns_kappa,
           cfg.damp_kappa, cfg.t4_kappa, cfg.near_only, cfg.theta0, cfg.theta_kappa, int(iters), lean_from, bool(xgate), damp_from,
           config.get("sbr_corr_prec"), bool(basis_x3))
    if key not in _WS:
        _WS[key] = DeviceSBR(n, device, cfg, iters, lean_from, xgate, damp_from, bool(basis_x3))
    return _WS[key]


def schedule_iters(n: int, level: str) -> int:
    """Refinement slots the ``level`` schedule runs at matrix order ``n``."""
    return schedule(level, n).iters


def device_config(ns_iters: int = None) -> SBRConfig:
    from .. import config

    kw = dict(DEVICE_CFG)
    if ns_iters is not None:
        kw["ns_iters"] = int(ns_iters)
    return SBRConfig(tol=config.get("eigh_tol"), block=config.get("sbr_block"), **kw)


def eigh_device(C: torch.Tensor, B_prev: torch.Tensor, cfg: SBRConfig = None, iters: int = None, report=None, restore: bool = True):
    """Converged-or-capped eigendecomposition of symmetric ``C`` warm-started from
    ``B_prev``, entirely on the device (see module docstring).  Returns ``(w, B, stats)``.
    ``iters``: an explicit schedule of that many slots, every slot full (tests, probes);
    default: the schedule of the active level (:func:`use_schedule`, warm outside a context).
    ``restore=False``: no restore-copy launch; a fourth value, the keep word, tells the caller
    whether B or B_prev is the basis (``ops.cma_eig_out(..., B_alt, keep)`` selects in-kernel)."""
    from .. import config

    if iters is None:
        sch = schedule(_LEVEL[0], C.shape[0])
    else:
        sch = Schedule(int(iters), None, None, DEVICE_CFG["ns_iters"], int(iters) >= int(config.get("sbr_cold_iters")))
    cfg = cfg or device_config(sch.ns_iters)
    ws = workspace(C.shape[0], C.device, cfg, sch.iters, sch.lean_from, sch.xgate, sch.damp_from, sch.basis_x3)
    out = ws.solve(C, B_prev, report, restore)
    # restore=False: (w, B, stats, keep) — B holds the result only while keep != 0, else it is B_prev
    return out if restore else (*out, ws.keep_word)


def all_histories():
    """Concatenated per-solve histories of every device workspace (bench diagnostics)."""
    out = [ws.history() for ws in _WS.values()]
    out = [h for h in out if h.shape[0]]
    return torch.cat(out) if out else torch.zeros(0, 4, dtype=torch.float64)


def history_count() -> int:
    return sum(int(ws.log_count.item()) for ws in _WS.values())


def histories_since(counts: dict):
    """Per-solve rows appended since ``counts`` (a {key: count} snapshot from
    :func:`snapshot_counts`), all workspaces concatenated."""
    rows = []
    for k, ws in _WS.items():
        new = int(ws.log_count.item()) - counts.get(k, 0)
        if new > 0:
            rows.append(ws.history(new))
    return torch.cat(rows) if rows else torch.zeros(0, 4, dtype=torch.float64)


def snapshot_counts() -> dict:
    return {k: int(ws.log_count.item()) for k, ws in _WS.items()}
