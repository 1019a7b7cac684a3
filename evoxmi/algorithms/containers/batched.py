"""Independent runs of one algorithm as ONE batched computation.

The fork's benchmark protocol runs every DE variant 32 times per CEC'22 function
(reference ``run/run_de.py:54-114``): at D = 20 and pop = 100 a generation is a few
hundred tiny kernels, so one run at a time leaves the GPU idle between launches.
``BatchedRuns(algorithm, n_runs)`` keeps the n_runs states stacked along a leading
axis and executes ``ask``/``tell`` once for all of them with ``torch.func.vmap`` —
the reference's own mechanism for independent copies (``jax.vmap``) — so a launch
sequence advances every run.  The evaluation sees one (n_runs·pop, d) matrix.

Run ``r`` starts from ``split(key, n_runs)[r]`` and is bit-identical to running the
algorithm alone from that key (``tests/test_batched_runs.py``).  The HIP ops used by the
DE zoo (Philox streams, the fused trial kernel, sorts) carry vmap rules that fold the run
axis into their launch (``evoxmi/ops/batching.py``), so a batched generation costs the
same number of launches as a single run.

NSGA-II and GDE3 batch the same way (``tests/test_batched_mo.py``, ``tests/test_batched_mo_gpu.py``):
on a HIP device their non-dominated sort, NSGA-II selection, SBX and polynomial mutation have
batched forms with one workgroup (or one grid row) per run (``nds_batched.hip``, ``nsga_select.hip``,
``evo_ops.hip``), for merged populations of at most 8192 rows and 8 objectives per run; above those
caps the batched step raises ``NotImplementedError`` instead of falling back to one launch per run.
On the CPU their environmental selection, which has data-dependent control flow, runs run by run
inside one op (``evoxmi.ops.nds.nsga2_survivors_torch``).

IBEA and SPEA2 batch too (``tests/test_batched_ibea_spea2.py``, ``tests/test_batched_ibea_spea2_gpu.py``).  Every
kernel of ``ibea_select.hip`` and ``spea2_select.hip`` takes a run index: the fitness passes put the run on the grid
and the removal loops, which run in one workgroup, get a workgroup per run, so R loops run at once on R compute
units (merged populations of at most 8192 rows and 16 objectives per run; above that the batched step raises
``NotImplementedError``).  SPEA2's runs each count their own removals.  On the CPU SPEA2's fitness and selection
run run by run inside Python-registered ops (``evoxmi.ops.spea2``); IBEA's torch path is traced by ``vmap`` itself.

CMA-ES batches on a HIP device through ``CMAES(..., fused_small=True)`` (d ≤ 64, λ ≤ 1024; ``tests/test_cma_small_gpu.py``): its
ask and tell are two ops with one workgroup per run (``cma_small.hip``), so R seeds advance with the launches of one and run r is
bit-identical to the flagged algorithm alone.  ``BatchedRuns(CMAES)`` without the flag works on the CPU only: on a device its
tell goes through ops without a vmap rule.

MOEA/D batches as well (``tests/test_batched_moead.py``, ``tests/test_batched_moead_gpu.py``): on a HIP device a generation is the two
launches of ``moead_small.hip`` — a wave per offspring draws its parents and varies its genes; one workgroup per run forms the
reference points, replaces without a reverse-neighbour CSR and selects the rows — for the default SBX(type 2) + polynomial-mutation
pipeline, float32 and at most 2048 subproblems and 16 objectives per run (``NotImplementedError`` otherwise); on the CPU its tell runs
run by run inside a Python-registered op.  ``MOEADDRA``, ``EAGMOEAD`` and ``MOEADM2M`` are not covered.

NSGA-III batches (``tests/test_batched_nsga3.py``, ``tests/test_nsga3_assoc_gpu.py``): after the batched non-dominated sort its tell is
four launches that take a run index — one workgroup per run finds the last rank, the ideal point, the extremes and the nadir, a grid row
per run associates every row with its reference point (``nsga3_assoc.hip``, float64, no (n, K) array), and one workgroup per run does
the niching (``nsga3_select.hip``) — for merged populations of at most 8192 rows, 8 objectives and 8192 reference points per run
(``NotImplementedError`` above).  The solo algorithm runs the same kernels, so run r is bit-identical to it.  On the CPU the tell's
selection runs run by run inside a Python-registered op (``evoxmi.ops.nsga3.survivors_run``).

HypE batches (``tests/test_batched_hype.py``, ``tests/test_batched_hype_gpu.py``): its Monte-Carlo fitness is ``ops.geom.hype_fitness``, on a
HIP device the two launches of ``hype_fitness.hip`` with the run on ``grid.y`` (no sample array; merged populations of at most 2048 rows,
16 objectives and 2^20 samples per run, and the non-dominated sort's 8192 rows and 8 objectives; ``NotImplementedError`` above), bit-identical
to the two-pass path it replaces, so the solo trajectory did not move.  On the CPU its non-dominated sort runs run by run inside a
Python-registered op (``evoxmi.ops.nds.rank_under_vmap``).

RVEA batches (``tests/test_batched_rvea.py``, ``tests/test_batched_rvea_gpu.py``): on a HIP device its APD selection, five launches
for one run, is ONE launch of ``rvea_small.hip`` for all of them, a workgroup per run that keeps the run's normalised reference
vectors, γ and the per-vector minima in LDS (no scratch, no global atomics), each run with its own adapted vectors and θ.  It gives
every run the words of the solo kernels, for merged populations of at most 4096 rows and 2048, 1024 or 512 reference vectors at up to
4, 8 or 16 objectives per run (``NotImplementedError`` above); the rest of its tell is torch ops that ``vmap`` batches itself.
RVEA* and LMOCSO, which share the solo kernels, are not covered: their ``rvea_cos_best`` raises under ``vmap``.

θ-DEA batches (``tests/test_batched_tdea.py``, ``tests/test_batched_tdea_gpu.py``): on a HIP device its θ-ranking, four launches for one
run, is ONE launch of ``tdea_small.hip`` for all of them, a workgroup per run that keeps the run's normalised directions, θ, and then
cls, val and the clusters' member lists in LDS (no scratch, no global atomics) and counts a row's rank inside its own cluster only.  It
gives every run the words of the solo kernels, within the caps of RVEA's batched selection (``NotImplementedError`` above) and the
non-dominated sort's 8192 rows and 8 objectives; the rest of its tell is torch ops that ``vmap`` batches itself.  On the CPU its
non-dominated sort and its θ-ranking run run by run inside Python-registered ops (``evoxmi.ops.nds.rank_under_vmap``,
``evoxmi_py::tdea_theta_rank_run``).

SRA batches (``tests/test_batched_sra.py``, ``tests/test_batched_sra_gpu.py``): on a HIP device its selection, two launches for one
run with the ranking on a single compute unit, is ONE launch of ``sra_small.hip`` for all runs, a workgroup per run that forms both
indicators from the run's rows in LDS and ranks them without writing them to global memory in between, each run with its own pc.  It
gives every run the words of the solo kernels, for merged populations of at most 2048 rows at up to 8 objectives and 1024 at up to 16
(``NotImplementedError`` above).  On the CPU the selection runs run by run inside a Python-registered op (``evoxmi.ops.sra.select_run``).

BiGE batches (``tests/test_batched_bige.py``, ``tests/test_batched_bige_gpu.py``): on a HIP device a bi-goal estimate and the
non-dominated sort of its result, three launches and a sort for one run, are ONE launch of ``bige_small.hip`` for all runs, a workgroup
per run that keeps the run's normalised rows and proximities in LDS (no scratch, no global atomics), forms the crowding degree in the
solo kernel's sum order and ranks the bi-goal pairs there.  It gives every run the words of the solo kernels, for merged populations of
at most 2048, 1024 or 512 rows at up to 4, 8 or 16 objectives per run (``NotImplementedError`` above) and the non-dominated sort's 8
objectives.  On the CPU its non-dominated sort and its estimate run run by run inside Python-registered ops
(``evoxmi.ops.nds.rank_under_vmap``, ``evoxmi_py::bige_estimate_rank_run``).

On the CPU the float32 powers of SBX and polynomial mutation are taken run by run under ``vmap`` (``utils.common.pow_under_vmap``):
torch's CPU ``pow`` rounds an element by its place in the tensor, so the power of the stacked runs is not the power of each run.

Covered multi-objective algorithms: NSGA-II, GDE3, IBEA, SPEA2, MOEA/D, NSGA-III, HypE, RVEA, SRA, θ-DEA, BiGE.  The others are not, and an uncovered
one is not guaranteed to raise, though most do, from ``vmap`` (their selections read the host or loop on data) or from an op's rule:
do not rely on ``BatchedRuns`` over an algorithm that is not listed here.
"""
from __future__ import annotations

import torch
from torch.func import vmap

from ...core import Algorithm, State
from ...ops import random as rnd


class BatchedRuns(Algorithm):
    def __init__(self, algorithm: Algorithm, n_runs: int):
        super().__init__()
        self._base = algorithm  # underscore: not a child module (its states live in `runs`)
        self.n_runs = int(n_runs)
        self.pop_size = getattr(algorithm, "pop_size", None)
        from ...ops import batching

        batching.register()  # vmap rules of the HIP ops (no-op cost after the first call)

    def wraps_init_ask(self):
        from ...core.algorithm import algorithm_has_init_ask

        return algorithm_has_init_ask(self._base)

    def run_keys(self, key):
        return rnd.split(key, self.n_runs)

    def setup(self, key):
        keys = self.run_keys(key)
        runs = vmap(self._base.init)(keys)
        return State(runs=runs)

    def _flat(self, pop):
        return pop.reshape((-1,) + tuple(pop.shape[2:]))

    def init_ask(self, state):
        if not self.wraps_init_ask():
            return None, state
        pop, runs = vmap(self._base.init_ask)(state.runs)
        return self._flat(pop), state.update(runs=runs)

    def init_tell(self, state, fitness):
        f = fitness.reshape((self.n_runs, -1) + tuple(fitness.shape[1:]))
        return state.update(runs=vmap(self._base.init_tell)(state.runs, f))

    def ask(self, state):
        pop, runs = vmap(self._base.ask)(state.runs)
        return self._flat(pop), state.update(runs=runs)

    def tell(self, state, fitness):
        f = fitness.reshape((self.n_runs, -1) + tuple(fitness.shape[1:]))
        return state.update(runs=vmap(self._base.tell)(state.runs, f))

    # ---------------------------------------------------------------- harness helpers
    def set_field(self, state, **fields):
        """Write a (scalar or per-run) value into every run's state, e.g. the fork's
        wall-clock ``progress`` injection (reference run/run_de.py:90-94)."""
        runs = state.runs
        upd = {}
        for k, v in fields.items():
            old = runs[k]
            v = torch.as_tensor(v, dtype=old.dtype, device=old.device) if not isinstance(v, torch.Tensor) else v.to(old.device, old.dtype)
            upd[k] = v.expand_as(old).clone() if v.shape != old.shape else v
        return state.update(runs=runs.update(**upd))

    def best_fitness(self, state):
        """Best fitness of every run, (n_runs,)."""
        return state.runs.fitness.reshape(self.n_runs, -1).min(1).values
