"""CMA-ES at benchmark dimensions: the one-workgroup generation (``CMAES(fused_small=True)``) against the default path.

CEC 2022 F1 at D = 10 and D = 20, default λ (10 and 12), one MI355X, every generation replayed from a hipGraph:

  fused_batched : BatchedRuns(CMAES(fused_small=True), R) — one generation of all R runs (default R = 32)
  fused_solo    : CMAES(fused_small=True), one run
  default_solo  : CMAES(), one run — the yardstick; R sequential seeds cost R times this (``default_x_runs_ms``).
                  At D = 10 (not a multiple of 4) its eigensolver is a host phase between graph segments.

Each configuration is warmed up, then timed in three alternating rounds of --gens generations between device events; the
JSON line per dimension carries every round, the median, the kernel launches of one eager generation (torch profiler;
null when the profiler is unavailable) and the Jacobi sweeps of the fused runs' last solve.

python tools/bench_cma_small.py [--runs 32] [--gens 200] [--warmup 20] [--out profiles/cma_small_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def make(name, d, runs, dev):
    from evoxmi.algorithms import CMAES
    from evoxmi.algorithms.containers.batched import BatchedRuns

    base = CMAES(torch.zeros(d, device=dev), 10.0, fused_small=name != "default_solo")
    return BatchedRuns(base, runs) if name == "fused_batched" else base


def launches_per_generation(name, d, runs, dev):
    """Kernel launches of one eager generation (after two warm-up generations)."""
    from torch.profiler import ProfilerActivity, profile

    from evoxmi import random as rnd
    from evoxmi.problems.numerical import CEC2022TestSuit
    from evoxmi.workflows import StdWorkflow

    try:
        wf = StdWorkflow(make(name, d, runs, dev), CEC2022TestSuit.create(1), graph=False)
        st = wf.init(rnd.PRNGKey(7, device=dev))
        for _ in range(3):
            st = wf.step(st)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            st = wf.step(st)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower())
        return n or None
    except Exception as e:  # a figure that could not be taken is reported as such, never guessed
        print(f"bench_cma_small.py: launches of {name} not counted: {e!r}", file=sys.stderr, flush=True)
        return None


def main():
    from evoxmi import random as rnd
    from evoxmi.problems.numerical import CEC2022TestSuit
    from evoxmi.workflows import StdWorkflow

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--gens", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cma_small.py times a HIP device; there is no CPU mode"
    dev = torch.device("cuda")
    names = ("fused_batched", "fused_solo", "default_solo")
    for d in args.dims:
        jobs = {}
        for name in names:
            wf = StdWorkflow(make(name, d, args.runs, dev), CEC2022TestSuit.create(1), graph=True)
            st = wf.init(rnd.PRNGKey(7, device=dev))
            for _ in range(1 + args.warmup):
                st = wf.step(st)
            jobs[name] = [wf, st]
        torch.cuda.synchronize()
        ms = {name: [] for name in names}
        for _ in range(3):  # alternating rounds: drift of the shared host shows up in every configuration alike
            for name in names:
                wf, st = jobs[name]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.gens):
                    st = wf.step(st)
                t1.record()
                t1.synchronize()
                jobs[name][1] = st
                ms[name].append(t0.elapsed_time(t1) / args.gens)
        med = {name: statistics.median(v) for name, v in ms.items()}
        runs_state = jobs["fused_batched"][1].get_child_state("algorithm").runs
        sweeps = runs_state.eig_stats[:, 1]
        out = {"bench": "cma_small", "problem": "CEC2022 F1", "dim": d, "pop": jobs["fused_solo"][0].algorithm.pop_size, "runs": args.runs,
               "gens_per_round": args.gens, "ms_per_gen": {k: round(v, 5) for k, v in med.items()},
               "ms_per_gen_rounds": {k: [round(x, 5) for x in v] for k, v in ms.items()},
               "default_x_runs_ms": round(med["default_solo"] * args.runs, 4),
               "speedup_batched_vs_sequential_default": round(med["default_solo"] * args.runs / med["fused_batched"], 2),
               "speedup_solo_vs_default": round(med["default_solo"] / med["fused_solo"], 3),
               "launches_per_gen_eager": {name: launches_per_generation(name, d, args.runs, dev) for name in names},
               "jacobi_sweeps_last_solve": {"mean": round(float(sweeps.mean()), 2), "max": int(sweeps.max())},
               "capped_solves_last_gen": int(runs_state.eig_stats[:, 3].sum()),
               "mean_finite": bool(torch.isfinite(runs_state.mean).all())}
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
