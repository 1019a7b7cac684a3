"""Time the exact hypervolume (``evoxmi.ops.hv`` / ``metrics.ExactHV``) on one GPU against the project's other ways to get
the number: the Monte-Carlo estimator ``HV(ref, 100_000)`` on the device and ``exact_hv`` on the host.

Every device figure is per call from device events: 5 warm-up calls, then 50 timed calls, in three rounds that alternate
over all cases (so a drift of the clocks or a neighbour's load shows as a spread between the rounds, not as a difference
between two cases).  ``graph`` times the replay of one captured call, which leaves the launch overheads out.  The host
baseline is a wall clock around one call (it takes seconds).

Inputs: ``front`` is |normal| rows normalised to the unit sphere, a DTLZ2-like front, measured from the reference point
1.1; ``uniform`` is rand in [0, 1]^m measured from 1.1.

python tools/bench_hv.py [--out profiles/hv_exact_bench.jsonl] [--calls 50] [--warmup 5] [--rounds 3] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from evoxmi import random as rnd  # noqa: E402
from evoxmi.metrics import HV, ExactHV, exact_hv  # noqa: E402

REF = 1.1
TOTALS = [(8192, 3), (32768, 3), (4096, 2), (2048, 4)]
CONTRIBS = [(2048, 3), (8192, 2)]
HOST = [(1024, 3), (128, 4)]


def objectives(kind: str, n: int, m: int, device) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * m + n + (7 if kind == "front" else 0))
    if kind == "front":
        t = torch.randn(n, m, generator=g).abs() + 1e-3
        return (t / t.norm(dim=1, keepdim=True)).to(device)
    return torch.rand(n, m, generator=g).to(device)


def time_calls(fn, calls: int, warmup: int) -> list:
    """Milliseconds of each of ``calls`` calls of ``fn``, from device events, after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of every n: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hv.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    shrink = (lambda n: max(16, n // 10)) if args.quick else (lambda n: n)
    ref = torch.full((1,), REF, device=dev)
    metric = ExactHV(ref)
    key = rnd.PRNGKey(0, device=dev)
    cases = []  # (name, n, m, kind, mode, fn)
    for kind in ("front", "uniform"):
        for what, shapes in (("total", TOTALS), ("contributions", CONTRIBS)):
            for n, m in shapes:
                n = shrink(n)
                objs = objectives(kind, n, m, dev)
                fn = (lambda o=objs: metric(o)) if what == "total" else (lambda o=objs: metric.contributions(o))
                cases.append((what, n, m, kind, "eager", fn))
                cases.append((what, n, m, kind, "graph", captured(fn)))
                if what == "total":
                    mc = HV(ref.expand(m), 100_000)
                    cases.append(("mc_100000", n, m, kind, "eager", lambda o=objs, mc=mc: mc(key, o)))
    rows = []
    for r in range(args.rounds):
        for what, n, m, kind, mode, fn in cases:
            ms = time_calls(fn, args.calls, args.warmup)
            rows.append({"op": what, "n": n, "m": m, "kind": kind, "mode": mode, "round": r, "calls": args.calls,
                         "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)})
            print(json.dumps(rows[-1]), flush=True)
    for n, m in HOST:  # the host routine: one call each, wall clock
        n = shrink(n)
        for kind in ("front", "uniform"):
            objs = objectives(kind, n, m, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = exact_hv(objs, ref.expand(m))
            dt = time.perf_counter() - t0
            ours = float(metric(objs))
            rows.append({"op": "host_exact_hv", "n": n, "m": m, "kind": kind, "mode": "host", "calls": 1, "ms_median": round(dt * 1e3, 2),
                         "rel_diff_to_device": abs(ours - host) / host})
            print(json.dumps(rows[-1]), flush=True)
    for what, n, m, kind, mode, fn in cases:  # what the timed calls computed
        if mode == "eager" and what != "contributions":
            rows.append({"op": what, "n": n, "m": m, "kind": kind, "value": float(fn())})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
