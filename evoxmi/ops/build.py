"""In-tree build of the evoxmi HIP extension (``evoxmi/_C.so``) for gfx950.

``python -m evoxmi.ops.build`` compiles

* every ``csrc/kernels/*.hip`` with ``hipcc --offload-arch=gfx950`` (device code,
  no torch headers — seconds per file), and
* ``csrc/bindings/*.cpp`` (the TORCH_LIBRARY registration) with the host compiler,

then links one shared object next to the package so it travels with the repo
snapshot to the GPU box.  Builds are incremental (mtime-based, headers included)
and parallel.  No hipify, no CUDA sources: the kernels are written for CDNA4.
"""
from __future__ import annotations

import glob
import os
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "csrc")
PKG = os.path.join(ROOT, "evoxmi")
BUILD = os.path.join(ROOT, "build", "evoxmi_ext")
OUT = os.path.join(PKG, "_C.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("EVOXMI_ARCH", "gfx950")


def _torch_dir():
    import torch

    return os.path.dirname(torch.__file__)


def _headers():
    hs = glob.glob(os.path.join(CSRC, "include", "*.h")) + glob.glob(os.path.join(CSRC, "host", "*.h"))
    return max((os.path.getmtime(h) for h in hs), default=0.0)


def _stale(src, obj, hdr_mtime, cmd=None):
    """Rebuild when the object is missing or older than its source / the headers, or when its
    compile command changed (a per-file flag edit must not leave an object built the old way)."""
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    if os.path.getmtime(src) > t or hdr_mtime > t:
        return True
    if cmd is not None:
        stamp = obj + ".cmd"
        try:
            with open(stamp) as f:
                return f.read() != " ".join(cmd)
        except OSError:
            return True
    return False


def _stamp(cmd):
    """Record the command line of a compiled object next to it (read by _stale)."""
    obj = cmd[cmd.index("-o") + 1]
    with open(obj + ".cmd", "w") as f:
        f.write(" ".join(cmd))


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed:\n" + " ".join(cmd) + "\n" + r.stdout)
    return r.stdout


# per-file device flags
# eigh_sbr.hip: kept so the Taylor operand pass (sbr_taylor_prep_kernel, on the hot path) compiles as it
# did; whether SLP packing helps or hurts that kernel has not been measured
# mo_geom.hip: its distance loop must stay unfused (bit-identical ties with the CPU
# oracle); plain "fast" contraction ignores the in-source pragma
# neuro.hip: the Ant sub-step is packed f32 by hand (v_pk_* with op_sel / neg swizzles); SLP packing
# of what is left scalar lengthens it from 642 to 734 instructions and makes the register-resident
# rollout spill (250 VGPRs and no scratch → 256 and 244 bytes of scratch per lane)
# gemm_ks.hip: the bf16x6 split's residual subtractions must stay scalar (v_pk_add_f32 issued
# beside MFMAs costs ≈13 cycles more than two v_sub_f32)
# knea_select.hip: its contract is float64 arithmetic in a stated operation order with no FMA, so a
# host implementation of the same operations reproduces its keys and box tests bit for bit
# rvea_select.hip: the same kind of contract: its cosines are symmetric bit for bit and a host implementation reproduces them
# bige_select.hip, tdea_select.hip: the same kind of contract: a host implementation reproduces BiGE's proximity and θ-DEA's
# penalised distance bit for bit
# hv_exact.hip: its accuracy contract counts one rounding per float64 operation of the stated formulas, so none may fuse
# planar_rollout.hip: its sub-step is scalar f32 arithmetic; SLP packing adds ~190 v_mov per
# sub-step (835 instructions against 704 without it in the two-chain instantiation)
FILE_FLAGS = {"eigh_sbr.hip": ["-fno-slp-vectorize"], "mo_geom.hip": ["-ffp-contract=fast-honor-pragmas"],
              "knea_select.hip": ["-ffp-contract=off"], "rvea_select.hip": ["-ffp-contract=off"],
              "bige_select.hip": ["-ffp-contract=off"], "tdea_select.hip": ["-ffp-contract=off"],
              "hv_exact.hip": ["-ffp-contract=off"], "rng.hip": ["-ffp-contract=fast-honor-pragmas"],
              "neuro.hip": ["-fno-slp-vectorize"], "planar_rollout.hip": ["-fno-slp-vectorize"], "gemm_ks.hip": ["-fno-slp-vectorize"]}


def build(verbose: bool = True, jobs: int = None) -> str:
    os.makedirs(BUILD, exist_ok=True)
    td = _torch_dir()
    hdr = _headers()
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    inc = ["-I" + os.path.join(CSRC, "include")]
    dev_flags = [
        f"--offload-arch={ARCH}",
        "-O3",
        "-fPIC",
        "-std=c++17",
        "-ffp-contract=fast",
        "-munsafe-fp-atomics",
    ] + inc
    host_flags = [
        "-O2",
        "-fPIC",
        "-std=c++17",
        "-D__HIP_PLATFORM_AMD__",
        "-DUSE_ROCM",
        "-D_GLIBCXX_USE_CXX11_ABI=1",
        "-I" + os.path.join(td, "include"),
        "-I" + os.path.join(td, "include", "torch", "csrc", "api", "include"),
        "-I" + os.path.join(ROCM, "include"),
        "-I" + sysconfig.get_paths()["include"],
    ] + inc
    jobs = jobs or min(8, os.cpu_count() or 4)
    tasks = []
    objs = []
    for src in sorted(glob.glob(os.path.join(CSRC, "kernels", "*.hip"))):
        obj = os.path.join(BUILD, os.path.basename(src) + ".o")
        objs.append(obj)
        cmd = [hipcc] + dev_flags + FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if _stale(src, obj, hdr, cmd):
            tasks.append(cmd)
    for src in sorted(glob.glob(os.path.join(CSRC, "bindings", "*.cpp"))):
        obj = os.path.join(BUILD, os.path.basename(src) + ".o")
        objs.append(obj)
        cmd = ["g++"] + host_flags + ["-c", src, "-o", obj]
        if _stale(src, obj, hdr, cmd):
            tasks.append(cmd)
    if verbose and tasks:
        print(f"[evoxmi.build] compiling {len(tasks)} translation unit(s) for {ARCH}", flush=True)
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(_run, tasks))
    for cmd in tasks:
        _stamp(cmd)
    need_link = tasks or not os.path.exists(OUT) or any(os.path.getmtime(o) > os.path.getmtime(OUT) for o in objs)
    if need_link:
        tl = os.path.join(td, "lib")
        link = (
            [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT]
            + objs
            + [
                "-L" + tl,
                "-Wl,-rpath," + tl,
                "-lc10",
                "-lc10_hip",
                "-ltorch",
                "-ltorch_cpu",
                "-ltorch_hip",
                "-L" + os.path.join(ROCM, "lib"),
                "-lamdhip64",
                "-fopenmp",
            ]
        )
        _run(link)
        if verbose:
            print(f"[evoxmi.build] linked {OUT}", flush=True)
    return OUT


if __name__ == "__main__":
    build(verbose=True)
    sys.exit(0)
