"""Build libcnmf_hip.so in-tree with hipcc for gfx950 (no JIT cache, no torch extension machinery).

    python -m cnmf_amd.build [--verbose] [--force] [--diag | --stamps | --all]

The product and diagnostic libraries are compiled one object per source file of csrc/ (each family
file, and cnmf_hip.hip with -DCNMF_SEPARATE: the families still in it) under build/obj/<variant>/ and
linked with one `hipcc -shared`; no -fgpu-rdc, so every kernel is compiled as in a single translation
unit.  An object is recompiled when its source, a csrc/*.hpp, include/cnmf_hip.h or its command line
changed; a library is relinked when an object is newer than it.  The stamps variant is one compile
of cnmf_hip.hip as the aggregate (without -DCNMF_SEPARATE it #includes every family file): its
__device__ counters are shared by kernels of several families, and without relocatable device code
a device variable is private to its code object.
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "cnmf_hip.hip")  # the aggregate, or with -DCNMF_SEPARATE the families still in it
OUT = os.path.join(HERE, "libcnmf_hip.so")
OBJ = os.path.join(ROOT, "build", "obj")
ARCH = os.environ.get("CNMF_OFFLOAD_ARCH", "gfx950")


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def jobs() -> int:
    """Concurrent compiles, across variants: at most 16 (and MAX_JOBS), whatever the machine shows."""
    n = min(16, os.cpu_count() or 1)
    try:
        n = min(n, int(os.environ["MAX_JOBS"]))
    except (KeyError, ValueError):
        pass
    return max(1, n)


def sources() -> list[str]:
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _headers() -> list[str]:
    return sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(ROOT, "include", "cnmf_hip.h")]


def _variant(stamps: bool, diag: bool) -> str:
    return "stamps" if stamps else ("diag" if diag else "product")


def _variant_out(stamps: bool, diag: bool) -> str:
    return OUT.replace(".so", "_stamps.so") if stamps else (OUT.replace(".so", "_diag.so") if diag else OUT)


def _flags(stamps: bool, diag: bool) -> list[str]:
    defs = (["-DCNMF_STAMPS"] if stamps else []) + (["-DCNMF_DIAG"] if stamps or diag else [])
    return [hipcc()] + defs + ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-I", os.path.join(ROOT, "include")]


def _newer(path: str, deps) -> bool:
    """`path` is missing or older than one of `deps`."""
    if not os.path.exists(path):
        return True
    m = os.path.getmtime(path)
    return any(os.path.getmtime(d) > m for d in deps)


class Plan(NamedTuple):
    """What brings one variant up to date."""
    variant: str
    out: str          # the library
    product: bool     # kcheck'ed before it is installed
    compiles: list    # hipcc command lines
    link: list | None
    stamp: str        # file that records the variant's command line
    flags: str


def needs_build(stamps: bool = False, diag: bool = False) -> bool:
    p = _plan(stamps, diag, force=False)
    return bool(p.compiles) or p.link is not None


def _read(path: str) -> str:
    if not os.path.exists(path):
        return ""
    with open(path) as f:
        return f.read()


def _plan(stamps: bool, diag: bool, force: bool) -> Plan:
    """The compile and link commands that bring this variant up to date (nothing is written)."""
    variant, out, flags = _variant(stamps, diag), _variant_out(stamps, diag), _flags(stamps, diag)
    odir = os.path.join(OBJ, variant)
    stamp = os.path.join(odir, "flags.txt")  # the command line of the variant's objects / library
    changed = force or _read(stamp) != " ".join(flags)
    if stamps:  # one compile of the aggregate
        stale = changed or _newer(out, sources() + _headers())
        return Plan(variant, out, False, [flags + ["-shared", "-o", out + ".tmp", SRC]] if stale else [], None,
                    stamp, " ".join(flags))
    objs, compiles = [], []
    for src in sources():
        obj = os.path.join(odir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if changed or _newer(obj, [src] + _headers()):
            compiles.append(flags + ["-DCNMF_SEPARATE", "-c", src, "-o", obj])
    link = None
    if compiles or _newer(out, objs):
        link = [hipcc(), "-shared", "-fPIC", "-o", out + ".tmp"] + objs
    return Plan(variant, out, not diag, compiles, link, stamp, " ".join(flags))


def _check(tmp: str) -> None:
    # the shipped wave-tile kernels' prefetch registers must never be spilled (tools/kcheck.py)
    env = dict(os.environ, HIPCC=hipcc(), CNMF_OFFLOAD_ARCH=ARCH)
    chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kcheck.py"), tmp, "--arch", ARCH],
                         capture_output=True, text=True, env=env)
    if chk.returncode == 2:  # the check could not run (tools / arch): not a finding
        raise RuntimeError("kernel check could not run on the built library:\n" + chk.stderr[-3000:])
    if chk.returncode != 0:
        raise RuntimeError("kernel check failed (prefetch registers touched outside their loads):\n"
                           + chk.stdout[-3000:] + chk.stderr[-2000:])


def build_many(variants, verbose: bool = False, force: bool = False) -> list[str]:
    """Bring several variants ((stamps, diag) pairs) up to date: their stale objects compiled as
    concurrent hipcc processes (jobs() at a time over all variants), then the variants linked; the
    product library is kcheck'ed before it is installed.  Returns the library paths."""
    plans = [_plan(s, d, force) for s, d in variants]
    for p in plans:
        os.makedirs(os.path.dirname(p.stamp), exist_ok=True)
    # the largest sources first: the longest compile bounds the wall time
    compiles = sorted((c for p in plans for c in p.compiles),
                      key=lambda c: -os.path.getsize(next(a for a in c if a.endswith(".hip"))))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        return subprocess.run(cmd).returncode

    def finish(p: Plan):  # link, check and install one variant
        with open(p.stamp, "w") as f:
            f.write(p.flags)
        if p.link and run(p.link) != 0:
            raise RuntimeError(f"linking {p.out} failed")
        if os.path.exists(p.out + ".tmp"):
            if p.product:
                _check(p.out + ".tmp")
            os.replace(p.out + ".tmp", p.out)

    try:
        with ThreadPoolExecutor(max_workers=jobs()) as pool:
            bad = [c for c, rc in zip(compiles, pool.map(run, compiles)) if rc != 0]
            if bad:
                raise RuntimeError("hipcc failed for " + ", ".join(next(a for a in c if a.endswith(".hip")) for c in bad))
            list(pool.map(finish, plans))
    finally:  # one variant's failure leaves no temporary output of another's
        for p in plans:
            if os.path.exists(p.out + ".tmp"):
                os.remove(p.out + ".tmp")
    return [p.out for p in plans]


def build(verbose: bool = False, force: bool = False, stamps: bool = False, diag: bool = False) -> str:
    """Compile libcnmf_hip.so.  Diagnostic builds, never loaded by the product (select one with
    CNMF_HIP_LIB=<path> in tools/ runs): stamps=True -> libcnmf_hip_stamps.so (in-kernel s_memtime /
    s_memrealtime stamps: per-phase sums, persistent-launch timelines; implies diag); diag=True ->
    libcnmf_hip_diag.so (the A/B environment switches CNMF_*, cnmf_hbm_probe and the layouts kept out
    of the product: 1-3 and the k = 8 matrix-core tiles, tests/test_gpu_mf8.py)."""
    return build_many([(stamps, diag)], verbose=verbose, force=force)[0]


if __name__ == "__main__":
    v, f = "--verbose" in sys.argv, "--force" in sys.argv
    if "--all" in sys.argv:  # product + diagnostic + stamps
        print(build_many([(False, False), (False, True), (True, True)], verbose=v, force=f))
    else:
        print(build(verbose=v, force=f, stamps="--stamps" in sys.argv, diag="--diag" in sys.argv))
