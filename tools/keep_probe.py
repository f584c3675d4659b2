"""Diagnostic: µs per MU iteration of the persistent wave-tile launch against the share of X kept in
the Infinity Cache (CNMF_WT_KEEP16 = sixteenths of X loaded with the default cache policy, the rest
`nt`; read by the DIAGNOSTIC library at every launch — csrc/keep.hpp holds the product's rule).

    python tools/keep_probe.py [--keeps 0,4,6,8,9,10,11,12,13,16] [--shapes 750000:4,1000000:4,...]
                               [--iters 500] [--warm 1500] [--passes 2] [--out LOG]

One run = one shape in one pass: its own process (this file with --child) on
cnmf_amd/libcnmf_hip_diag.so under its own time limit; the runs follow one another and the first that
fails ends the sweep.  A run warms up (--warm iterations), then for every share settles the cache
with 100 iterations and times one launch of --iters.  The second pass walks the shapes and the shares
in the opposite order.  Prints one JSON line per run and a table of the per-share minimum and both
passes at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEPS = "0,4,6,8,9,10,11,12,13,16"
SHAPES = "750000:4,1000000:4,1500000:4,2000000:4,1250000:8"


def child(args):
    import numpy as np
    import torch
    from cnmf_amd.solver import MUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init

    X = iop_spectra(args.rows, 81, seed=0, dtype=np.float32)
    W0, H0 = random_init(X, args.k, 42)
    plan = MUPlan(torch.from_numpy(X).cuda(), args.k)
    plan.set_W(torch.from_numpy(W0))
    plan.set_H(torch.from_numpy(H0).cuda())
    os.environ["CNMF_WT_KEEP16"] = "0"
    desc = plan.describe()
    assert "mu_iter_wt_kernel" in desc, desc
    plan.iterate(args.warm)  # clocks up
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    res = {}
    for keep in [int(v) for v in args.keeps.split(",")]:
        os.environ["CNMF_WT_KEEP16"] = str(keep)
        plan.iterate(100)  # the resident set of this share in place
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        plan.iterate(args.iters)
        e1.record(st)
        torch.cuda.synchronize()
        plan.check_sync_error()
        res[keep] = round(e0.elapsed_time(e1) * 1e3 / args.iters, 2)
    H = plan.H64.cpu().numpy()
    print(json.dumps({"rows": args.rows, "k": args.k, "x_mb": round(args.rows * 81 * 4 / 1e6, 1),
                      "us_per_iteration": res, "H_finite": bool(np.isfinite(H).all()), "kernel": desc.split(":")[0]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keeps", default=KEEPS)
    ap.add_argument("--shapes", default=SHAPES, help="rows:k, comma separated")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warm", type=int, default=1500)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=4)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lib = os.environ.get("CNMF_HIP_LIB", os.path.join(ROOT, "cnmf_amd", "libcnmf_hip_diag.so"))
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    keeps = args.keeps.split(",")
    lines, runs = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# keep_probe: lib {os.path.basename(lib)}, {args.iters}-iteration launches after {args.warm} warm-up")
    for p in range(args.passes):
        fwd = p % 2 == 0
        for rows, k in (shapes if fwd else shapes[::-1]):
            cmd = [sys.executable, "-u", os.path.abspath(__file__), "--child", "--rows", str(rows), "--k", str(k),
                   "--keeps", ",".join(keeps if fwd else keeps[::-1]), "--iters", str(args.iters),
                   "--warm", str(args.warm)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit,
                                   env=dict(os.environ, CNMF_HIP_LIB=lib))
            except subprocess.TimeoutExpired:
                say(f"# pass {p} {rows}x81 k{k}: over its {args.limit} s limit; the sweep ends here")
                return finish(lines, runs, args.out, 1)
            if r.returncode != 0:
                say(f"# pass {p} {rows}x81 k{k}: exit {r.returncode}; the sweep ends here\n{r.stderr[-2000:]}")
                return finish(lines, runs, args.out, 1)
            out = json.loads(r.stdout.strip().splitlines()[-1])
            out["pass"] = p
            runs.append(out)
            say(json.dumps(out))
    return finish(lines, runs, args.out, 0)


def finish(lines, runs, out, status):
    shapes = []
    for r in runs:
        if (r["rows"], r["k"]) not in shapes:
            shapes.append((r["rows"], r["k"]))
    table = []
    for rows, k in shapes:
        mine = [r for r in runs if (r["rows"], r["k"]) == (rows, k)]
        table.append(f"\n{rows} x 81, k = {k} ({mine[0]['x_mb']} MB of X): share/16, resident MB, "
                     f"us per iteration (min; each pass)")
        for keep in sorted(mine[0]["us_per_iteration"], key=int):
            v = [r["us_per_iteration"][keep] for r in mine if keep in r["us_per_iteration"]]
            table.append(f"  {int(keep):2d}  {mine[0]['x_mb'] * int(keep) / 16:6.1f}  {min(v):8.2f}   "
                         + "  ".join(f"{x:8.2f}" for x in v))
    print("\n".join(table), flush=True)
    text = "\n".join(lines + table) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main() or 0)
