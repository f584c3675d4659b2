"""factorise_multistart timing on the box.

per-iteration (default): µs of one multistart iteration of all R starts (one cnmf_ms_step launch per
    batch) against R back-to-back cnmf_hals_step launches on R separate states over the same X — the
    loop the function replaces — alternated in the same process, at each `--shapes` entry
    (rows,features,k,starts; fp32).  tol = 0, so no launch is a no-op.
--fit: on rows x 81, k = 4, seeds 0..7, tol = 1e-4, max_iter = 200: the eight final errors, and the
    wall and device time of one factorise_multistart call against eight factorise(solver='hals')
    calls from the same seeds (X already on the device for both).

HIP events around back-to-back launches after warm-up; every per-iteration figure is the median of
`--repeats` windows with the spread (min..max) next to it.  One process, one GPU.  Prints one JSON
line.  With the diagnostic library (CNMF_HIP_LIB=.../libcnmf_hip_diag.so) CNMF_MS_TEAMS=1|2|4 sets
the teams per workgroup, and with them the starts a launch takes.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_ms(fn, reps, stream):
    """ms of `reps` back-to-back calls of fn (events on `stream`)."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(samples):
    return {"median_us": round(statistics.median(samples), 2), "min_us": round(min(samples), 2),
            "max_us": round(max(samples), 2)}


def per_iteration(a, out):
    import torch
    from cnmf_amd.multistart import MS_STOPPED, MultiStartPlan
    from cnmf_amd.solver import HALSPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    for shape in a.shapes:
        n, F, k, R = (int(v) for v in shape.split(","))
        X = iop_spectra(n, F, seed=0, dtype=np.float32)
        Xd = torch.from_numpy(X).to(dev)
        ms = MultiStartPlan(Xd, k, R, max_batch=a.max_batch)
        singles = [HALSPlan(Xd, k) for _ in range(R)]
        for r, p in enumerate(singles):
            W0, H0 = random_init(X, k, r)
            p.set_W(torch.from_numpy(W0))
            p.set_H(torch.from_numpy(H0))
            p.ctl = p.new_ctl(tol=0.0)  # never stops: every launch does the work
            ms.set_start(r, W0, H0)
        ms.ctl = ms.new_ctl(tol=0.0)

        def batched():
            for b in range(len(ms.batches)):
                ms.step(b)

        def sequential():
            for p in singles:
                p.step()
        for _ in range(a.warm):
            batched()
            sequential()
        torch.cuda.synchronize()
        t_b, t_s = [], []
        for _ in range(a.repeats):
            t_b.append(window_ms(batched, a.reps, stream) / a.reps * 1e3)
            t_s.append(window_ms(sequential, a.reps, stream) / a.reps * 1e3)
        assert not ms.read_ctl()[:, MS_STOPPED].any() and all(p.read_ctl()[0] == 0.0 for p in singles), \
            "the timed launches were no-ops"
        same = all(torch.equal(ms.W_of(r), p.W) and torch.equal(ms.H64[r], p.H64) for r, p in enumerate(singles))
        out[f"per_iteration_{n}x{F}_k{k}_R{R}"] = {
            "multistart": summary(t_b), "sequential_hals_steps": summary(t_s),
            "ratio_multistart_over_sequential": round(statistics.median(t_b) / statistics.median(t_s), 3),
            "starts_per_launch": ms.RB, "batches": [cnt for _, cnt in ms.batches], "same_bits_as_sequential": same,
            "teams_env": os.environ.get("CNMF_MS_TEAMS")}
        del ms, singles, Xd


def fit(a, out):
    import torch
    from cnmf_amd import factorise, factorise_multistart
    from cnmf_amd.synthetic import iop_spectra
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    n, F, k, seeds = a.rows, 81, 4, list(range(8))
    Xd = torch.from_numpy(iop_spectra(n, F, seed=0, dtype=np.float32)).to(dev)
    kw = dict(tol=1e-4, max_iter=200)

    def multi():
        return factorise_multistart(Xd, k, n_init=len(seeds), random_state=seeds, **kw)

    def loop():
        return [factorise(Xd, n_components=k, init="random", random_state=s, solver="hals", **kw) for s in seeds]

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        res = fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runs = {"multistart": [], "loop": []}
        for _ in range(1 + a.fit_repeats):  # the first pair warms the clocks
            res, wall, devt = timed(multi)
            runs["multistart"].append((wall, devt))
            singles, wall, devt = timed(loop)
            runs["loop"].append((wall, devt))
    out["fit"] = {
        "rows": n, "seeds": seeds, "errors": [float(e) for e in res.errors], "n_iters": res.n_iters.tolist(),
        "best": res.best, "loop_n_iters": [int(s[2]) for s in singles],
        "multistart_wall_ms": [round(w, 1) for w, _ in runs["multistart"][1:]],
        "multistart_device_ms": [round(d, 1) for _, d in runs["multistart"][1:]],
        "loop_wall_ms": [round(w, 1) for w, _ in runs["loop"][1:]],
        "loop_device_ms": [round(d, 1) for _, d in runs["loop"][1:]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000000,81,4,8", "1000000,81,8,4", "200000,300,16,4"])
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--max-batch", type=int, default=None)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit-repeats", type=int, default=2)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"warm": a.warm, "reps": a.reps, "repeats": a.repeats}
    if a.fit:
        fit(a, out)
    else:
        per_iteration(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
