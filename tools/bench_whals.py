"""solver='whals' timing on the box, with the method of tools/bench_hals.py.

per-iteration (default): µs per cnmf_whals_step launch against cnmf_hals_step on the same X (what the
    weights cost) and against one weighted-MU iteration (cnmf_wmu_iterations, the persistent launch of
    `--reps` iterations, divided by their number), alternated in the same process, at rows x features,
    k (fp32) with a share `--zeros` of the weights zero and the rest in [0.25, 4].
--time-to-error: from the same random_init start, the weighted error and device time of `--mu-iters`
    iterations of the weighted MU, then the iterations and the device time solver='whals' needs to
    get below that error.

--only-whals: nothing but `--warm` + `--reps` cnmf_whals_step launches, for one counter pass:
    rocprofv3 --pmc <counters> -d <dir> -o run --output-format csv -- python tools/bench_whals.py \
        --only-whals --warm 2 --reps 5

HIP events around back-to-back launches after warm-up; every per-iteration figure is the median of
`--repeats` windows with the spread (min..max) next to it.  One process, one GPU.  Prints one JSON
line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_hals import summary, window_ms  # noqa: E402


def weights(shape, zeros, seed=7):
    rng = np.random.RandomState(seed)
    M = rng.uniform(0.25, 4.0, size=shape).astype(np.float32)
    M[rng.uniform(size=shape) < zeros] = 0.0
    return M


def setup(a):
    import torch
    from cnmf_amd.solver import HALSPlan, WeightedHALSPlan, WeightedMUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    dev = torch.device("cuda", torch.cuda.current_device())
    n, F, k = a.rows, a.features, a.k
    X = iop_spectra(n, F, seed=0, dtype=np.float32)
    W0, H0 = random_init(X, k, 42)
    Xd = torch.from_numpy(X).to(dev)
    Md = torch.from_numpy(weights(X.shape, a.zeros)).to(dev)
    plans = {"whals": WeightedHALSPlan(Xd, Md, k), "hals": HALSPlan(Xd, k), "wmu": WeightedMUPlan(Xd, Md, k)}

    def reset():
        for p in plans.values():
            p.set_W(torch.from_numpy(W0))
            p.set_H(torch.from_numpy(H0))
        for name in ("whals", "hals"):
            plans[name].ctl = plans[name].new_ctl(tol=0.0)  # never stops: every launch does the work
    reset()
    return plans, reset, torch.cuda.current_stream(dev)


def per_iteration(a, out):
    import torch
    plans, _, stream = setup(a)
    whals, hals, wmu = plans["whals"], plans["hals"], plans["wmu"]

    def wmu_window():
        wmu.iterate(a.reps)
    for _ in range(a.warm):
        whals.step()
        hals.step()
    wmu.iterate(a.warm)
    torch.cuda.synchronize()
    t_w, t_h, t_m = [], [], []
    for _ in range(a.repeats):
        t_w.append(window_ms(whals.step, a.reps, stream) / a.reps * 1e3)
        t_h.append(window_ms(hals.step, a.reps, stream) / a.reps * 1e3)
        t_m.append(window_ms(wmu_window, 1, stream) / a.reps * 1e3)
    wmu.check_sync_error()
    assert whals.read_ctl()[0] == 0.0 and hals.read_ctl()[0] == 0.0, "the timed launches were no-ops"
    n, F, k = a.rows, a.features, a.k
    out[f"per_iteration_{n}x{F}_k{k}"] = {
        "whals_step": summary(t_w), "hals_step": summary(t_h), "wmu_iteration": summary(t_m),
        "wmu_persistent": bool(wmu.persistent),
        "ratio_whals_over_hals": round(statistics.median(t_w) / statistics.median(t_h), 3),
        "ratio_whals_over_wmu": round(statistics.median(t_w) / statistics.median(t_m), 3),
        "whals_GBs": round(n * (2 * F * 4 + 2 * k * 4) / statistics.median(t_w) / 1e3, 1),
        "partial_rows": whals.hals_rows, "row_doubles": whals.hals_row_doubles}


def only_whals(a, out):
    """`--warm` + `--reps` cnmf_whals_step launches and nothing else timed or launched beside them:
    what a `rocprofv3 --pmc` counter pass (a run of its own, no tracing) is taken over."""
    import torch
    plans, _, stream = setup(a)
    whals = plans["whals"]
    for _ in range(a.warm):
        whals.step()
    torch.cuda.synchronize()
    ms = window_ms(whals.step, a.reps, stream)
    assert whals.read_ctl()[0] == 0.0, "the launches were no-ops"
    out["only_whals"] = {"launches": a.warm + a.reps, "us_per_step_under_the_profiler": round(ms / a.reps * 1e3, 2)}


def time_to_error(a, out):
    import torch
    plans, reset, stream = setup(a)
    whals, wmu = plans["whals"], plans["wmu"]

    def wmu_fit():
        wmu.iterate(a.mu_iters)
    times = []
    for _ in range(1 + a.repeats):  # the first run warms the clocks
        reset()
        torch.cuda.synchronize()
        times.append(window_ms(wmu_fit, 1, stream))
        wmu.check_sync_error()
    target = wmu.frobenius_error()
    out["wmu"] = {"iterations": a.mu_iters, "persistent": bool(wmu.persistent), "weighted_error": target,
                  "device_ms": round(statistics.median(times[1:]), 3), "device_ms_runs": [round(t, 3) for t in times[1:]]}

    reset()
    errors, reached = [], None
    for it in range(1, a.max_iters + 1):  # the count: the error after every iteration, not timed
        whals.step()
        errors.append(whals.frobenius_error())
        if errors[-1] <= target:
            reached = it
            break
    r = {"iterations_to_target": reached, "iterations_run": len(errors), "error_after_1": errors[0],
         "last_error": errors[-1]}
    if reached is not None:  # the device time of exactly that many back-to-back launches from the same start
        times = []
        for _ in range(1 + a.repeats):
            reset()
            torch.cuda.synchronize()
            times.append(window_ms(whals.step, reached, stream))
        r["device_ms"] = round(statistics.median(times[1:]), 3)
        r["device_ms_runs"] = [round(t, 3) for t in times[1:]]
        r["weighted_error"] = whals.frobenius_error()
        r["wmu_over_whals_device_time"] = round(out["wmu"]["device_ms"] / r["device_ms"], 2)
        for _ in range(200 - reached):  # how far 200 iterations go
            whals.step()
        r["error_after_200"] = whals.frobenius_error()
    out["whals"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=81)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--zeros", type=float, default=0.3)
    ap.add_argument("--time-to-error", action="store_true")
    ap.add_argument("--only-whals", action="store_true")
    ap.add_argument("--mu-iters", type=int, default=500)
    ap.add_argument("--max-iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"warm": a.warm, "reps": a.reps, "repeats": a.repeats, "zeros": a.zeros}
    if a.time_to_error:
        time_to_error(a, out)
    elif a.only_whals:
        only_whals(a, out)
    else:
        per_iteration(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
