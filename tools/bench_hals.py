"""solver='hals' timing on the box.

per-iteration (default): µs per cnmf_hals_step launch against the per-iteration MU sequence it stands
    beside (cnmf_mu_sample_pass + cnmf_reduce_update over the same rows), alternated in the same
    process, at each `--shapes` entry (rows,features,k; fp32).
--split: µs per iteration of the sharded form on one rank (cnmf_hals_shard_step + cnmf_hals_basis, two
    launches, no all-reduce) against the one cnmf_hals_step launch, alternated in the same process at
    each `--shapes` entry: the price of the split.
--time-to-error: on rows x 81, k = 4 from random_init, the error and device time of `--mu-iters`
    iterations of the default MU fit (the persistent wave-tile launch), then the iterations and the
    device time solver='hals' needs to reach that error.

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
    from cnmf_amd import _lib
    from cnmf_amd.solver import HALSPlan, MUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    for shape in a.shapes:
        n, F, k = (int(v) for v in shape.split(","))
        X = iop_spectra(n, F, seed=0, dtype=np.float32)
        W0, H0 = random_init(X, k, 42)
        Xd = torch.from_numpy(X).to(dev)
        hals = HALSPlan(Xd, k)
        mu = MUPlan(Xd, k)
        for p in (hals, mu):
            p.set_W(torch.from_numpy(W0))
            p.set_H(torch.from_numpy(H0))
        hals.ctl = hals.new_ctl(tol=0.0)  # never stops: every launch does the work
        s = stream.cuda_stream

        def sequence():
            mu.sample_pass(_lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE)
            _lib.check(lib.cnmf_reduce_update(mu.partials.data_ptr(), mu.n_parts, mu.stage.data_ptr(),
                                              mu.counter.data_ptr(), mu.AB.data_ptr(), mu.H64.data_ptr(),
                                              mu.Ht.data_ptr(), mu.HHt.data_ptr(), F, k, 0.0, 0.0,
                                              mu.stats.data_ptr(), s))
        for _ in range(a.warm):
            hals.step()
            sequence()
        torch.cuda.synchronize()
        t_h, t_m = [], []
        for _ in range(a.repeats):
            t_h.append(window_ms(hals.step, a.reps, stream) / a.reps * 1e3)
            t_m.append(window_ms(sequence, a.reps, stream) / a.reps * 1e3)
        assert hals.read_ctl()[0] == 0.0, "the timed launches were no-ops"
        r = {"hals_step": summary(t_h), "mu_pass_plus_reduce_update": summary(t_m),
             "ratio_hals_over_mu": round(statistics.median(t_h) / statistics.median(t_m), 3),
             "hals_GBs": round(n * (F * 4 + 2 * k * 4) / statistics.median(t_h) / 1e3, 1),
             "partial_rows": int(lib.cnmf_hals_rows(n)), "mu_kernel": mu.describe()[:60]}
        out[f"per_iteration_{n}x{F}_k{k}"] = r
        del hals, mu, Xd


def split_price(a, out):
    """The one launch against the split form (shard step + basis launch; one rank, so no all-reduce)."""
    import torch
    from cnmf_amd.solver import HALSPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    for shape in a.shapes:
        n, F, k = (int(v) for v in shape.split(","))
        X = iop_spectra(n, F, seed=0, dtype=np.float32)
        W0, H0 = random_init(X, k, 42)
        Xd = torch.from_numpy(X).to(dev)
        one, split = HALSPlan(Xd, k), HALSPlan(Xd, k, split=True)
        for p in (one, split):
            p.set_W(torch.from_numpy(W0))
            p.set_H(torch.from_numpy(H0))
            p.ctl = p.new_ctl(tol=0.0)  # never stops: every launch does the work
        for _ in range(a.warm):
            one.step()
            split.step()
        torch.cuda.synchronize()
        t_o, t_s = [], []
        for _ in range(a.repeats):
            t_o.append(window_ms(one.step, a.reps, stream) / a.reps * 1e3)
            t_s.append(window_ms(split.step, a.reps, stream) / a.reps * 1e3)
        assert one.read_ctl()[0] == 0.0 and split.read_ctl()[0] == 0.0, "the timed launches were no-ops"
        same = all(torch.equal(x, y) for x, y in ((one.W, split.W), (one.H64, split.H64), (one.ctl, split.ctl)))
        out[f"split_{n}x{F}_k{k}"] = {
            "one_launch": summary(t_o), "split": summary(t_s), "same_bits": same,
            "extra_us": round(statistics.median(t_s) - statistics.median(t_o), 2),
            "ratio_split_over_one": round(statistics.median(t_s) / statistics.median(t_o), 4)}
        del one, split, Xd


def time_to_error(a, out):
    import torch
    from cnmf_amd.solver import HALSPlan, MUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    n, F, k = a.rows, 81, 4
    X = iop_spectra(n, F, seed=0, dtype=np.float32)
    W0, H0 = random_init(X, k, 42)
    Xd = torch.from_numpy(X).to(dev)
    mu = MUPlan(Xd, k)

    def mu_fit():
        mu.iterate(a.mu_iters)
    times = []
    for _ in range(1 + a.repeats):  # the first run warms the clocks
        mu.set_W(torch.from_numpy(W0))
        mu.set_H(torch.from_numpy(H0))
        torch.cuda.synchronize()
        times.append(window_ms(mu_fit, 1, stream))
        mu.check_sync_error()
    target = mu.frobenius_error()
    out["mu"] = {"iterations": a.mu_iters, "persistent": bool(mu.persistent), "error": target,
                 "device_ms": round(statistics.median(times[1:]), 3), "device_ms_runs": [round(t, 3) for t in times[1:]]}

    hals = HALSPlan(Xd, k)
    hals.set_W(torch.from_numpy(W0))
    hals.set_H(torch.from_numpy(H0))
    hals.ctl = hals.new_ctl(tol=0.0)
    errors, reached = [], None
    for it in range(1, a.max_hals_iters + 1):  # the count: the error after every iteration, not timed
        hals.step()
        errors.append(hals.frobenius_error())
        if errors[-1] <= target:
            reached = it
            break
    r = {"iterations_to_target": reached, "iterations_run": len(errors), "error_after_1": errors[0],
         "last_error": errors[-1]}
    if reached is not None:  # the device time of exactly that many back-to-back launches from the same start
        times = []
        for _ in range(1 + a.repeats):
            hals.set_W(torch.from_numpy(W0))
            hals.set_H(torch.from_numpy(H0))
            hals.ctl = hals.new_ctl(tol=0.0)
            torch.cuda.synchronize()
            times.append(window_ms(hals.step, reached, stream))
        r["device_ms"] = round(statistics.median(times[1:]), 3)
        r["device_ms_runs"] = [round(t, 3) for t in times[1:]]
        r["error"] = hals.frobenius_error()
        r["mu_over_hals_device_time"] = round(out["mu"]["device_ms"] / r["device_ms"], 2)
        for _ in range(200 - reached):  # how far 200 iterations go
            hals.step()
        r["error_after_200"] = hals.frobenius_error()
    out["hals"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000000,81,4", "200000,300,16"])
    ap.add_argument("--time-to-error", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--mu-iters", type=int, default=500)
    ap.add_argument("--max-hals-iters", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"warm": a.warm, "reps": a.reps, "repeats": a.repeats}
    if a.time_to_error:
        time_to_error(a, out)
    elif a.split:
        split_price(a, out)
    else:
        per_iteration(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
