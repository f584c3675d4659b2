"""Minibatch step timing on the box: µs per cnmf_mb_step launch at several batch
sizes, one full-batch step against the non-persistent sequence it replaces (cnmf_mu_sample_pass +
cnmf_reduce_update over the same rows, alternated in the same process), and the epochs / device time
the online fit needs to reach the error of 200 full-batch MU iterations.

HIP events around back-to-back launches after >= 20 warm steps; every figure is the median of
`--repeats` windows, with the spread (min..max) next to it.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_us(fn, reps, stream):
    """µs per call of fn over `reps` back-to-back calls (events on `stream`)."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def summary(samples):
    return {"median_us": round(statistics.median(samples), 2), "min_us": round(min(samples), 2),
            "max_us": round(max(samples), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=81)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[1024, 65536, 1_000_000])
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit-batch", type=int, default=65536, help="batch size of the time-to-error fit")
    ap.add_argument("--max-epochs", type=int, default=60)
    a = ap.parse_args()

    import torch
    from cnmf_amd import _lib
    from cnmf_amd.minibatch import MiniBatchPlan, _gen_batches
    from cnmf_amd.solver import MUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    assert torch.cuda.is_available(), "needs a HIP device"
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, F, k = a.rows, a.features, a.k
    X = iop_spectra(n, F, seed=0, dtype=np.float32)
    W0, H0 = random_init(X, k, 42)
    Xd = torch.from_numpy(X).to(dev)
    W0d = torch.from_numpy(W0).to(dev)
    stream = torch.cuda.current_stream(dev)
    out = {"shape": [n, F, k, "f32"], "warm": a.warm, "reps": a.reps, "repeats": a.repeats}

    def mb_plan(bs):
        plan = MiniBatchPlan(H0, torch.float32, dev, rho=0.7 ** (min(bs, n) / n), n_samples=n)
        plan.attach(Xd, W0d.clone())
        return plan, _gen_batches(n, min(bs, n))

    # ---- µs per step
    for bs in a.batch_sizes:
        plan, batches = mb_plan(bs)
        full = [b for b in batches if b[1] - b[0] == min(bs, n)]  # time whole batches only
        state = {"i": 0}

        def step():
            lo, hi = full[state["i"] % len(full)]
            state["i"] += 1
            plan.step(lo, hi)
        for _ in range(a.warm):
            step()
        torch.cuda.synchronize()
        out[f"step_bs{bs}"] = summary([window_us(step, a.reps, stream) for _ in range(a.repeats)])
        out[f"step_bs{bs}"]["partial_rows"] = int(lib.cnmf_mb_rows(min(bs, n)))

    # ---- one full-batch step against pass + reduce_update over the same rows, alternated
    plan, _ = mb_plan(n)
    mu = MUPlan(Xd, k)
    mu.set_W(W0d)
    mu.set_H(torch.from_numpy(H0))
    s = stream.cuda_stream

    def sequence():
        mu.sample_pass(_lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE)
        _lib.check(lib.cnmf_reduce_update(mu.partials.data_ptr(), mu.n_parts, mu.stage.data_ptr(),
                                          mu.counter.data_ptr(), mu.AB.data_ptr(), mu.H64.data_ptr(),
                                          mu.Ht.data_ptr(), mu.HHt.data_ptr(), F, k, 0.0, 0.0, mu.stats.data_ptr(), s))

    def one_step():
        plan.step(0, n)
    for _ in range(a.warm):
        one_step()
        sequence()
    torch.cuda.synchronize()
    t_step, t_seq = [], []
    for _ in range(a.repeats):
        t_step.append(window_us(one_step, a.reps, stream))
        t_seq.append(window_us(sequence, a.reps, stream))
    out["full_batch_step"] = summary(t_step)
    out["pass_plus_reduce_update"] = summary(t_seq)
    out["ratio_step_over_sequence"] = round(statistics.median(t_step) / statistics.median(t_seq), 3)
    bytes_moved = n * (F * 4 + 2 * k * 4)
    out["full_batch_step_GBs"] = round(bytes_moved / statistics.median(t_step) / 1e3, 1)

    # ---- time to the error of 200 full-batch MU iterations
    mu.set_W(W0d)
    mu.set_H(torch.from_numpy(H0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mu.iterate(200)
    torch.cuda.synchronize()
    out["full_batch_200_iter_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    target = mu.frobenius_error()
    out["full_batch_200_iter_error"] = target
    plan, batches = mb_plan(a.fit_batch)
    device_ms, wall_ms, errors, reached = 0.0, 0.0, [], None
    for epoch in range(1, a.max_epochs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        for lo, hi in batches:
            plan.step(lo, hi)
        e1.record(stream)
        torch.cuda.synchronize()
        wall_ms += (time.perf_counter() - t0) * 1e3
        device_ms += e0.elapsed_time(e1)
        errors.append(plan.frobenius_error())  # not timed: the fit itself never evaluates it
        if errors[-1] <= target:
            reached = epoch
            break
    out["minibatch_fit"] = {"batch_size": a.fit_batch, "steps_per_epoch": len(batches), "epochs_to_target": reached,
                            "epochs_run": len(errors), "device_ms": round(device_ms, 2),
                            "wall_ms": round(wall_ms, 2), "error_after_1_epoch": errors[0],
                            "last_error": errors[-1], "best_error": min(errors)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
