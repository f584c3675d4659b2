"""init='spa' timing and value on the box.

per-launch (default): µs per cnmf_spa_step launch at steps j = 0, 3, 7, 15 (those below k) and per
    cnmf_spa_start_w launch, against cnmf_mu_sample_pass over the same rows, alternated in the same
    process, at each `--shapes` entry (rows,features,k; fp32).  Every timed launch has its own event
    pair (step k-1 sets the control block's STOPPED word, which is cleared outside the timed
    region); a figure is the median over `--repeats` windows of the median of `--reps` launches.
--whole-start: wall time of spa_init against _initial_factors(init='nndsvda') at rows x 81, k = 4,
    for float32 X (the host start) and float64 X (the GPU start).
--value: ‖X − WH‖ at rows x 81, k = 4 after 50 / 200 / 500 MU and 20 / 50 HALS iterations from the
    'spa', 'nndsvda' and random_init(X, 4, 42) starts.

One process, one GPU.  Prints one JSON line.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def launch_us(fn, stream, before=None):
    """µs of one launch of fn between its own event pair."""
    import torch
    if before is not None:
        before()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(samples):
    return {"median_us": round(statistics.median(samples), 2), "min_us": round(min(samples), 2),
            "max_us": round(max(samples), 2)}


def per_launch(a, out):
    import torch
    from cnmf_amd import _lib
    from cnmf_amd.solver import MUPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    spa_mod = importlib.import_module("cnmf_amd.spa")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev)
    for shape in a.shapes:
        n, F, k = (int(v) for v in shape.split(","))
        X = iop_spectra(n, F, seed=0, dtype=np.float32)
        Xd = torch.from_numpy(X).to(dev)
        st = spa_mod.SPAState(Xd, k)
        idx, info = st.run()
        steps = info["steps"]  # below k when the rank of X ran out: only those steps are timed
        M = torch.from_numpy(np.linalg.pinv(X[idx].astype(np.float64), rcond=1e-6)).to(dev)
        mu = MUPlan(Xd, k)
        W0, H0 = random_init(X, k, 42)
        mu.set_W(torch.from_numpy(W0))
        mu.set_H(torch.from_numpy(H0))

        def clear():
            st.ctl[spa_mod.SPA_STOPPED] = 0.0

        def mu_pass():
            mu.sample_pass(_lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE)

        fns = {f"spa_step_j{j}": (lambda j=j: st.step(j)) for j in (0, 3, 7, 15) if j < steps}
        fns["spa_start_w"] = lambda: spa_mod.start_w(Xd, M, info["mean"] / 100)
        fns["mu_sample_pass"] = mu_pass
        for _ in range(a.warm):
            for fn in fns.values():
                clear()
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, fn in fns.items():  # alternated: every window visits every launch
                times[name].append(statistics.median(launch_us(fn, stream, clear) for _ in range(a.reps)))
        base = statistics.median(times["mu_sample_pass"])
        r = {name: dict(summary(t), ratio_to_mu_pass=round(statistics.median(t) / base, 3)) for name, t in times.items()}
        r["x_GBs_at_step_j0"] = round(n * F * 4 / statistics.median(times["spa_step_j0"]) / 1e3, 1)
        r["steps"] = steps
        r["partial_rows"] = int(st.rows)
        r["mu_kernel"] = mu.describe()[:60]
        out[f"per_launch_{n}x{F}_k{k}"] = r
        del st, mu, Xd, M


def whole_start(a, out):
    import torch
    import cnmf_amd
    from cnmf_amd import api
    from cnmf_amd.synthetic import iop_spectra
    for dtype in (np.float32, np.float64):
        X = iop_spectra(a.rows, 81, seed=0, dtype=dtype)
        r = {}
        for name, fn in (("spa_init", lambda: cnmf_amd.spa_init(X, 4)),
                         ("nndsvda", lambda: api._initial_factors(X, 4, "nndsvda", None, None, False, None))):
            ts = []
            for _ in range(1 + a.repeats):  # the first run warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            r[name + "_ms"] = round(statistics.median(ts[1:]), 2)
            r[name + "_ms_runs"] = [round(t, 2) for t in ts[1:]]
        out[f"whole_start_{a.rows}x81_k4_{np.dtype(dtype).name}"] = r


def value(a, out):
    import cnmf_amd
    from cnmf_amd import api
    from cnmf_amd.synthetic import iop_spectra, random_init
    X = iop_spectra(a.rows, 81, seed=0, dtype=np.float32)
    starts = {"spa": tuple(t.cpu().numpy() for t in cnmf_amd.spa_init(X, 4)),
              "nndsvda": api._initial_factors(X, 4, "nndsvda", None, None, False, None, init_device="host"),
              "random": random_init(X, 4, 42)}
    r = {}
    for name, (W0, H0) in starts.items():
        W0, H0 = np.ascontiguousarray(W0, dtype=np.float32), np.ascontiguousarray(H0, dtype=np.float32)
        for solver, iters in (("mu", (50, 200, 500)), ("hals", (20, 50))):
            for it in iters:
                W, H, _ = cnmf_amd.factorise(X, W0, H0, init="custom", n_components=4, solver=solver, tol=0, max_iter=it)
                err = 0.0
                for lo in range(0, a.rows, 1 << 17):
                    d = X[lo:lo + (1 << 17)].astype(np.float64) - W[lo:lo + (1 << 17)].astype(np.float64) @ H.astype(np.float64)
                    err += float((d * d).sum())
                r[f"{name}_{solver}_{it}"] = round(err ** 0.5, 4)
    out[f"value_{a.rows}x81_k4"] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000000,81,4", "1000000,81,16", "200000,300,16"])
    ap.add_argument("--whole-start", action="store_true")
    ap.add_argument("--value", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    out = {"warm": a.warm, "reps": a.reps, "repeats": a.repeats}
    if a.whole_start:
        whole_start(a, out)
    elif a.value:
        value(a, out)
    else:
        per_launch(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
