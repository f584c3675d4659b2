"""Write the init='spa' goldens: tests/golden/spa_*.npz and MANIFEST_spa.json.

    python tests/golden/make_golden_spa.py

Every case is `iop_spectra(n, F, seed, dtype)` for float32 and float64 and both row scales.  The
picks come from tests/spa_ref.py, and the generator asserts two conditions on the INPUTS before it
writes a case:
  * the picks equal the first k pivots of scipy.linalg.qr(Y.T, pivoting=True) — LAPACK's pivoted
    QR, an oracle independent of the restatement;
  * the runner-up margin (best score − second-best score) / best is at least 1e-4 at every step, so
    that a device whose fp64 scores differ from NumPy's by ~1e-13 must pick the same rows.
A float64 variant whose margin is too small takes another seed; one whose rank runs out before k
rows (spectra evaluated in float64 have numerical rank ~11) takes the float32 values widened to
float64 (both recorded in the manifest; tests call make_x of this file's recipe).  X is stored
only where it is small; otherwise the test regenerates it from the seed.
"""
import json
import os
import sys

import numpy as np
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from spa_ref import margins, row_scale, spa_ref  # noqa: E402
from cnmf_amd.synthetic import iop_spectra  # noqa: E402

CASES = [  # (n, F, k, seed)
    (333, 81, 4, 1), (337, 81, 8, 2), (200, 300, 16, 3), (150, 17, 3, 4), (32805, 83, 5, 5), (337, 512, 16, 9),
    (70, 5, 1, 7),
]
MIN_MARGIN = 1e-4
STORE_X_BYTES = 128 * 1024


def make_x(n, F, seed, dtype, widened=False):
    """The case's X; widened: the float32 spectra cast to float64 (see main)."""
    if widened:
        return iop_spectra(n, F, seed=seed, dtype=np.float32).astype(dtype)
    return iop_spectra(n, F, seed=seed, dtype=dtype)


def variant(X, k, normalise):
    idx, info = spa_ref(X, k, normalise=normalise, return_scores=True)
    m = margins(info["scores"])
    piv = scipy.linalg.qr(row_scale(X, normalise).T, mode="r", pivoting=True)[1][:k]
    ok = len(idx) == k and np.array_equal(piv, idx) and min(m) >= MIN_MARGIN
    return ok, idx, info, m


def main():
    manifest = {}
    for n, F, k, seed0 in CASES:
        for dtype in (np.float32, np.float64):
            seed, widened = seed0, False
            for attempt in range(8):
                X = make_x(n, F, seed, dtype, widened)
                res = {nm: variant(X, k, nm) for nm in ("l1", None)}
                if all(r[0] for r in res.values()):
                    break
                assert dtype == np.float64, f"the float32 case {(n, F, k, seed)} misses its conditions"
                if any(len(r[1]) < k for r in res.values()):
                    # spectra evaluated in float64 have numerical rank ~11 (the smooth exponentials);
                    # it is float32 rounding that gives the k = 16 cases their rank: widen those values
                    widened = True
                else:
                    seed += 100
            else:
                raise AssertionError(f"no float64 variant of {(n, F, k, seed0)} meets the conditions")
            name = f"spa_{n}x{F}_k{k}_{np.dtype(dtype).name}"
            out = dict(n=n, F=F, k=k, seed=seed, widened=widened)
            entry = dict(n=n, F=F, k=k, seed=seed, dtype=np.dtype(dtype).name, widened=widened,
                         stores_X=X.nbytes <= STORE_X_BYTES)
            if entry["stores_X"]:
                out["X"] = X
            for nm, (_, idx, info, m) in res.items():
                tag = "l1" if nm == "l1" else "none"
                out.update({f"idx_{tag}": idx, f"Q_{tag}": info["Q"], f"rho_{tag}": info["rho"],
                            f"margins_{tag}": np.asarray(m), f"ymax_{tag}": info["ymax"], f"mean_{tag}": info["mean"]})
                entry[tag] = dict(idx=[int(i) for i in idx], min_margin=min(m), rho_last=float(info["rho"][-1]))
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) < (1 << 20), path
            manifest[name] = entry
            print(name, "seed", seed, {t: (entry[t]["min_margin"], entry[t]["rho_last"]) for t in ("l1", "none")})
    with open(os.path.join(HERE, "MANIFEST_spa.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
