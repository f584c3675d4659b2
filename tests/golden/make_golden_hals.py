"""Generate the solver='hals' golden vectors (tests/golden/hals_*.npz + MANIFEST_hals.json) by running
scikit-learn 1.7.2's `non_negative_factorization(solver='cd', init='custom', shuffle=False)` itself,
in float64.

Run where sklearn is importable; the GPU box only reads the files.  X and the start are stored as
float32 and sklearn is given the same values as float64 arrays, so the golden is sklearn's fp64
answer on numbers that a float32 run sees unrounded.

A stop must not sit on a knife's edge: with the restatement (tests/hals_ref.py, which this script
checks against sklearn to 1e-12) it asserts, and records in the manifest, that no iteration's
violation / violation_init lies within 0.1 % (relative) of tol — twelve times the largest drift of
that ratio that rounding W to float32 every iteration produced in a CPU model (8.2e-5).

    python tests/golden/make_golden_hals.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hals_ref as ref  # noqa: E402
from cnmf_amd.synthetic import iop_spectra, random_init  # noqa: E402

TOL_MARGIN = 1e-3


def cases():
    """(name, X, W0, H0, kwargs)."""
    out = []
    stop = dict(tol=1e-4, max_iter=200)

    def start(X, k, seed):
        W0, H0 = random_init(X, k, seed)
        return X, W0, H0

    out.append(("k4", *start(iop_spectra(333, 81, seed=1), 4, 1), dict(stop)))
    out.append(("k8", *start(iop_spectra(337, 81, seed=2), 8, 2), dict(stop)))
    out.append(("k16", *start(iop_spectra(200, 300, seed=3), 16, 3), dict(stop)))
    out.append(("f17", *start(iop_spectra(150, 17, seed=4), 3, 4), dict(stop)))
    out.append(("tol0", *start(iop_spectra(333, 81, seed=1), 4, 1), dict(tol=0.0, max_iter=30)))
    out.append(("reg", *start(iop_spectra(120, 81, seed=5), 4, 5),
                dict(tol=0.0, max_iter=20, alpha_W=0.01, alpha_H=0.02, l1_ratio=0.5)))
    # all-zero rows in X; component 2 dead on both sides: a zero row of H0 makes the W-sweep's
    # hess zero, the zero column of W0 that it leaves makes the H-sweep's hess zero
    X, W0, H0 = start(iop_spectra(130, 81, seed=6), 4, 6)
    X[::9] = 0.0
    H0[2] = 0.0
    W0[:, 2] = 0.0
    out.append(("dead", X, W0, H0, dict(tol=1e-4, max_iter=40)))
    out.append(("k1", *start(iop_spectra(70, 5, seed=7), 1, 7), dict(tol=1e-4, max_iter=50)))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main():
    import sklearn
    from sklearn.decomposition import non_negative_factorization

    manifest = {"sklearn": sklearn.__version__, "numpy": np.__version__, "tol_margin": TOL_MARGIN, "cases": {}}

    def save(name, entry, **arrays):
        path = os.path.join(HERE, f"hals_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        entry["bytes"] = os.path.getsize(path)
        entry["sha"] = {k: _sha(v) for k, v in arrays.items() if isinstance(v, np.ndarray) and v.ndim}
        manifest["cases"][name] = entry

    def run(name, X, W0, H0, kw, update_H=True):
        k = H0.shape[0]
        X64, H64 = X.astype(np.float64), H0.astype(np.float64)
        W64 = None if W0 is None else W0.astype(np.float64)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            W, H, n_iter = non_negative_factorization(
                X64.copy(), None if W64 is None else W64.copy(), H64.copy(), n_components=k, init="custom",
                update_H=update_H, solver="cd", shuffle=False, **kw)
        warned = any("Maximum number of iterations" in str(w.message) for w in caught)
        reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
        l1_W, l1_H, l2_W, l2_H = ref.regularization(*X.shape, **reg)
        r = ref.fit(X64, W64, H64, tol=kw["tol"], max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W,
                    l2_H=l2_H, update_H=update_H)
        assert r["n_iter"] == n_iter, (name, r["n_iter"], n_iter)
        assert np.linalg.norm(r["W"] - W) <= 1e-12 * np.linalg.norm(W), name
        assert np.linalg.norm(r["H"] - H) <= 1e-12 * np.linalg.norm(H), name
        margin = ref.tol_margin(r["violations"], kw["tol"])
        assert margin is None or margin >= TOL_MARGIN, (name, margin)
        print(f"{name}: n_iter {n_iter} warned {warned} closest approach to tol {margin}")
        entry = dict(kwargs=kw, k=k, shape=list(X.shape), update_H=update_H, n_iter=int(n_iter), warned=warned,
                     min_tol_margin=margin)
        return W, H, n_iter, entry

    fitted = {}
    for name, X, W0, H0, kw in cases():
        W, H, n_iter, entry = run(name, X, W0, H0, kw)
        fitted[name] = H
        save(name, entry, X=X, W0=W0, H0=H0, W=W, H=H, n_iter=np.int64(n_iter))

    # transform: update_H=False against k4's fitted H (rounded to float32) on 100 new rows
    Xt = iop_spectra(100, 81, seed=8)
    Hf = fitted["k4"].astype(np.float32)
    W, H, n_iter, entry = run("transform", Xt, None, Hf, dict(tol=1e-4, max_iter=200), update_H=False)
    assert np.array_equal(H, Hf.astype(np.float64))
    save("transform", entry, X=Xt, H0=Hf, W=W, H=H, n_iter=np.int64(n_iter))

    with open(os.path.join(HERE, "MANIFEST_hals.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
