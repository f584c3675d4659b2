"""Generate the factorise_multistart golden vectors (tests/golden/ms_*.npz + MANIFEST_multistart.json)
by running scikit-learn 1.7.2's `non_negative_factorization(solver='cd', init='custom',
shuffle=False)` itself, in float64, once per start.

Run where sklearn is importable; the GPU box only reads the files.  X is stored as float32.  A start
of init='random' depends on X's dtype (sklearn draws and scales it in X's dtype), so every case
holds two sets of starts and of sklearn's answers for the same seeds:
  W0 / H0 (float32)      the starts `random_init(X, k, seed)` of the float32 X, and W / H / n_iter /
                         errors: sklearn's fp64 answer from these values given as float64 arrays;
  W0_64 / H0_64          the starts of X.astype(float64), and W_64 / H_64 / n_iter_64 / errors_64:
                         sklearn's answer from them — what a float64 fit with init='random' sees.

A stop must not sit on a knife's edge: with the restatement (tests/hals_ref.py, which this script
checks against sklearn to 1e-12 for every start) it asserts, and records in the manifest, that no
iteration's violation / violation_init of any start lies within TOL_MARGIN (relative) of tol — the
margin of the HALS goldens.  The best start must beat the runner-up by more than BEST_GAP relative,
so that `best` cannot flip on rounding; k1, whose starts reach the same error, is exempt (it tests
the tie rule).  The regularised case `reg` runs 10 iterations at tol = 0: its starts run into the
same point (after 20 iterations the two best are 1.1e-5 apart, after 40 2.8e-9), and after 10 the
best leads by 6.6e-4.

    python tests/golden/make_golden_multistart.py
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
BEST_GAP = 1e-4
GAP_EXEMPT = ("k1",)


def cases():
    """(name, X, k, seeds, kwargs)."""
    stop = dict(tol=1e-4, max_iter=200)
    Xz = iop_spectra(130, 81, seed=6)
    Xz[::9] = 0.0
    return [
        ("k4", iop_spectra(333, 81, seed=1), 4, [0, 1, 2, 3, 4, 5], dict(stop)),
        ("k8", iop_spectra(337, 81, seed=2), 8, [1, 2, 3, 4, 5], dict(stop)),
        ("k16", iop_spectra(200, 300, seed=3), 16, [1, 2, 3], dict(stop)),
        ("f17", iop_spectra(150, 17, seed=4), 3, [0, 1, 2, 3, 4], dict(stop)),
        ("k1", iop_spectra(70, 5, seed=7), 1, [0, 1, 2], dict(tol=1e-4, max_iter=50)),
        ("reg", iop_spectra(120, 81, seed=5), 4, [0, 1, 2],
         dict(tol=0.0, max_iter=10, alpha_W=0.01, alpha_H=0.02, l1_ratio=0.5)),
        ("zero", Xz, 4, [0, 1, 2, 3], dict(tol=1e-4, max_iter=60)),
    ]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main():
    import sklearn
    from sklearn.decomposition import non_negative_factorization

    manifest = {"sklearn": sklearn.__version__, "numpy": np.__version__, "tol_margin": TOL_MARGIN,
                "best_gap": BEST_GAP, "cases": {}}

    def run(name, X64, W0, H0, kw):
        """sklearn from one start (given as float64), checked against the restatement."""
        k = H0.shape[0]
        W64, H64 = W0.astype(np.float64), H0.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W, H, n_iter = non_negative_factorization(X64.copy(), W64.copy(), H64.copy(), n_components=k,
                                                      init="custom", solver="cd", shuffle=False, **kw)
        reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
        l1_W, l1_H, l2_W, l2_H = ref.regularization(*X64.shape, **reg)
        r = ref.fit(X64, W64, H64, tol=kw["tol"], max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W,
                    l2_H=l2_H)
        assert r["n_iter"] == n_iter, (name, r["n_iter"], n_iter)
        assert np.linalg.norm(r["W"] - W) <= 1e-12 * np.linalg.norm(W), name
        assert np.linalg.norm(r["H"] - H) <= 1e-12 * np.linalg.norm(H), name
        margin = ref.tol_margin(r["violations"], kw["tol"])
        assert margin is None or margin >= TOL_MARGIN, (name, margin)
        return W, H, int(n_iter), margin, float(np.linalg.norm(X64 - W @ H))

    def run_starts(name, X64, starts, kw):
        out = [run(name, X64, W0, H0, kw) for W0, H0 in starts]
        W, H = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        n_iter, errors = np.array([o[2] for o in out], dtype=np.int64), np.array([o[4] for o in out])
        margins = [o[3] for o in out if o[3] is not None]
        order = np.sort(errors)
        gap = float((order[1] - order[0]) / order[0])
        if name not in GAP_EXEMPT:
            assert gap > BEST_GAP, (name, gap)
        return W, H, n_iter, errors, (min(margins) if margins else None), gap

    for name, X, k, seeds, kw in cases():
        assert X.dtype == np.float32
        X64 = X.astype(np.float64)
        s32 = [random_init(X, k, s) for s in seeds]
        s64 = [random_init(X64, k, s) for s in seeds]
        assert all(W0.dtype == np.float32 and H0.dtype == np.float32 for W0, H0 in s32)
        W, H, n_iter, errors, margin, gap = run_starts(name, X64, s32, kw)
        W_64, H_64, n_iter_64, errors_64, margin_64, gap_64 = run_starts(name, X64, s64, kw)
        print(f"{name}: n_iter {n_iter.tolist()} ({n_iter_64.tolist()} from the float64 starts) closest approach "
              f"to tol {margin} ({margin_64}) best {int(np.argmin(errors))} gap {gap:.2e} ({gap_64:.2e})")
        arrays = dict(X=X, seeds=np.array(seeds, dtype=np.int64),
                      W0=np.stack([a for a, _ in s32]), H0=np.stack([b for _, b in s32]), W=W, H=H, n_iter=n_iter,
                      errors=errors, W0_64=np.stack([a for a, _ in s64]), H0_64=np.stack([b for _, b in s64]),
                      W_64=W_64, H_64=H_64, n_iter_64=n_iter_64, errors_64=errors_64)
        path = os.path.join(HERE, f"ms_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        manifest["cases"][name] = dict(
            kwargs=kw, k=k, shape=list(X.shape), seeds=seeds, n_iter=n_iter.tolist(), n_iter_64=n_iter_64.tolist(),
            min_tol_margin=margin, min_tol_margin_64=margin_64, best=int(np.argmin(errors)),
            best_64=int(np.argmin(errors_64)), best_gap=gap, best_gap_64=gap_64, bytes=os.path.getsize(path),
            sha={k_: _sha(v) for k_, v in arrays.items()})

    with open(os.path.join(HERE, "MANIFEST_multistart.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
