"""Generate the MiniBatchNMF golden vectors (tests/golden/mb_*.npz + MANIFEST_minibatch.json) by
running scikit-learn 1.7.2's MiniBatchNMF itself, in float64.

Run where sklearn is importable; the GPU box only reads the files.  float32 cases store a float32
X (and start) and sklearn is given the same values as float64 arrays, so the golden is sklearn's
fp64 answer on exactly the numbers the GPU sees.

Stopping cases must not sit on a knife's edge: the GPU's ~1e-6 arithmetic differences may not flip
a stop.  With the restatement (tests/minibatch_ref.py, which reproduces sklearn's steps) this script
asserts, and records in the manifest, that over all steps of every stopping case
|H_diff - tol| / tol >= 1e-2, that every ewa_cost vs ewa_cost_min comparison is separated by >= 1e-3
relative, and that |W_diff - tol| / tol >= 1e-2 over the transform case's iterations.

    python tests/golden/make_golden_minibatch.py
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

import minibatch_ref as ref  # noqa: E402
from cnmf_amd.synthetic import iop_spectra, random_init  # noqa: E402

H_MARGIN, EWA_MARGIN = 1e-2, 1e-3


def fit_cases():
    """(name, X, k, init seed, kwargs): fits from sklearn's 'random' start restated by random_init."""
    out = []
    f32, f64 = np.float32, np.float64
    # stop by the change of H; 1000 = 3 x 300 + 100: a ragged last batch
    out.append(("hstop", iop_spectra(1000, 81, seed=0, dtype=f32), 5, 0,
                dict(batch_size=300, tol=1e-3, max_no_improvement=None, max_iter=200)))
    # stop by lack of improvement of the smoothed cost
    out.append(("noimp", iop_spectra(2048, 81, seed=3, dtype=f32), 4, 3,
                dict(batch_size=256, tol=1e-4, max_no_improvement=3, max_iter=200)))
    # fixed number of steps
    out.append(("tol0", iop_spectra(1000, 81, seed=1, dtype=f64), 4, 1,
                dict(batch_size=256, tol=0.0, max_no_improvement=None, max_iter=5)))
    # windows that start misaligned (301 rows x 81 floats)
    out.append(("b301", iop_spectra(1000, 81, seed=2, dtype=f32), 4, 2,
                dict(batch_size=301, tol=0.0, max_no_improvement=None, max_iter=6)))
    # batch_size > n
    out.append(("bigbatch", iop_spectra(500, 81, seed=4, dtype=f32), 4, 4,
                dict(batch_size=1024, tol=0.0, max_no_improvement=None, max_iter=10)))
    # l1 + l2 regularisation on sklearn's 20 x 10 test shape
    rng = np.random.mtrand.RandomState(1337)
    out.append(("reg20x10", np.abs(rng.randn(20, 10)), 5, 42,
                dict(batch_size=7, tol=0.0, max_no_improvement=None, max_iter=10, alpha_W=0.1, alpha_H=0.05,
                     l1_ratio=0.5)))
    out.append(("k8", iop_spectra(384, 300, seed=5, dtype=f32), 8, 5,
                dict(batch_size=128, tol=0.0, max_no_improvement=None, max_iter=5)))
    out.append(("k16", iop_spectra(300, 300, seed=6, dtype=f32), 16, 6,
                dict(batch_size=100, tol=0.0, max_no_improvement=None, max_iter=5)))
    out.append(("f17", iop_spectra(500, 17, seed=7, dtype=f64), 3, 7,
                dict(batch_size=128, tol=0.0, max_no_improvement=None, max_iter=8)))
    # zero rows in X: their W goes to zero and the zero denominator takes the eps rule
    Xz = iop_spectra(400, 81, seed=8, dtype=f32)
    Xz[::7] = 0.0
    out.append(("zerorows", Xz, 4, 8, dict(batch_size=128, tol=0.0, max_no_improvement=None, max_iter=5)))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def main():
    from sklearn.decomposition import MiniBatchNMF
    import sklearn

    manifest = {"sklearn": sklearn.__version__, "numpy": np.__version__, "h_margin": H_MARGIN,
                "ewa_margin": EWA_MARGIN, "cases": {}}

    def save(name, entry, **arrays):
        path = os.path.join(HERE, f"mb_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), (name, os.path.getsize(path))
        entry["bytes"] = os.path.getsize(path)
        entry["sha"] = {k: _sha(v) for k, v in arrays.items() if isinstance(v, np.ndarray) and v.ndim}
        manifest["cases"][name] = entry

    for name, X, k, seed, kw in fit_cases():
        W0, H0 = random_init(X, k, seed)
        X64, W64, H64 = (a.astype(np.float64) for a in (X, W0, H0))
        est = MiniBatchNMF(n_components=k, init="custom", **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W = est.fit_transform(X64.copy(), W=W64.copy(), H=H64.copy())
        r = ref.fit(X64, W64, H64, **kw)
        assert r["n_steps"] == est.n_steps_ and r["n_iter"] == est.n_iter_, (name, r["n_steps"], est.n_steps_)
        assert np.linalg.norm(r["H"] - est.components_) <= 1e-12 * np.linalg.norm(est.components_), name
        hm = min([m for w, m in r["margins"] if w == "hdiff"], default=None)
        em = min([m for w, m in r["margins"] if w == "ewa"], default=None)
        if kw["tol"] > 0:
            assert hm >= H_MARGIN, (name, hm)
        if kw["max_no_improvement"] is not None:
            assert em >= EWA_MARGIN, (name, em)
        save(name, dict(kwargs=kw, k=k, dtype=X.dtype.name, shape=list(X.shape), n_steps=int(est.n_steps_),
                        n_iter=int(est.n_iter_), reason=int(r["reason"]), min_hdiff_margin=hm, min_ewa_margin=em),
             X=X, W0=W0, H0=H0, W=W, H=est.components_, n_steps=np.int64(est.n_steps_),
             n_iter=np.int64(est.n_iter_), reason=np.int64(r["reason"]),
             reconstruction_err=np.float64(est.reconstruction_err_))
        print(f"{name}: steps {est.n_steps_} iter {est.n_iter_} reason {r['reason']} margins {hm} {em}")

    # transform: a short fit, then _solve_W of other rows with its own tolerance stop
    X = iop_spectra(800, 81, seed=9, dtype=np.float32)
    Xt = iop_spectra(600, 81, seed=13, dtype=np.float32)
    W0, H0 = random_init(X, 4, 9)
    kw = dict(batch_size=200, tol=1e-3, max_no_improvement=None, max_iter=3)
    est = MiniBatchNMF(n_components=4, init="custom", transform_max_iter=100, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X.astype(np.float64), W=W0.astype(np.float64), H=H0.astype(np.float64))
        Wt = est.transform(Xt.astype(np.float64))
    r = ref.fit(X.astype(np.float64), W0, H0, **kw)
    hm = min(m for w, m in r["margins"] if w == "hdiff")
    assert hm >= H_MARGIN and r["n_steps"] == est.n_steps_, ("transform fit", hm)
    log = []
    Wr, n_w = ref.solve_w(Xt.astype(np.float64), est.components_, 100, kw["tol"], log=log)
    wm = min(abs(d - kw["tol"]) / kw["tol"] for d in log)
    assert wm >= H_MARGIN, ("transform", wm)
    assert np.linalg.norm(Wr - Wt) <= 1e-12 * np.linalg.norm(Wt)
    save("transform", dict(kwargs=kw, transform_max_iter=100, k=4, dtype="float32", shape=list(Xt.shape), n_steps=int(est.n_steps_),
                           n_iter=int(est.n_iter_), w_iters=n_w, min_hdiff_margin=hm, min_wdiff_margin=wm),
         X=X, W0=W0, H0=H0, H=est.components_, Xt=Xt, Wt=Wt, w_iters=np.int64(n_w),
         n_steps=np.int64(est.n_steps_), n_iter=np.int64(est.n_iter_))
    print(f"transform: fit steps {est.n_steps_}, solve_W iterations {n_w}, margins {hm} {wm}")

    # partial_fit over four chunks
    X = iop_spectra(1000, 81, seed=11, dtype=np.float32)
    W0, H0 = random_init(X[:250], 4, 11)
    kw = dict(batch_size=1024, tol=8e-3, fresh_restarts_max_iter=30)
    est = MiniBatchNMF(n_components=4, init="custom", **kw)
    logs = []
    for i in range(4):
        c = X[250 * i:250 * (i + 1)].astype(np.float64)
        lg = []
        ref.solve_w(c, H0.astype(np.float64) if i == 0 else est.components_, 30, kw["tol"], log=lg)
        logs += lg
        est.partial_fit(c, W=W0.astype(np.float64), H=H0.astype(np.float64))
    wm = min(abs(d - kw["tol"]) / kw["tol"] for d in logs)
    assert wm >= H_MARGIN, ("partial_fit", wm)
    Hr, steps = ref.partial_fit_sequence([X[250 * i:250 * (i + 1)] for i in range(4)], H0, **kw)
    assert steps == est.n_steps_ and np.linalg.norm(Hr - est.components_) <= 1e-12 * np.linalg.norm(Hr)
    save("partial", dict(kwargs=kw, k=4, dtype="float32", shape=list(X.shape), chunks=4, n_steps=int(est.n_steps_),
                         min_wdiff_margin=wm),
         X=X, W0=W0, H0=H0, H=est.components_, n_steps=np.int64(est.n_steps_))
    print(f"partial_fit: steps {est.n_steps_}, W_diff margin {wm}")

    with open(os.path.join(HERE, "MANIFEST_minibatch.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
