"""The fp64 restatement of solver='whals' (tests/whals_ref.py): with unit weights it is sklearn's
solver='cd' on every golden (exact n_iter, W and H to 1e-12); with weights the objective never
increases, values under zero weights are never used, and rows / columns masked whole reduce the
fit to the unweighted one of the submatrix.  Also: every weighted case of the GPU tests with tol > 0
stops at least 0.1 % away from tol."""
import json
import os

import numpy as np
import pytest

import hals_ref
import whals_cases as cases
import whals_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)
GOLDENS = ["k4", "k8", "k16", "f17", "tol0", "reg", "dead", "k1", "transform"]


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def golden_inputs(name):
    g = np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))
    c = MANIFEST["cases"][name]
    kw = c["kwargs"]
    reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
    l1_W, l1_H, l2_W, l2_H = ref.regularization(*c["shape"], **reg)
    W0 = g["W0"].astype(np.float64) if c["update_H"] else None
    opts = dict(tol=kw["tol"], max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H,
                update_H=c["update_H"])
    return g, g["X"].astype(np.float64), W0, g["H0"].astype(np.float64), opts


@pytest.mark.parametrize("name", GOLDENS)
def test_unit_weights_are_sklearn(name):
    g, X, W0, H0, opts = golden_inputs(name)
    r = ref.fit(X, np.ones_like(X), W0, H0, **opts)
    print(f"{name}: n_iter {r['n_iter']} relW {rel(r['W'], g['W']):.2e} relH {rel(r['H'], g['H']):.2e}")
    assert r["n_iter"] == int(g["n_iter"]) == MANIFEST["cases"][name]["n_iter"]
    assert rel(r["W"], g["W"]) <= 1e-12 and rel(r["H"], g["H"]) <= 1e-12


@pytest.mark.parametrize("zeros", [0.3, 0.6])
def test_objective_never_increases_and_masked_values_are_never_used(zeros):
    g, X, W0, H0, opts = golden_inputs("k4")
    M = ref.weights(X.shape, 7, zeros=zeros)
    r = ref.fit(X, M, W0, H0, **opts)
    obj = np.array([ref.objective(X, M, W0, H0)] + r["objectives"])
    assert r["n_iter"] > 5 and (np.diff(obj) <= 1e-12 * obj[:-1]).all()
    junk = X.copy()
    junk[M == 0] = 1e3 * np.random.RandomState(8).uniform(size=int((M == 0).sum()))
    rj = ref.fit(junk, M, W0, H0, **opts)
    assert rj["n_iter"] == r["n_iter"] and np.array_equal(rj["W"], r["W"]) and np.array_equal(rj["H"], r["H"])


def test_masked_rows_and_columns_give_the_submatrix_fit():
    g, X, W0, H0, opts = golden_inputs("k4")
    kr, kc = np.arange(X.shape[0]) % 7 != 3, np.arange(X.shape[1]) % 5 != 1
    M = np.ones_like(X)
    M[~kr] = 0.0
    M[:, ~kc] = 0.0
    r = ref.fit(X, M, W0, H0, **opts)
    sub = hals_ref.fit(X[kr][:, kc], W0[kr], H0[:, kc], **opts)
    assert r["n_iter"] == sub["n_iter"]
    assert rel(r["W"][kr], sub["W"]) <= 1e-12 and rel(r["H"][:, kc], sub["H"]) <= 1e-12
    assert np.array_equal(r["W"][~kr], W0[~kr]) and np.array_equal(r["H"][:, ~kc], H0[:, ~kc])


@pytest.mark.parametrize("name, dt", [p for p in cases.PARAMS if cases.CASES[p[0]]["tol"] > 0])
def test_gpu_cases_stop_away_from_tol(name, dt):
    c = cases.CASES[name]
    r = cases.expected(name, dt)
    margin = ref.tol_margin(r["violations"], c["tol"])
    print(f"{name} {dt}: n_iter {r['n_iter']} margin {margin:.2e}")
    assert margin >= 1e-3
    if name == "masked":
        sub = cases.expected_submatrix(name, dt)
        assert sub["n_iter"] == r["n_iter"] and ref.tol_margin(sub["violations"], c["tol"]) >= 1e-3


def test_gpu_cases_are_what_they_claim():
    X, M, W0, H0 = cases.inputs("w30", "f32")
    assert X.dtype == M.dtype == W0.dtype == np.float32 and 0.25 < (M == 0).mean() < 0.35
    assert M[M > 0].min() >= 0.25 and M.max() <= 4.0
    assert cases.inputs("transform", "f64")[2] is None
    X, M, _, _ = cases.inputs("masked", "f64")
    kr, kc = cases.kept("masked")
    assert not M[~kr].any() and not M[:, ~kc].any() and (M[kr][:, kc] == 1).all()
    for name, F, k, itemsize in (("k5f83", 83, 5, 4), ("k8f81", 81, 8, 8)):
        assert (F * itemsize) % 16 != 0 and cases.CASES[name]["shape"][0] % 64 != 0
