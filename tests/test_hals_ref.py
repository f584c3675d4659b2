"""The fp64 restatement of sklearn's coordinate-descent solver (tests/hals_ref.py) against every
golden (tests/golden/hals_*.npz, written by sklearn 1.7.2's solver='cd' itself): W and H to 1e-12
relative Frobenius and the exact n_iter."""
import json
import os

import numpy as np
import pytest

import hals_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)

CASES = ["k4", "k8", "k16", "f17", "tol0", "reg", "dead", "k1", "transform"]


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def load(name):
    return np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))


def run_ref(name, g=None, dtype=np.float64):
    """hals_ref on the case's inputs as the GPU sees them in `dtype` (rounded, then fp64)."""
    g = load(name) if g is None else g
    c = MANIFEST["cases"][name]
    kw = c["kwargs"]
    reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
    l1_W, l1_H, l2_W, l2_H = ref.regularization(*c["shape"], **reg)
    W0 = g["W0"].astype(dtype).astype(np.float64) if c["update_H"] else None
    return ref.fit(g["X"].astype(dtype).astype(np.float64), W0, g["H0"].astype(dtype).astype(np.float64),
                   tol=kw["tol"], max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H,
                   update_H=c["update_H"])


def test_manifest_lists_every_case_with_its_margin():
    assert sorted(MANIFEST["cases"]) == sorted(CASES)
    assert MANIFEST["sklearn"] == "1.7.2" and MANIFEST["tol_margin"] == 1e-3
    for name, c in MANIFEST["cases"].items():
        assert c["bytes"] < (1 << 20), name
        if c["kwargs"]["tol"] > 0:
            assert c["min_tol_margin"] >= 1e-3, name


@pytest.mark.parametrize("name", CASES)
def test_ref_matches_sklearn(name):
    g = load(name)
    r = run_ref(name, g)
    assert r["n_iter"] == int(g["n_iter"]) == MANIFEST["cases"][name]["n_iter"]
    assert rel(r["W"], g["W"]) <= 1e-12 and rel(r["H"], g["H"]) <= 1e-12
    margin = ref.tol_margin(r["violations"], MANIFEST["cases"][name]["kwargs"]["tol"])
    assert margin is None or margin >= 1e-3


def test_cases_are_what_they_claim():
    c = MANIFEST["cases"]
    assert (c["k4"]["n_iter"], c["k8"]["n_iter"], c["k16"]["n_iter"], c["f17"]["n_iter"]) == (61, 200, 103, 200)
    assert c["k8"]["warned"] and c["f17"]["warned"] and not c["k4"]["warned"] and not c["k16"]["warned"]
    assert c["tol0"]["n_iter"] == c["tol0"]["kwargs"]["max_iter"] == 30 and c["tol0"]["kwargs"]["tol"] == 0
    assert c["reg"]["kwargs"]["alpha_W"] == 0.01 and c["reg"]["kwargs"]["alpha_H"] == 0.02 and c["reg"]["n_iter"] == 20
    assert (c["k1"]["k"], c["k1"]["shape"]) == (1, [70, 5])
    assert not c["transform"]["update_H"] and c["transform"]["shape"][0] == 100
    # both hess == 0 branches: the dead component stays exactly as it started, on both sides
    g = load("dead")
    assert not g["X"][::9].any() and not g["H0"][2].any() and not g["W0"][:, 2].any()
    assert not g["H"][2].any() and not g["W"][:, 2].any() and g["H"][[0, 1, 3]].any(axis=1).all()
    # the transform case fixed H and started from W = 0
    g = load("transform")
    assert np.array_equal(g["H"], g["H0"].astype(np.float64)) and "W0" not in g.files
