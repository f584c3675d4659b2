"""The factorise_multistart goldens (tests/golden/ms_*.npz) against the fp64 restatement of sklearn's
coordinate-descent solver (tests/hals_ref.py): every start of every case, from the float32 starts
and from the float64 ones, n_iter equal and W, H to 1e-12; the manifest's records of what the
generator asserted."""
import json
import os

import numpy as np
import pytest

import hals_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_multistart.json")) as f:
    MANIFEST = json.load(f)
CASES = ["k4", "k8", "k16", "f17", "k1", "reg", "zero"]


def test_manifest_lists_the_cases():
    assert sorted(MANIFEST["cases"]) == sorted(CASES)
    assert MANIFEST["tol_margin"] == 1e-3 and MANIFEST["best_gap"] == 1e-4
    for name, c in MANIFEST["cases"].items():
        assert c["bytes"] == os.path.getsize(os.path.join(GOLDEN, f"ms_{name}.npz")) < (1 << 20)
        for m in (c["min_tol_margin"], c["min_tol_margin_64"]):
            assert m is None or m >= MANIFEST["tol_margin"], name
        if name != "k1":  # its three starts reach the same error: the tie rule
            assert c["best_gap"] > MANIFEST["best_gap"] and c["best_gap_64"] > MANIFEST["best_gap"], name
    assert MANIFEST["cases"]["k1"]["best"] == 0 and MANIFEST["cases"]["k1"]["best_64"] == 0
    assert MANIFEST["cases"]["k4"]["n_iter"] == [200, 61, 200, 200, 200, 200]


@pytest.mark.parametrize("suffix", ["", "_64"], ids=["f32-starts", "f64-starts"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_start(name, suffix):
    g, c = np.load(os.path.join(GOLDEN, f"ms_{name}.npz")), MANIFEST["cases"][name]
    kw = c["kwargs"]
    reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
    l1_W, l1_H, l2_W, l2_H = ref.regularization(*c["shape"], **reg)
    X = g["X"].astype(np.float64)
    assert g["X"].dtype == np.float32 and g["W0"].dtype == np.float32 and g["W0_64"].dtype == np.float64
    assert g["seeds"].tolist() == c["seeds"] and len(c["seeds"]) == g["W0" + suffix].shape[0]
    for r in range(len(c["seeds"])):
        out = ref.fit(X, g["W0" + suffix][r].astype(np.float64), g["H0" + suffix][r].astype(np.float64), tol=kw["tol"],
                      max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H)
        W, H = g["W" + suffix][r], g["H" + suffix][r]
        assert out["n_iter"] == int(g["n_iter" + suffix][r]) == c["n_iter" + suffix][r], (name, r)
        assert np.linalg.norm(out["W"] - W) <= 1e-12 * np.linalg.norm(W), (name, r)
        assert np.linalg.norm(out["H"] - H) <= 1e-12 * np.linalg.norm(H), (name, r)
        err = np.linalg.norm(X - W @ H)
        assert abs(err - g["errors" + suffix][r]) <= 1e-12 * err
    assert int(np.argmin(g["errors" + suffix])) == c["best" + suffix]
