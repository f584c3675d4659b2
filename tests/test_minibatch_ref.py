"""The fp64 restatement of sklearn's MiniBatchNMF (tests/minibatch_ref.py) against every golden
(tests/golden/mb_*.npz, written by sklearn 1.7.2 itself): W and H to 1e-12 relative Frobenius,
n_steps, n_iter and the stop reason equal."""
import json
import os

import numpy as np
import pytest

import minibatch_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_minibatch.json")) as f:
    MANIFEST = json.load(f)

FIT_CASES = ["hstop", "noimp", "tol0", "b301", "bigbatch", "reg20x10", "k8", "k16", "f17", "zerorows"]
REASON = {"hstop": ref.STOP_H_CHANGE, "noimp": ref.STOP_NO_IMPROVEMENT}


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def load(name):
    return np.load(os.path.join(GOLDEN, f"mb_{name}.npz"))


def test_manifest_lists_every_case_with_its_margins():
    assert sorted(MANIFEST["cases"]) == sorted(FIT_CASES + ["transform", "partial"])
    for name, c in MANIFEST["cases"].items():
        assert c["bytes"] < (1 << 20), name
        if c["kwargs"].get("tol", 0) > 0 and "min_hdiff_margin" in c:
            assert c["min_hdiff_margin"] >= 1e-2, name
        if c["kwargs"].get("max_no_improvement") is not None:
            assert c["min_ewa_margin"] >= 1e-3, name
        if "min_wdiff_margin" in c:
            assert c["min_wdiff_margin"] >= 1e-2, name


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_matches_sklearn(name):
    g = load(name)
    kw = MANIFEST["cases"][name]["kwargs"]
    r = ref.fit(g["X"].astype(np.float64), g["W0"], g["H0"], **kw)
    assert r["n_steps"] == int(g["n_steps"]) and r["n_iter"] == int(g["n_iter"])
    assert r["reason"] == int(g["reason"]) == REASON.get(name, ref.STOP_NONE)
    assert rel(r["W"], g["W"]) <= 1e-12 and rel(r["H"], g["H"]) <= 1e-12
    err = np.linalg.norm(g["X"].astype(np.float64) - r["W"] @ r["H"])
    assert abs(err - float(g["reconstruction_err"])) <= 1e-12 * err
    if name == "zerorows":  # the eps rule left the zero rows' W at zero
        assert not g["X"][::7].any() and not r["W"][::7].any()


def test_cases_cover_the_batch_shapes():
    c = MANIFEST["cases"]
    assert c["hstop"]["shape"][0] % c["hstop"]["kwargs"]["batch_size"] != 0            # ragged last batch
    assert c["bigbatch"]["kwargs"]["batch_size"] > c["bigbatch"]["shape"][0]
    assert c["b301"]["kwargs"]["batch_size"] * c["b301"]["shape"][1] * 4 % 16 != 0     # misaligned windows
    assert c["tol0"]["n_steps"] == c["tol0"]["kwargs"]["max_iter"] * 4
    assert (c["k8"]["k"], c["k16"]["k"], c["f17"]["shape"][1]) == (8, 16, 17)
    assert c["reg20x10"]["shape"] == [20, 10] and c["reg20x10"]["kwargs"]["alpha_W"] > 0


def test_transform_matches_sklearn():
    g = load("transform")
    c = MANIFEST["cases"]["transform"]
    log = []
    W, n = ref.solve_w(g["Xt"].astype(np.float64), g["H"], c["transform_max_iter"], c["kwargs"]["tol"], log=log)
    assert n == int(g["w_iters"]) == len(log) < c["transform_max_iter"]
    assert rel(W, g["Wt"]) <= 1e-12
    r = ref.fit(g["X"].astype(np.float64), g["W0"], g["H0"], **c["kwargs"])
    assert rel(r["H"], g["H"]) <= 1e-12 and r["n_steps"] == int(g["n_steps"])


def test_partial_fit_sequence_matches_sklearn():
    g = load("partial")
    c = MANIFEST["cases"]["partial"]
    X = g["X"]
    chunks = [X[250 * i:250 * (i + 1)] for i in range(c["chunks"])]
    H, steps = ref.partial_fit_sequence(chunks, g["H0"], **c["kwargs"])
    assert steps == int(g["n_steps"]) == 4
    assert rel(H, g["H"]) <= 1e-12
