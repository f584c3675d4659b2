"""The sharded restatement of solver='hals' (tests/hals_shard_ref.py) against every golden
(tests/golden/hals_*.npz, sklearn 1.7.2's own answers) at worlds 2, 3 and 5: the exact n_iter, W and
H to 1e-12 relative Frobenius (only the order of the sums over the rows differs; the worst measured
is 4.5e-14).  This is what lets the sharded GPU fit keep the bars of the one-device fit."""
import json
import os

import numpy as np
import pytest

import hals_ref as ref
import hals_shard_ref as shard_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)

CASES = ["k4", "k8", "k16", "f17", "tol0", "reg", "dead", "k1", "transform"]
WORLDS = [2, 3, 5]


def rel(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b)


def run(name, world):
    g = np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))
    c = MANIFEST["cases"][name]
    kw = c["kwargs"]
    reg = {a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw}
    l1_W, l1_H, l2_W, l2_H = ref.regularization(*c["shape"], **reg)  # from the global shape
    W0 = g["W0"].astype(np.float64) if c["update_H"] else None
    r = shard_ref.fit(g["X"].astype(np.float64), W0, g["H0"].astype(np.float64), world, tol=kw["tol"],
                      max_iter=kw["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H, update_H=c["update_H"])
    return g, c, r


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", CASES)
def test_sharded_ref_matches_sklearn(name, world):
    g, c, r = run(name, world)
    ew, eh = rel(r["W"], g["W"]), rel(r["H"], g["H"])
    print(f"{name} world {world}: n_iter {r['n_iter']} relW {ew:.2e} relH {eh:.2e}")
    assert r["n_iter"] == int(g["n_iter"]) == c["n_iter"]
    assert ew <= 1e-12 and eh <= 1e-12
    margin = ref.tol_margin(r["violations"], c["kwargs"]["tol"])
    assert margin is None or margin >= 1e-3


def test_shards_are_contiguous_and_an_empty_one_changes_nothing():
    g, c, r = run("k1", 5)
    assert r["bounds"][0][0] == 0 and r["bounds"][-1][1] == 70
    assert all(a[1] == b[0] for a, b in zip(r["bounds"], r["bounds"][1:]))
    X, W0, H0 = (g[n].astype(np.float64) for n in ("X", "W0", "H0"))
    # 2 rows over 3 ranks: the last rank owns none
    few = shard_ref.fit(X[:2], W0[:2], H0, 3, tol=0.0, max_iter=10)
    one = ref.fit(X[:2], W0[:2], H0, tol=0.0, max_iter=10)
    assert few["bounds"] == [(0, 1), (1, 2), (2, 2)] and few["n_iter"] == one["n_iter"] == 10
    assert rel(few["W"], one["W"]) <= 1e-12 and rel(few["H"], one["H"]) <= 1e-12
