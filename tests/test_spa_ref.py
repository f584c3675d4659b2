"""tests/spa_ref.py, the NumPy fp64 specification of init='spa': it reproduces every golden
(tests/golden/spa_*.npz, written by make_golden_spa.py, which checked the picks against LAPACK's
pivoted QR), keeps Q orthonormal, stops at the rank of X, never picks a zero row and takes the lower
index of a duplicated best row."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from spa_ref import margins, spa_ref, spa_start_ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
with open(os.path.join(GOLDEN, "MANIFEST_spa.json")) as f:
    MANIFEST = json.load(f)


def golden_x(name):
    """The case's X: stored, or regenerated from the seed by the generator's recipe."""
    from cnmf_amd.synthetic import iop_spectra
    e = MANIFEST[name]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    dtype = np.dtype(e["dtype"])
    X = iop_spectra(e["n"], e["F"], seed=e["seed"], dtype=np.float32 if e["widened"] else dtype).astype(dtype)
    if e["stores_X"]:
        assert np.array_equal(X, g["X"]) and g["X"].dtype == dtype
    return X, g


def rank2():
    rng = np.random.default_rng(0)
    return (rng.integers(0, 5, (40, 2)) @ rng.integers(1, 5, (2, 9))).astype(float)


def test_manifest_lists_the_cases_with_their_margins():
    assert len(MANIFEST) == 14
    for name, e in MANIFEST.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)
        for tag in ("l1", "none"):
            assert e[tag]["min_margin"] >= 1e-4 and len(e[tag]["idx"]) == e["k"]


@pytest.mark.parametrize("name", sorted(MANIFEST))
@pytest.mark.parametrize("normalise", ["l1", None])
def test_reproduces_golden(name, normalise):
    X, g = golden_x(name)
    tag = "l1" if normalise == "l1" else "none"
    idx, info = spa_ref(X, int(g["k"]), normalise=normalise, return_scores=True)
    assert idx.dtype == np.int64 and np.array_equal(idx, g[f"idx_{tag}"])
    for j, rho in enumerate(g[f"rho_{tag}"]):  # another BLAS: the bound the device is held to
        assert np.linalg.norm(info["Q"][j] - g[f"Q_{tag}"][j]) <= 1e-12 / rho
    np.testing.assert_allclose(info["rho"], g[f"rho_{tag}"], rtol=1e-6)
    np.testing.assert_allclose(margins(info["scores"]), g[f"margins_{tag}"], rtol=1e-3, atol=1e-7)
    Q = info["Q"]
    assert np.abs(Q @ Q.T - np.eye(len(idx))).max() <= 1e-14
    assert info["rho"][0] == 1.0 and np.all(np.diff(info["rho"]) <= 0)


def test_rank_two_matrix_stops_with_two_rows():
    X = rank2()
    idx, info = spa_ref(X, 4, return_scores=True)
    assert len(idx) == 2 and info["steps"] == 2 and info["Q"].shape == (2, 9)
    assert np.sqrt(info["scores"][2].max()) / info["ymax"] <= 1e-12  # the third residual: ~2.6e-16
    idx_none, _ = spa_ref(X, 4, normalise=None)
    assert len(idx_none) == 2


def test_zero_rows_are_never_picked():
    from cnmf_amd.synthetic import iop_spectra
    X = iop_spectra(180, 17, seed=4)
    X[::9] = 0
    for normalise in ("l1", None):
        idx, _ = spa_ref(X, 3, normalise=normalise)
        assert len(idx) == 3 and np.all(idx % 9 != 0)
    idx, info = spa_ref(np.zeros((5, 4)), 2)
    assert len(idx) == 0 and info["steps"] == 0


def test_duplicated_best_row_gives_the_lower_index():
    from cnmf_amd.synthetic import iop_spectra
    X = iop_spectra(150, 17, seed=4)
    p = int(spa_ref(X, 1)[0][0])
    lo, hi = (p - 40) % 150, (p + 40) % 150
    X[hi] = X[p]
    assert int(spa_ref(X, 1)[0][0]) == min(p, hi)
    X[lo] = X[p]
    assert int(spa_ref(X, 1)[0][0]) == min(lo, p, hi)


def test_start_is_the_specified_one():
    X, g = golden_x("spa_333x81_k4_float32")
    idx = g["idx_l1"]
    W0, H0, M, floor = spa_start_ref(X, idx)
    assert W0.dtype == X.dtype and H0.dtype == X.dtype and M.shape == (81, 4)
    assert floor == float(X.astype(np.float64).mean()) / 100
    assert np.array_equal(H0, np.where(X[idx] == 0, np.float32(floor), X[idx])) and W0.min() >= np.float32(floor)
    # the picked rows reproduce themselves: W0[p_j] = e_j up to the floor
    np.testing.assert_allclose(W0[idx], np.maximum(np.eye(4), floor), atol=1e-5)
