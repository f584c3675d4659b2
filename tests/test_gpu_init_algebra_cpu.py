"""The host algebra of the GPU NNDSVD init (cnmf_amd/gpu_init.py: _nndsvd, _combine_stats) without a
GPU: the product's own algebra over NumPy fp64 passes (tests/gpu_init_ref.py: NumpyPasses).

a. every `init_*` golden of tests/test_gpu_init.py at its bars (fp64 X 1e-8, fp32 X 2e-5 relative
   Frobenius, identical zero patterns);
b. rank-deficient X (rank 2 with k = 4, and all zeros): before the fix the dropped components'
   H rows were 0/0 = NaN;
c. edge shapes (ragged last tile, several workgroups of stats rows, F = 96 / 95 / 1, k = 16 / 5 / 3 /
   1, bf16-rounded X) against the host restatement on the same values in fp64, identical fill
   patterns."""
import warnings

import numpy as np
import pytest

from golden_io import init_names, load_init, rel_fro
from gpu_init_ref import (EDGE_NAMES, NumpyPasses, check_rank2, edge_cases, edge_host, nndsvd_numpy, rank2_x,
                          stats_ref)

from cnmf_amd.gpu_init import _combine_stats
from cnmf_amd.init import initialize_nmf


def _strict(fn, *a, **kw):
    """fn(...) with every NumPy floating-point warning (0/0, x/0) an error."""
    with warnings.catch_warnings(), np.errstate(divide="raise", invalid="raise"):
        warnings.simplefilter("error", RuntimeWarning)
        return fn(*a, **kw)


@pytest.mark.parametrize("name", [n for n in init_names() if load_init(n)["kwargs"]["init"] != "random"])
def test_algebra_reproduces_golden(name):
    case = load_init(name)
    kw = case["kwargs"]
    X = case["X"]
    W, H = _strict(nndsvd_numpy, X, kw["n_components"], init=kw["init"] or "nndsvda",
                   random_state=kw["random_state"])
    assert W.dtype == case["W"].dtype and H.dtype == case["H"].dtype
    tol = 1e-8 if X.dtype == np.float64 else 2e-5
    ew, eh = rel_fro(W, case["W"]), rel_fro(H, case["H"])
    print(f"{name}: rel W {ew:.2e} rel H {eh:.2e}")
    np.testing.assert_array_equal(W == 0, case["W"] == 0)
    np.testing.assert_array_equal(H == 0, case["H"] == 0)
    assert ew <= tol and eh <= tol, (ew, eh)


@pytest.mark.parametrize("init", ["nndsvd", "nndsvda", "nndsvdar"])
def test_rank_deficient_x(init):
    X = rank2_x()
    W, H = _strict(nndsvd_numpy, X, 4, init=init, random_state=0)
    Wh, Hh = initialize_nmf(X, 4, init=init, random_state=0)
    assert W.dtype == np.float64 and H.dtype == np.float64
    check_rank2(W, H, Wh, Hh, X, init)
    if init == "nndsvda":  # the host restatement arrives at the same fill from its noise-level components
        assert np.all(Wh[:, 2:] == X.mean()) and np.all(Hh[2:] == X.mean())


@pytest.mark.parametrize("init", ["nndsvd", "nndsvda", "nndsvdar"])
def test_all_zero_x(init):
    X = np.zeros((100, 5))
    W, H = _strict(nndsvd_numpy, X, 2, init=init, random_state=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # sklearn's own arithmetic on a zero matrix
        Wh, Hh = initialize_nmf(X, 2, init=init, random_state=0)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    assert np.array_equal(W, Wh) and np.array_equal(H, Hh)


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_shape_matches_host(name):
    X, k, kind, bar = edge_cases()[name]
    np_dt = np.float64 if kind == "f64" else np.float32
    for init in ("nndsvd", "nndsvda"):
        W, H = _strict(nndsvd_numpy, X, k, init=init, random_state=0, np_dt=np_dt)
        Wh, Hh = edge_host(name, init)
        assert W.dtype == np_dt and H.dtype == np_dt and W.shape == Wh.shape and H.shape == Hh.shape
        ew, eh = rel_fro(W, Wh), rel_fro(H, Hh)
        fill_h = 0.0 if init == "nndsvd" else X.astype(np.float64).mean()
        fill = np_dt(0.0) if init == "nndsvd" else np_dt(NumpyPasses(X).gram()[1].sum() / X.size)
        bad = int(((W == fill) != (Wh == fill_h)).sum() + ((H == fill) != (Hh == fill_h)).sum())
        print(f"{name} {init}: rel W {ew:.2e} rel H {eh:.2e} fill-pattern mismatches {bad}")
        assert bad == 0
        assert ew <= bar and eh <= bar, (ew, eh)


def test_combine_stats_picks_first_row_of_largest_abs():
    """_combine_stats over the block rows of NumpyPasses.stats against np.argmax(abs(u)) on the whole
    column: equal |u| of opposite signs in one block and in two blocks (the lower row wins), an
    all-zero column, an all-negative column, the maximum in the last row."""
    rs = np.random.RandomState(11)
    N, k = 8200, 6
    U = rs.uniform(-1, 1, size=(N, k))
    U[[5, 261, 5000], 0] = [-3.0, 3.0, 3.0]
    U[[5000, 8199], 1] = [3.0, -3.0]
    U[:, 2] = 0.0
    U[:, 3] = -np.abs(U[:, 3])
    U[N - 1, 4] = 5.0
    st = NumpyPasses(np.zeros((N, 1))).stats(U)
    assert st.shape[0] == 3
    sp, sn, best, val, row = _combine_stats(st)
    rsp, rsn, rbest, rval, rrow = stats_ref(U)
    assert np.array_equal(best, rbest) and np.array_equal(val, rval) and np.array_equal(row, rrow)
    assert list(row[:5]) == [5, 5000, 0, int(np.argmax(np.abs(U[:, 3]))), N - 1] and val[0] == -3.0 and val[1] == 3.0
    assert np.allclose(sp, rsp.astype(np.float64), rtol=1e-12, atol=0)
    assert np.allclose(sn, rsn.astype(np.float64), rtol=1e-12, atol=0)
    # the order of the rows must not matter to the tie rule
    sp2, sn2, best2, val2, row2 = _combine_stats(st[::-1])
    assert np.array_equal(val2, val) and np.array_equal(row2, row)
