"""MiniBatchNMF without a GPU: parameter validation (sklearn's messages), the refusals, the
exports, and the cnmf_mb_* part of the C ABI (sizing helpers and argument checks run before any
device work)."""
import numpy as np
import pytest

import cnmf
import cnmf_amd
from cnmf_amd import _lib
from cnmf_amd.minibatch import MiniBatchNMF

X = np.abs(np.random.RandomState(0).randn(12, 6))


@pytest.mark.parametrize("params, message", [
    (dict(n_components=0), "The 'n_components' parameter must be an int in the range [1, inf), None or 'auto'. Got 0 instead."),
    (dict(init="spam"), "The 'init' parameter must be a str among"),
    (dict(batch_size=0), "The 'batch_size' parameter must be an int in the range [1, inf). Got 0 instead."),
    (dict(batch_size=2.5), "The 'batch_size' parameter must be an int in the range [1, inf). Got 2.5 instead."),
    (dict(tol=-1.0), "The 'tol' parameter must be a float in the range [0, inf). Got -1.0 instead."),
    (dict(max_no_improvement=0), "The 'max_no_improvement' parameter must be an int in the range [1, inf) or None. Got 0 instead."),
    (dict(max_iter=0), "The 'max_iter' parameter must be an int in the range [1, inf). Got 0 instead."),
    (dict(alpha_W=-1.0), "The 'alpha_W' parameter must be a float in the range [0, inf). Got -1.0 instead."),
    (dict(alpha_H="spam"), "The 'alpha_H' parameter must be a float in the range [0, inf) or a str among {'same'}. Got 'spam' instead."),
    (dict(l1_ratio=2.0), "The 'l1_ratio' parameter must be a float in the range [0, 1]. Got 2.0 instead."),
    (dict(forget_factor=1.5), "The 'forget_factor' parameter must be a float in the range [0.0, 1.0]. Got 1.5 instead."),
    (dict(fresh_restarts="yes"), "The 'fresh_restarts' parameter must be an instance of 'bool' or an instance of 'numpy.bool_'. Got 'yes' instead."),
    (dict(fresh_restarts_max_iter=0), "The 'fresh_restarts_max_iter' parameter must be an int in the range [1, inf). Got 0 instead."),
    (dict(transform_max_iter=0), "The 'transform_max_iter' parameter must be an int in the range [1, inf) or None. Got 0 instead."),
    (dict(beta_loss="kullback-leibler"), "beta_loss='kullback-leibler' is not available"),
    (dict(fresh_restarts=True), "fresh_restarts=True is not available yet"),
])
def test_invalid_parameters(params, message):
    est = MiniBatchNMF(**{"n_components": 2, **params})
    for call in (est.fit, est.fit_transform, est.partial_fit):
        with pytest.raises(ValueError) as e:
            call(X)
        assert message in str(e.value)


def test_invalid_inputs():
    with pytest.raises(ValueError, match="Negative values in data passed to MiniBatchNMF"):
        MiniBatchNMF(n_components=2).fit(-X)
    with pytest.raises(ValueError, match="contains NaN"):
        MiniBatchNMF(n_components=2).fit(np.where(X > 1, np.nan, X))
    with pytest.raises(ValueError, match="Expected 2D array"):
        MiniBatchNMF(n_components=2).fit(X[0])
    with pytest.raises(ValueError, match="must be provided when init='custom'"):
        MiniBatchNMF(n_components=2, init="custom").fit(X)
    with pytest.raises(ValueError, match="wrong first dimension"):
        MiniBatchNMF(n_components=2, init="custom").fit(X, W=np.ones((12, 2)), H=np.ones((3, 6)))
    with pytest.raises(TypeError, match="same dtype as X"):
        MiniBatchNMF(n_components=2, init="custom").fit(X, W=np.ones((12, 2), np.float32), H=np.ones((2, 6)))
    with pytest.raises(ValueError, match="n_components=17 is not supported"):
        MiniBatchNMF(n_components=17, init="random").fit(np.ones((20, 20)))
    with pytest.raises(ValueError, match="handles 1..512"):
        MiniBatchNMF(n_components=2).fit(np.ones((2, 513)))


@pytest.mark.parametrize("option", [dict(weights=np.ones_like(X)), dict(solver="als"), dict(memory_budget=1 << 20),
                                    dict(devices=[0, 1]), dict(group=object()), dict(normalise="l2"),
                                    dict(sum_to_one=1.0), dict(smoothness=0.5)])
def test_refusals(option):
    name = next(iter(option))
    with pytest.raises(ValueError, match=f"{name}=.* is not available for MiniBatchNMF"):
        MiniBatchNMF(n_components=2, **option)
    with pytest.raises(ValueError, match=f"{name}=.* is not available for MiniBatchNMF"):
        MiniBatchNMF(n_components=2).fit(X, **option)
    with pytest.raises(ValueError, match=f"{name}=.* is not available for MiniBatchNMF"):
        MiniBatchNMF(n_components=2).partial_fit(X, **option)


def test_bf16_and_unknown_options_are_refused():
    import torch
    with pytest.raises(TypeError, match="bfloat16 is not available"):
        MiniBatchNMF(n_components=2).fit(torch.ones(4, 3, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="unexpected keyword argument 'spam'"):
        MiniBatchNMF(spam=1)
    assert MiniBatchNMF(solver="mu").get_params()["batch_size"] == 1024


def test_not_fitted():
    est = MiniBatchNMF(n_components=2)
    with pytest.raises(ValueError, match="This MiniBatchNMF instance is not fitted yet"):
        est.transform(X)
    with pytest.raises(ValueError, match="not fitted yet"):
        est.inverse_transform(np.ones((3, 2)))


def test_params_round_trip():
    est = MiniBatchNMF(n_components=3, batch_size=64, forget_factor=0.5)
    p = est.get_params()
    assert (p["n_components"], p["batch_size"], p["forget_factor"], p["tol"], p["max_no_improvement"]) == (3, 64, 0.5, 1e-4, 10)
    assert list(p) == ["n_components", "init", "batch_size", "beta_loss", "tol", "max_no_improvement", "max_iter",
                       "alpha_W", "alpha_H", "l1_ratio", "forget_factor", "fresh_restarts", "fresh_restarts_max_iter",
                       "transform_max_iter", "random_state", "verbose", "device"]
    assert est.set_params(tol=0.0, max_no_improvement=None) is est and est.tol == 0.0
    with pytest.raises(ValueError, match="Invalid parameter 'spam'"):
        est.set_params(spam=1)


def test_exports():
    assert cnmf.MiniBatchNMF is cnmf_amd.MiniBatchNMF is MiniBatchNMF
    assert "MiniBatchNMF" in cnmf_amd.__all__ and "MiniBatchNMF" in cnmf.__all__


NEW_SYMBOLS = ["cnmf_mb_rows", "cnmf_mb_row_doubles", "cnmf_mb_ctl_doubles", "cnmf_mb_step", "cnmf_mb_solve_w"]


def test_library_exports_the_minibatch_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert lib.cnmf_abi_version() == 303


def test_sizing_helpers_answer_without_a_gpu():
    lib = _lib.load()
    assert lib.cnmf_mb_rows(0) == 0 and lib.cnmf_mb_rows(1) == 1 and lib.cnmf_mb_rows(64) == 1
    assert lib.cnmf_mb_rows(65) == 2 and lib.cnmf_mb_rows(1024) == 16
    for n in (65536 + 37, 10 ** 6, 10 ** 7, 2 ** 31 + 5):
        assert 1 <= lib.cnmf_mb_rows(n) <= 256
    # [A (k·F) | B (k·k) | Σx² | Σw | Σw²], rows of whole 16-byte chunks
    assert lib.cnmf_mb_row_doubles(81, 4) == 344 and lib.cnmf_mb_row_doubles(81, 5) == 434
    assert lib.cnmf_mb_row_doubles(17, 3) == 64 and lib.cnmf_mb_row_doubles(512, 16) == 8452
    assert lib.cnmf_mb_row_doubles(513, 4) == -3 and lib.cnmf_mb_row_doubles(81, 17) == -3
    assert lib.cnmf_mb_row_doubles(0, 4) == -2
    assert lib.cnmf_mb_ctl_doubles(0) == 32 and lib.cnmf_mb_ctl_doubles(100) == 332
    assert lib.cnmf_mb_ctl_doubles(-1) == -1


def test_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences
    step = lambda X=p, W=p, ctl=p, n=100, F=81, k=4, flags=3: lib.cnmf_mb_step(  # noqa: E731
        X, 0, W, p, p, p, p, p, p, 256, p, ctl, n, F, k, 0.0, 0.0, 0.0, 0.0, flags, None)
    solve = lambda X=p, W=p, n=100, F=81, k=4: lib.cnmf_mb_solve_w(  # noqa: E731
        X, 0, W, p, p, p, 256, p, p, n, F, k, 0.0, 0.0, None)
    for call in (step, solve):
        assert call(X=None) == -1 and b"null" in lib.cnmf_last_error()
        assert call(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
        assert call(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
        assert call(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
        assert call(W=p + 8) == -4
        assert call(n=0) == -2
    assert step(ctl=None) == -1
    assert step(flags=8) == -1 and b"flags" in lib.cnmf_last_error()
    assert lib.cnmf_mb_step(p, 2, p, p, p, p, p, p, p, 256, p, p, 100, 81, 4, 0.0, 0.0, 0.0, 0.0, 3, None) == -1  # bf16
    assert lib.cnmf_mb_step(p, 0, p, p, p, p, p, p, p, 1, p, p, 1000, 81, 4, 0.0, 0.0, 0.0, 0.0, 3, None) == -1
    assert b"partials hold 1 rows" in lib.cnmf_last_error()
