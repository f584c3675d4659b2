"""init='spa' without a GPU: the refusals (each raised before any device work), parameter validation,
the exports, and the cnmf_spa_* part of the C ABI (sizing helpers and argument checks run before any
device work)."""
import importlib

import numpy as np
import pytest

import cnmf_amd
from cnmf_amd import _lib
from cnmf_amd import api

spa_mod = importlib.import_module("cnmf_amd.spa")
X = np.abs(np.random.RandomState(0).randn(12, 6))


def test_spa_passes_parameter_validation():
    for solver in ("mu", "als", "hals"):
        api._validate_params(4, "spa", solver, "frobenius", 1e-4, 200, 0.0, "same", 0.0)
    assert "spa" in api._INITS
    cnmf_amd.NMF(n_components=2, init="spa")._validate()
    cnmf_amd.MiniBatchNMF(n_components=2, init="spa")._validate()
    with pytest.raises(ValueError) as e:
        cnmf_amd.factorise(X, n_components=2, init="vca")
    assert "'spa'" in str(e.value) and "'nndsvdar'" in str(e.value)
    api._validate_spa("nndsvda", weights=X, devices=[0], group=object(), streamed=True)  # only 'spa' is concerned


def test_exports():
    assert "spa" in cnmf_amd.__all__ and "spa_init" in cnmf_amd.__all__
    assert cnmf_amd.spa is spa_mod.spa and cnmf_amd.spa_init is spa_mod.spa_init


@pytest.mark.parametrize("options, error, message", [
    (dict(weights=np.ones((12, 6), np.float32)), ValueError, "init='spa' is not available with weights="),
    (dict(devices=[0, 1]), ValueError, "init='spa' is not available with devices="),
    (dict(memory_budget=64), ValueError, "init='spa' is not available with a memory_budget"),
    (dict(n_components=7), ValueError, "n_components=7 must be <= min(n_samples, n_features) = 6"),
])
def test_refusals(options, error, message):
    kw = dict(n_components=2, init="spa")
    kw.update(options)
    with pytest.raises(error) as e:
        cnmf_amd.factorise(X.astype(np.float32), **kw)
    assert message in str(e.value)


def test_group_is_refused():
    with pytest.raises(ValueError, match="init='spa' is not available for a sharded fit"):
        api._initial_factors(X, 2, "spa", None, None, False, object())
    with pytest.raises(ValueError, match="init='spa' is not available for a sharded fit"):
        api._fit_transform(X, None, None, 2, "spa", True, 1e-4, 10, 0.0, "same", 0.0, None, 0, None, group=object())


def test_estimator_refusals():
    with pytest.raises(ValueError, match="init='spa' is not available with weights="):
        cnmf_amd.NMF(n_components=2, init="spa").fit_transform(X.astype(np.float32),
                                                               weights=np.ones((12, 6), np.float32))
    with pytest.raises(ValueError, match="init='spa' is not available with a memory_budget"):
        cnmf_amd.NMF(n_components=2, init="spa", memory_budget=64).fit(X)
    with pytest.raises(ValueError, match="must be <= min"):
        cnmf_amd.MiniBatchNMF(n_components=7, init="spa").fit(X)


def test_bf16_is_refused():
    import torch
    Xb = torch.ones(4, 3, dtype=torch.bfloat16)
    for call in (lambda: cnmf_amd.factorise(Xb, n_components=2, init="spa"),
                 lambda: cnmf_amd.spa(Xb, 2), lambda: cnmf_amd.spa_init(Xb, 2)):
        with pytest.raises(TypeError, match="bfloat16 X is not available for init='spa'"):
            call()


def test_spa_validates_x_as_the_estimators_do():
    with pytest.raises(ValueError, match="Expected 2D array"):
        cnmf_amd.spa(np.ones(5), 1)
    with pytest.raises(ValueError, match="NaN or infinity"):
        cnmf_amd.spa(np.array([[1.0, np.nan], [1.0, 2.0]]), 1)
    with pytest.raises(ValueError, match="Negative values in data passed to SPA"):
        cnmf_amd.spa(np.array([[1.0, -1.0], [1.0, 2.0]]), 1)
    with pytest.raises(ValueError, match="must be <= min"):
        cnmf_amd.spa(X, 7)
    with pytest.raises(ValueError, match="1..16"):
        cnmf_amd.spa(np.ones((40, 40)), 17)
    with pytest.raises(ValueError, match="handles 1..512"):
        cnmf_amd.spa(np.ones((4, 513)), 2)
    with pytest.raises(ValueError, match="'normalise' parameter of spa"):
        cnmf_amd.spa(X, 2, normalise="l2")
    with pytest.raises(ValueError, match="'rank_tol'"):
        cnmf_amd.spa(X, 2, rank_tol=-1.0)
    with pytest.raises(ValueError, match="'n_components' parameter of spa"):
        cnmf_amd.spa(X, 0)


NEW_SYMBOLS = ["cnmf_spa_rows", "cnmf_spa_row_doubles", "cnmf_spa_ctl_doubles", "cnmf_spa_step", "cnmf_spa_start_w"]


def test_library_exports_the_spa_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert lib.cnmf_abi_version() == 303  # the entry points only add symbols


def test_slots_match_the_header():
    with open(_lib.header_path()) as f:
        text = f.read()
    for name, value in (("STOPPED", 0), ("STEPS_DONE", 1), ("SUM_X", 2), ("YMAX", 3), ("RANK_TOL", 4), ("IDX", 8),
                        ("RHO", 24)):
        assert f"CNMF_SPA_{name} = {value}" in text
        assert getattr(spa_mod, f"SPA_{name}") == value
    assert "CNMF_SPA_NORM_NONE = 0, CNMF_SPA_NORM_L1 = 1" in text
    assert (spa_mod.SPA_NORM_NONE, spa_mod.SPA_NORM_L1) == (0, 1)


def test_sizing_helpers_answer_without_a_gpu():
    lib = _lib.load()
    assert lib.cnmf_spa_rows(0) == 0 and lib.cnmf_spa_rows(1) == 1 and lib.cnmf_spa_rows(64) == 1
    assert lib.cnmf_spa_rows(65) == 2 and lib.cnmf_spa_rows(1024) == 16
    assert lib.cnmf_spa_rows(32805) == 171  # 192 rows per workgroup
    for n in (65536 + 37, 10 ** 6, 10 ** 7, 2 ** 31 + 5):
        assert 1 <= lib.cnmf_spa_rows(n) <= 256
    assert lib.cnmf_spa_row_doubles() == 4
    assert lib.cnmf_spa_ctl_doubles(1) == 25 and lib.cnmf_spa_ctl_doubles(16) == 40
    assert lib.cnmf_spa_ctl_doubles(0) == -2 and lib.cnmf_spa_ctl_doubles(17) == -3


def test_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences

    def step(X=p, dt=0, Q=p, parts=p, n_parts=256, counter=p, ctl=p, scores=None, n=100, F=81, k=4, j=0, norm=1):
        return lib.cnmf_spa_step(X, dt, Q, parts, n_parts, counter, ctl, scores, n, F, k, j, norm, None)

    for name in ("X", "Q", "parts", "counter", "ctl"):
        assert step(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert step(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert step(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
    assert step(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert step(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert step(n=0) == -2
    assert step(dt=2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert step(dt=9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()
    assert step(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
    assert step(j=4) == -1 and b"step j=4" in lib.cnmf_last_error()
    assert step(j=-1) == -1
    assert step(norm=2) == -1 and b"normalise 2" in lib.cnmf_last_error()
    assert step(n=1000, n_parts=1) == -1 and b"partials hold 1 rows" in lib.cnmf_last_error()

    def start(X=p, dt=0, M=p, W=p, wdt=0, n=100, F=81, k=4):
        return lib.cnmf_spa_start_w(X, dt, M, 0.5, W, wdt, n, F, k, None)

    for name in ("X", "M", "W"):
        assert start(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert (start(k=0), start(k=17), start(F=0), start(F=513), start(n=0)) == (-2, -3, -2, -3, -2)
    assert (start(dt=2), start(dt=9), start(wdt=2), start(wdt=9)) == (-1, -1, -1, -1)
    assert start(X=p + 4) == -4 and start(W=p + 8) == -4
