"""solver='hals' without a GPU: the refusals (each raised before any device work), parameter
validation, and the cnmf_hals_* part of the C ABI (sizing helpers and argument checks run before
any device work)."""
import numpy as np
import pytest

import cnmf_amd
from cnmf_amd import _lib
from cnmf_amd import api

X = np.abs(np.random.RandomState(0).randn(12, 6))


def test_hals_passes_parameter_validation():
    api._validate_params(4, None, "hals", "frobenius", 1e-4, 200, 0.0, "same", 0.0)
    api._validate_params(4, "custom", "hals", 2, 0.0, 1, 0.1, 0.2, 0.5)
    api._validate_hals("hals", False)
    api._validate_hals("mu", True, devices=[0])  # only 'hals' is concerned
    cnmf_amd.NMF(n_components=2, solver="hals", alpha_W=0.1, l1_ratio=0.5)._validate()


def test_cd_is_still_refused_with_its_message():
    for call in (lambda: cnmf_amd.factorise(X, n_components=2, solver="cd"),
                 lambda: cnmf_amd.NMF(n_components=2, solver="cd").fit(X)):
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert "solver='cd' is not available" in msg and "multiplicative-update solver ('mu')" in msg
        assert "constrained ALS ('als')" in msg and "HALS ('hals')" in msg
    with pytest.raises(ValueError, match="beta_loss='kullback-leibler' is not available"):
        cnmf_amd.factorise(X, n_components=2, solver="hals", beta_loss="kullback-leibler")


@pytest.mark.parametrize("options, error, message", [
    (dict(shuffle=True), ValueError, "is not available for solver='hals'"),
    (dict(weights=np.ones_like(X)), ValueError, "weights apply to solver='mu' only"),
    (dict(memory_budget=64), ValueError, "memory_budget (out-of-core streaming) serves the unweighted 'mu' solver"),
    (dict(devices=[0, 1]), ValueError, "devices= is not available for solver='hals'"),
    (dict(sum_to_one=1.0), ValueError, "solver='als' only"),
    (dict(smoothness=0.5), ValueError, "solver='als' only"),
])
def test_refusals(options, error, message):
    with pytest.raises(error) as e:
        cnmf_amd.factorise(X, n_components=2, solver="hals", init="random", random_state=0, **options)
    assert message in str(e.value)


def test_estimator_refusals():
    with pytest.raises(ValueError, match="shuffle=True is not available for solver='hals'"):
        cnmf_amd.NMF(n_components=2, solver="hals", shuffle=True).fit(X)
    with pytest.raises(ValueError, match="weights apply to solver='mu' only"):
        cnmf_amd.NMF(n_components=2, solver="hals", init="random").fit_transform(X, weights=np.ones_like(X))
    with pytest.raises(ValueError, match="solver='als' only"):
        cnmf_amd.NMF(n_components=2, solver="hals", smoothness=1.0).fit(X)
    with pytest.raises(ValueError, match="memory_budget"):
        cnmf_amd.NMF(n_components=2, solver="hals", init="random", memory_budget=64).fit(X)


def test_bf16_is_refused():
    import torch
    with pytest.raises(TypeError, match="bfloat16 X is not available for solver='hals'"):
        cnmf_amd.factorise(torch.ones(4, 3, dtype=torch.bfloat16), n_components=2, solver="hals", init="random")
    with pytest.raises(TypeError, match="bfloat16 X is not available for solver='hals'"):
        cnmf_amd.NMF(n_components=2, solver="hals", init="random").fit(torch.ones(4, 3, dtype=torch.bfloat16))


def test_params_round_trip():
    est = cnmf_amd.NMF(n_components=3, solver="hals", alpha_W=0.01, alpha_H=0.02, l1_ratio=0.5, tol=1e-5)
    p = est.get_params()
    assert (p["solver"], p["alpha_W"], p["alpha_H"], p["l1_ratio"], p["tol"], p["shuffle"]) == \
        ("hals", 0.01, 0.02, 0.5, 1e-5, False)
    clone = cnmf_amd.NMF(**p)
    assert clone.get_params() == p
    assert est.set_params(solver="mu") is est and est.solver == "mu"


NEW_SYMBOLS = ["cnmf_hals_rows", "cnmf_hals_row_doubles", "cnmf_hals_ctl_doubles", "cnmf_hals_step",
               "cnmf_hals_loss"]


def test_library_exports_the_hals_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert lib.cnmf_abi_version() == 303  # the entry points only add symbols


def test_slots_match_the_header():
    from cnmf_amd import solver
    with open(_lib.header_path()) as f:
        text = f.read()
    for name, value in (("STOPPED", 0), ("ITERS_DONE", 1), ("VIOL_INIT", 2), ("VIOL_LAST", 3), ("TOL", 4),
                        ("LOG_CAP", 5), ("NLOG", 6), ("LOG", 16)):
        assert f"CNMF_HALS_{name} = {value}" in text
        assert getattr(solver, f"HALS_{name}") == value
    assert "CNMF_HALS_UPDATE_H = 1" in text and solver.HALS_UPDATE_H == 1 and solver.HALS_STRETCH == 16


def test_sizing_helpers_answer_without_a_gpu():
    lib = _lib.load()
    assert lib.cnmf_hals_rows(0) == 0 and lib.cnmf_hals_rows(1) == 1 and lib.cnmf_hals_rows(64) == 1
    assert lib.cnmf_hals_rows(65) == 2 and lib.cnmf_hals_rows(1024) == 16
    assert lib.cnmf_hals_rows(64 * 2 * 256 + 37) == 171  # 192 rows per workgroup: three tiles each
    for n in (65536 + 37, 10 ** 6, 10 ** 7, 2 ** 31 + 5):
        assert 1 <= lib.cnmf_hals_rows(n) <= 256
    # [A (k·F) | B (k·k) | Σ|pg|], padded to whole 16-byte chunks
    assert lib.cnmf_hals_row_doubles(81, 4) == 342 and lib.cnmf_hals_row_doubles(81, 5) == 432
    assert lib.cnmf_hals_row_doubles(17, 3) == 62 and lib.cnmf_hals_row_doubles(512, 16) == 8450
    assert lib.cnmf_hals_row_doubles(1, 1) == 4
    assert lib.cnmf_hals_row_doubles(513, 4) == -3 and lib.cnmf_hals_row_doubles(81, 17) == -3
    assert lib.cnmf_hals_row_doubles(0, 4) == -2 and lib.cnmf_hals_row_doubles(81, 0) == -2
    assert lib.cnmf_hals_ctl_doubles(0) == 16 and lib.cnmf_hals_ctl_doubles(200) == 216
    assert lib.cnmf_hals_ctl_doubles(-1) == -1


def test_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences

    def step(X=p, dt=0, W=p, H64=p, Ht=p, HHt=p, parts=p, n_parts=256, counter=p, ctl=p, n=100, F=81, k=4, flags=1):
        return lib.cnmf_hals_step(X, dt, W, H64, Ht, HHt, parts, n_parts, counter, ctl, n, F, k, 0.0, 0.0, 0.0, 0.0,
                                  flags, None)

    for name in ("X", "W", "H64", "Ht", "HHt", "parts", "counter", "ctl"):
        assert step(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert step(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert step(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
    assert step(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert step(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert step(n=0) == -2
    assert step(dt=2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert step(dt=9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()
    assert step(flags=2) == -1 and b"flags" in lib.cnmf_last_error()
    assert step(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
    assert step(W=p + 8) == -4
    assert step(n=1000, n_parts=1) == -1 and b"partials hold 1 rows" in lib.cnmf_last_error()

    def loss(X=p, dt=0, W=p, H64=p, parts=p, n_parts=256, counter=p, out=p, n=100, F=81, k=4):
        return lib.cnmf_hals_loss(X, dt, W, H64, parts, n_parts, counter, out, n, F, k, None)

    for name in ("X", "W", "H64", "parts", "counter", "out"):
        assert loss(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert (loss(k=0), loss(k=17), loss(F=0), loss(F=513), loss(dt=2), loss(dt=9)) == (-2, -3, -2, -3, -1, -1)
    assert loss(X=p + 4) == -4 and loss(n=1000, n_parts=1) == -1
