"""solver='whals' without a GPU: parameter validation, the refusals (each raised before any device
work, each naming 'whals'), what stays refused for 'hals', and the cnmf_whals_* part of the C ABI
(sizing helpers and argument checks run before any device work)."""
import numpy as np
import pytest

import cnmf_amd
from cnmf_amd import _lib
from cnmf_amd import api

X = np.abs(np.random.RandomState(0).randn(12, 6))
M = np.ones_like(X)


def test_whals_passes_parameter_validation():
    api._validate_params(4, None, "whals", "frobenius", 1e-4, 200, 0.0, "same", 0.0)
    api._validate_params(4, "custom", "whals", 2, 0.0, 1, 0.1, 0.2, 0.5)
    api._validate_hals("whals", False)
    cnmf_amd.NMF(n_components=2, solver="whals", alpha_W=0.1, l1_ratio=0.5)._validate()
    for init in (None, "random", "nndsvd", "nndsvda", "nndsvdar", "custom"):  # the weighted MU's starts
        api._validate_params(2, init, "whals", "frobenius", 1e-4, 200, 0.0, "same", 0.0)
    Mw = api._validate_weights(M.astype(np.float32), X, "whals", 0.1, 0.2, None)  # alpha is accepted
    assert Mw.shape == X.shape


def test_unknown_solver_message_names_every_solver():
    with pytest.raises(ValueError) as e:
        cnmf_amd.factorise(X, n_components=2, solver="cd")
    msg = str(e.value)
    assert "solver='cd' is not available" in msg and "multiplicative-update solver ('mu')" in msg
    assert "constrained ALS ('als')" in msg and "HALS ('hals')" in msg and "('whals')" in msg


def test_weights_are_required_and_validated():
    with pytest.raises(ValueError, match=r"solver='whals' needs weights=.*solver='hals'"):
        cnmf_amd.factorise(X, n_components=2, solver="whals", init="random", random_state=0)
    with pytest.raises(ValueError, match=r"solver='whals' needs weights="):
        cnmf_amd.NMF(n_components=2, solver="whals", init="random").fit(X)
    with pytest.raises(ValueError, match=r"weights must have X's shape \(12, 6\), got \(12, 5\)"):
        cnmf_amd.factorise(X, n_components=2, solver="whals", init="random", weights=M[:, :5])
    with pytest.raises(ValueError, match="Negative values in data passed to NMF \\(input weights\\)"):
        cnmf_amd.factorise(X, n_components=2, solver="whals", init="random", weights=-M)
    bad = M.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        cnmf_amd.factorise(X, n_components=2, solver="whals", init="random", weights=bad)


@pytest.mark.parametrize("options, message", [
    (dict(shuffle=True), "shuffle=True is not available for solver='whals'"),
    (dict(devices=[0, 1]), "devices= is not available for solver='whals'"),
    (dict(memory_budget=64), "a memory_budget that streams X is not available for solver='whals'"),
    (dict(normalise="l2"), "normalise is not available for solver='whals'"),
    (dict(sum_to_one=1.0), "sum_to_one / smoothness are not available for solver='whals'"),
    (dict(smoothness=0.5), "sum_to_one / smoothness are not available for solver='whals'"),
    (dict(init="spa"), "init='spa' is not available with weights="),
    (dict(n_components=9), "solver='whals' does not serve n_components k=9 with n_features F=6"),
])
def test_refusals(options, message):
    kw = dict(n_components=2, solver="whals", init="random", random_state=0, weights=M)
    kw.update(options)
    with pytest.raises(ValueError) as e:
        cnmf_amd.factorise(X, **kw)
    assert message in str(e.value)


def test_shapes_outside_the_envelope_name_k_and_f():
    from cnmf_amd.solver import whals_row_doubles
    assert whals_row_doubles(81, 4) == 1136
    for F, k in ((513, 4), (193, 5), (81, 9)):
        with pytest.raises(ValueError, match=rf"k={k} with n_features F={F}"):
            whals_row_doubles(F, k)
    Xw = np.ones((6, 193))
    with pytest.raises(ValueError, match="k=5 with n_features F=193"):
        cnmf_amd.factorise(Xw, n_components=5, solver="whals", init="random", random_state=0, weights=np.ones_like(Xw))


def test_sharded_fits_are_refused():
    from cnmf_amd.distributed import factorise_sharded
    with pytest.raises(ValueError, match="solver='whals' is not available for a sharded fit"):
        factorise_sharded(X, None, None, solver="whals", weights=M)
    with pytest.raises(ValueError, match=r"solver='whals' is not available for a sharded fit \(group=\)"):
        api._resolve(X, None, None, 2, "random", True, 0.0, "same", 0.0, 0, None, group=object(), solver="whals",
                     weights=M)


def test_estimator_refusals():
    with pytest.raises(ValueError, match="shuffle=True is not available for solver='whals'"):
        cnmf_amd.NMF(n_components=2, solver="whals", shuffle=True).fit(X, weights=M)
    with pytest.raises(ValueError, match="normalise is not available for solver='whals'"):
        cnmf_amd.NMF(n_components=2, solver="whals", init="random", normalise="l1").fit(X, weights=M)
    with pytest.raises(ValueError, match="memory_budget that streams X is not available for solver='whals'"):
        cnmf_amd.NMF(n_components=2, solver="whals", init="random", memory_budget=64).fit(X, weights=M)
    with pytest.raises(ValueError, match="not available for solver='whals'"):
        cnmf_amd.NMF(n_components=2, solver="whals", smoothness=1.0).fit(X, weights=M)


def test_bf16_is_refused():
    import torch
    Xb = torch.ones(4, 3, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bfloat16 X is not available for solver='whals'"):
        cnmf_amd.factorise(Xb, n_components=2, solver="whals", init="random", weights=torch.ones(4, 3))
    with pytest.raises(TypeError, match="bfloat16 X is not available for solver='whals'"):
        cnmf_amd.NMF(n_components=2, solver="whals", init="random").fit(Xb, weights=torch.ones(4, 3))


def test_weights_with_hals_and_als_stay_refused_with_their_text():
    for solver in ("hals", "als"):
        with pytest.raises(ValueError) as e:
            cnmf_amd.factorise(X, n_components=2, solver=solver, init="random", random_state=0, weights=M)
        assert str(e.value) == "weights apply to solver='mu' only"
    with pytest.raises(ValueError, match="weights apply to solver='mu' only"):
        cnmf_amd.NMF(n_components=2, solver="hals", init="random").fit_transform(X, weights=M)
    with pytest.raises(ValueError, match="shuffle=True is not available for solver='hals': the sweep visits"):
        cnmf_amd.factorise(X, n_components=2, solver="hals", shuffle=True)
    with pytest.raises(ValueError, match="devices= is not available for solver='hals': it runs on one device."):
        cnmf_amd.factorise(X, n_components=2, solver="hals", devices=[0, 1])


def test_params_round_trip():
    est = cnmf_amd.NMF(n_components=3, solver="whals", alpha_W=0.01, alpha_H=0.02, l1_ratio=0.5, tol=1e-5)
    p = est.get_params()
    assert (p["solver"], p["alpha_W"], p["alpha_H"], p["l1_ratio"], p["tol"], p["shuffle"]) == \
        ("whals", 0.01, 0.02, 0.5, 1e-5, False)
    clone = cnmf_amd.NMF(**p)
    assert clone.get_params() == p
    assert est.set_params(solver="hals") is est and est.solver == "hals"


NEW_SYMBOLS = ["cnmf_whals_rows", "cnmf_whals_row_doubles", "cnmf_whals_step", "cnmf_whals_loss"]


def test_library_exports_the_whals_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert lib.cnmf_abi_version() == 303  # the entry points only add symbols


def test_sizing_helpers_answer_without_a_gpu():
    lib = _lib.load()
    assert lib.cnmf_whals_rows(0) == 0 and lib.cnmf_whals_rows(1) == 1 and lib.cnmf_whals_rows(64) == 1
    assert lib.cnmf_whals_rows(65) == 2 and lib.cnmf_whals_rows(32805) == 171
    for n in (10 ** 6, 10 ** 7, 2 ** 31 + 5):
        assert 1 <= lib.cnmf_whals_rows(n) <= 256
    # [A (k·F) | S (F·k(k+1)/2) | Σ|pg|], padded to whole 16-byte chunks
    assert lib.cnmf_whals_row_doubles(81, 4) == 1136 and lib.cnmf_whals_row_doubles(81, 8) == 3566
    assert lib.cnmf_whals_row_doubles(1, 1) == 4
    assert lib.cnmf_whals_row_doubles(512, 4) == 7170 and lib.cnmf_whals_row_doubles(128, 8) == 5634
    assert lib.cnmf_whals_row_doubles(192, 8) == 8450 and lib.cnmf_whals_row_doubles(192, 5) == 3842
    assert lib.cnmf_whals_row_doubles(0, 4) == -2 and lib.cnmf_whals_row_doubles(81, 0) == -2
    assert lib.cnmf_whals_row_doubles(513, 4) == -3 and lib.cnmf_whals_row_doubles(193, 5) == -3
    assert lib.cnmf_whals_row_doubles(81, 9) == -3 and b"k=9" in lib.cnmf_last_error()


def test_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences

    def step(X=p, M=p, dt=0, W=p, H64=p, Ht=p, parts=p, n_parts=256, counter=p, ctl=p, n=100, F=81, k=4, flags=1):
        return lib.cnmf_whals_step(X, M, dt, W, H64, Ht, parts, n_parts, counter, ctl, n, F, k, 0.0, 0.0, 0.0, 0.0,
                                   flags, None)

    for name in ("X", "M", "W", "H64", "Ht", "parts", "counter", "ctl"):
        assert step(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert step(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert step(k=9) == -3 and b"k=9" in lib.cnmf_last_error()
    assert step(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert step(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert step(F=193, k=5) == -3 and b"n_features=193" in lib.cnmf_last_error()
    assert step(n=0) == -2
    assert step(dt=2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert step(dt=9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()
    assert step(flags=2) == -1 and b"flags" in lib.cnmf_last_error()
    assert step(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
    assert step(M=p + 4) == -4 and b"M must be 16-byte aligned" in lib.cnmf_last_error()
    assert step(W=p + 8) == -4
    assert step(n=1000, n_parts=1) == -1 and b"partials hold 1 rows" in lib.cnmf_last_error()

    def loss(X=p, M=p, dt=0, W=p, H64=p, parts=p, n_parts=256, counter=p, out=p, n=100, F=81, k=4):
        return lib.cnmf_whals_loss(X, M, dt, W, H64, parts, n_parts, counter, out, n, F, k, None)

    for name in ("X", "M", "W", "H64", "parts", "counter", "out"):
        assert loss(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert (loss(k=0), loss(k=9), loss(F=0), loss(F=513), loss(dt=2), loss(dt=9)) == (-2, -3, -2, -3, -1, -1)
    assert loss(X=p + 4) == -4 and loss(M=p + 8) == -4 and loss(n=1000, n_parts=1) == -1
