"""factorise_multistart without a GPU: the refusals (each raised before any device work), the seed
rules, the exports, and the cnmf_ms_* part of the C ABI (sizing helpers and argument checks run
before any device work)."""
import numpy as np
import pytest

import cnmf
import cnmf_amd
from cnmf_amd import _lib
from cnmf_amd import multistart as ms

X = np.abs(np.random.RandomState(0).randn(12, 6))


@pytest.mark.parametrize("options, error, message", [
    (dict(solver="mu"), ValueError, "solver='mu' is not available for factorise_multistart"),
    (dict(solver="cd"), ValueError, "solver='cd' is not available for factorise_multistart"),
    (dict(init="nndsvd"), ValueError, "the other inits are deterministic and give one start"),
    (dict(init=None), ValueError, "the other inits are deterministic and give one start"),
    (dict(init="spa"), ValueError, "init='spa' is not available for factorise_multistart"),
    (dict(n_init=0), ValueError, "The 'n_init' parameter must be an int in the range [1, 64]. Got 0 instead."),
    (dict(n_init=65), ValueError, "The 'n_init' parameter must be an int in the range [1, 64]. Got 65 instead."),
    (dict(n_init=2.0), ValueError, "The 'n_init' parameter must be an int in the range [1, 64]"),
    (dict(n_init=True), ValueError, "The 'n_init' parameter must be an int in the range [1, 64]"),
    (dict(keep="first"), ValueError, "The 'keep' parameter must be a str among {'all', 'best'}. Got 'first' instead."),
    (dict(tol=-1.0), ValueError, "The 'tol' parameter must be a float in the range [0, inf)"),
    (dict(max_iter=0), ValueError, "The 'max_iter' parameter must be an int in the range [1, inf)"),
    (dict(alpha_W=-1.0), ValueError, "The 'alpha_W' parameter must be a float in the range [0, inf)"),
    (dict(l1_ratio=2.0), ValueError, "The 'l1_ratio' parameter must be a float in the range [0, 1]"),
    (dict(random_state=[1, 2]), ValueError, "random_state holds 2 seeds for n_init=3 starts"),
    (dict(random_state=["a", "b", "c"]), ValueError, "every seed must be an int"),
    (dict(random_state=1.5), TypeError, "random_state must be None, an int, a sequence"),
])
def test_refusals(options, error, message):
    kw = dict(n_init=3, random_state=0)
    kw.update(options)
    with pytest.raises(error) as e:
        cnmf_amd.factorise_multistart(X, 2, **kw)
    assert message in str(e.value)


def test_shape_and_dtype_refusals():
    import torch
    with pytest.raises(ValueError, match="n_components=17 is not supported: the MI355X kernels handle 1..16"):
        cnmf_amd.factorise_multistart(np.ones((40, 20)), 17, n_init=2, random_state=0)
    with pytest.raises(ValueError, match=r"n_features=513 is not supported by factorise_multistart \(1..512\)"):
        cnmf_amd.factorise_multistart(np.ones((4, 513)), 2, n_init=2, random_state=0)
    with pytest.raises(TypeError, match="bfloat16 X is not available for factorise_multistart"):
        cnmf_amd.factorise_multistart(torch.ones(4, 3, dtype=torch.bfloat16), 2, n_init=2, random_state=0)
    with pytest.raises(ValueError, match="Expected 2D array, got 1D array instead"):
        cnmf_amd.factorise_multistart(np.ones(5), 2)
    with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
        cnmf_amd.factorise_multistart(np.full((4, 3), np.nan), 2)
    with pytest.raises(ValueError, match="n_components' parameter must be an int"):
        cnmf_amd.factorise_multistart(X, 0)
    with pytest.raises(ValueError, match="Negative values in data passed to NMF"):
        cnmf_amd.factorise_multistart(-X, 2, n_init=2, random_state=0)
    with pytest.raises(TypeError):  # no parameters for weights, devices=, shuffle, update_H, normalise
        cnmf_amd.factorise_multistart(X, 2, weights=np.ones_like(X))
    for name in ("devices", "shuffle", "update_H", "normalise", "memory_budget", "group"):
        with pytest.raises(TypeError):
            cnmf_amd.factorise_multistart(X, 2, **{name: None})


def test_custom_starts_are_validated_per_slice():
    W, H = np.ones((3, 12, 2)), np.ones((3, 2, 6))
    call = lambda **kw: cnmf_amd.factorise_multistart(X, 2, init="custom", **kw)  # noqa: E731
    with pytest.raises(ValueError, match=r"NMF \(input W\) must be provided when init='custom'"):
        call(H=H)
    with pytest.raises(ValueError, match=r"takes W with one slice per start: \(R, n_samples, k\)"):
        call(W=W[0], H=H)
    with pytest.raises(ValueError, match="W holds 2 starts and H holds 3"):
        call(W=W[:2], H=H)
    with pytest.raises(ValueError, match="n_init=4 but W and H hold 3 starts"):
        call(W=W, H=H, n_init=4)
    with pytest.raises(ValueError, match="n_init=8 but W and H hold 3 starts"):  # 8 given is not 8 by default
        call(W=W, H=H, n_init=8)
    Wn = W.copy()
    Wn[2, 0, 0] = -1.0
    with pytest.raises(ValueError, match=r"Negative values in data passed to NMF \(input W\)"):
        call(W=Wn, H=H)
    Hz = H.copy()
    Hz[1] = 0.0
    with pytest.raises(ValueError, match=r"Array passed to NMF \(input H\) is full of zeros"):
        call(W=W, H=Hz)
    with pytest.raises(ValueError, match=r"Array with wrong second dimension passed to NMF \(input H\). Expected 6, but got 5"):
        call(W=W, H=H[:, :, :5])
    with pytest.raises(ValueError, match=r"Array with wrong first dimension passed to NMF \(input W\). Expected 12"):
        call(W=W[:, :11], H=H)
    with pytest.raises(TypeError, match="H and W should have the same dtype as X"):
        call(W=W.astype(np.float32), H=H.astype(np.float32))
    with pytest.raises(ValueError, match=r"The 'n_init' parameter must be an int in the range \[1, 64\]. Got 65"):
        call(W=np.ones((65, 12, 2)), H=np.ones((65, 2, 6)))


def test_seed_rules():
    assert ms._seeds(7, 4) == [7, 8, 9, 10]
    assert ms._seeds(np.int64(3), 2) == [3, 4]
    assert ms._seeds([5, 1, 9], 3) == [5, 1, 9] and ms._seeds(np.array([5, 1, 9]), 3) == [5, 1, 9]
    assert ms._seeds((2,), 1) == [2]
    drawn = ms._seeds(np.random.RandomState(11), 5)
    assert drawn == [int(s) for s in np.random.RandomState(11).randint(0, 2 ** 31 - 1, size=5)]
    assert len(set(drawn)) == 5
    np.random.seed(123)
    a = ms._seeds(None, 3)
    np.random.seed(123)
    b = ms._seeds(None, 3)
    assert a == b and a == [a[0], a[0] + 1, a[0] + 2]  # a base seed from NumPy's global state
    with pytest.raises(ValueError, match="an int seed must lie in"):
        ms._seeds(-1, 2)
    with pytest.raises(ValueError, match="every seed must be an int"):
        ms._seeds([1, 2.5], 2)


def test_one_start_goes_to_the_hals_step_in_the_product_library():
    """cnmf_ms_batch is 1 at every shape: a launch takes one start, which cnmf_ms_step hands to
    cnmf_hals_step, so the teams, the LDS and every bit are that launch's at every width."""
    lib = _lib.load()
    if "diag" in _lib.lib_path():
        pytest.skip("CNMF_HIP_LIB points at the diagnostic library")
    for dt in (_lib.F32, _lib.F64):
        for k in range(1, 17):
            for F in list(range(1, 513, 7)) + [74, 146, 147, 282, 285, 481, 484, 512]:
                assert lib.cnmf_ms_batch(F, k, dt) == 1, (F, k, dt)
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True).stdout
    assert "cnmf_ms_step" in syms and "ms_loss_kernel" in syms
    assert "ms_step_kernel" not in syms  # the batched kernel is in the diagnostic library only


def test_exports():
    for name in ("factorise_multistart", "MultiStartResult"):
        assert name in cnmf_amd.__all__ and name in cnmf.__all__
    assert cnmf.factorise_multistart is cnmf_amd.factorise_multistart is ms.factorise_multistart
    import dataclasses
    fields = [f.name for f in dataclasses.fields(cnmf_amd.MultiStartResult)]
    assert fields == ["W", "H", "n_iter", "best", "errors", "n_iters", "seeds", "W_all", "H_all"]


NEW_SYMBOLS = ["cnmf_ms_batch", "cnmf_ms_rows", "cnmf_ms_row_doubles", "cnmf_ms_ctl_doubles", "cnmf_ms_step",
               "cnmf_ms_loss"]


def test_library_exports_the_multistart_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert lib.cnmf_abi_version() == 303  # the entry points only add symbols


def test_slots_match_the_header():
    with open(_lib.header_path()) as f:
        text = f.read()
    for name, value in (("STOPPED", 0), ("ITERS_DONE", 1), ("VIOL_INIT", 2), ("VIOL_LAST", 3), ("TOL", 4),
                        ("STRIDE", 8)):
        assert f"CNMF_MS_{name} = {value}" in text
        assert getattr(ms, f"MS_{name}") == value
    assert "CNMF_MS_UPDATE_H = 1" in text and ms.MS_UPDATE_H == 1 and ms.MS_STRETCH == 16
    from cnmf_amd import solver  # the per-start words have the meanings (and order) of cnmf_hals_slots
    for name in ("STOPPED", "ITERS_DONE", "VIOL_INIT", "VIOL_LAST", "TOL"):
        assert getattr(ms, f"MS_{name}") == getattr(solver, f"HALS_{name}")


def test_sizing_helpers_answer_without_a_gpu():
    lib = _lib.load()
    assert lib.cnmf_ms_rows(0) == 0 and lib.cnmf_ms_rows(1) == 1 and lib.cnmf_ms_rows(65) == 2
    assert lib.cnmf_ms_rows(64 * 2 * 256 + 37) == 171
    for n in (1, 64, 65, 1024, 65536 + 37, 10 ** 6, 2 ** 31 + 5):
        assert lib.cnmf_ms_rows(n) == lib.cnmf_hals_rows(n)  # the step's workgroups and rows
    for F, k in ((81, 4), (81, 5), (17, 3), (512, 16), (1, 1)):
        for R in (1, 3, 8):
            assert lib.cnmf_ms_row_doubles(F, k, R) == R * lib.cnmf_hals_row_doubles(F, k)
    assert lib.cnmf_ms_row_doubles(513, 4, 1) == -3 and lib.cnmf_ms_row_doubles(81, 17, 1) == -3
    assert lib.cnmf_ms_row_doubles(81, 4, 9) == -3
    assert lib.cnmf_ms_row_doubles(0, 4, 1) == -2 and lib.cnmf_ms_row_doubles(81, 0, 1) == -2
    assert lib.cnmf_ms_row_doubles(81, 4, 0) == -2
    assert lib.cnmf_ms_ctl_doubles(1) == 8 and lib.cnmf_ms_ctl_doubles(6) == 48 and lib.cnmf_ms_ctl_doubles(0) == -1
    # a batch of at least one start on every served shape, fp32 and fp64
    for dt in (_lib.F32, _lib.F64):
        for k in range(1, 17):
            for F in (1, 5, 17, 64, 65, 81, 83, 128, 129, 256, 257, 300, 511, 512):
                rb = lib.cnmf_ms_batch(F, k, dt)
                assert 1 <= rb <= 8, (F, k, dt, rb)
    assert lib.cnmf_ms_batch(513, 4, 0) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert lib.cnmf_ms_batch(81, 17, 0) == -3 and b"k=17" in lib.cnmf_last_error()
    assert lib.cnmf_ms_batch(0, 4, 0) == -2 and lib.cnmf_ms_batch(81, 0, 1) == -2
    assert lib.cnmf_ms_batch(81, 4, 2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert lib.cnmf_ms_batch(81, 4, 9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()


def test_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences
    rb = lib.cnmf_ms_batch(81, 4, 0)

    def step(X=p, dt=0, W=p, H64=p, Ht=p, HHt=p, parts=p, n_parts=256, counter=p, ctl=p, n=100, F=81, k=4, R=1,
             flags=1):
        return lib.cnmf_ms_step(X, dt, W, H64, Ht, HHt, parts, n_parts, counter, ctl, n, F, k, R, 0.0, 0.0, 0.0, 0.0,
                                flags, None)

    for name in ("X", "W", "H64", "Ht", "HHt", "parts", "counter", "ctl"):
        assert step(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert step(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert step(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
    assert step(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert step(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert step(n=0) == -2 and step(R=0) == -2 and b"n_starts=0" in lib.cnmf_last_error()
    assert step(R=rb + 1) == -3 and b"n_starts=%d" % (rb + 1) in lib.cnmf_last_error()
    assert step(dt=2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert step(dt=9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()
    assert step(flags=2) == -1 and b"flags" in lib.cnmf_last_error()
    assert step(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
    assert step(W=p + 8) == -4
    assert step(n=1000, n_parts=1) == -1 and b"partials hold 1 rows" in lib.cnmf_last_error()

    def loss(X=p, dt=0, W=p, H64=p, parts=p, n_parts=256, counter=p, out=p, n=100, F=81, k=4, R=1):
        return lib.cnmf_ms_loss(X, dt, W, H64, parts, n_parts, counter, out, n, F, k, R, None)

    for name in ("X", "W", "H64", "parts", "counter", "out"):
        assert loss(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert (loss(k=0), loss(k=17), loss(F=0), loss(F=513), loss(dt=2), loss(dt=9)) == (-2, -3, -2, -3, -1, -1)
    assert loss(R=0) == -2 and loss(R=rb + 1) == -3
    assert loss(X=p + 4) == -4 and loss(n=1000, n_parts=1) == -1
