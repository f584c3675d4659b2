"""The sharded form of solver='hals' without a GPU: the two entry points it adds to the C ABI
(cnmf_hals_shard_step, cnmf_hals_basis: declared, bound, exported, their argument checks answered
before any device work) and the refusals of factorise_sharded(solver='hals')."""
import numpy as np
import pytest

from cnmf_amd import _lib

NEW_SYMBOLS = ["cnmf_hals_shard_step", "cnmf_hals_basis"]


def test_library_exports_the_sharded_hals_symbols():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._SIGS and hasattr(lib, s), s
    assert len(_lib._SIGS["cnmf_hals_shard_step"][1]) == 16 and len(_lib._SIGS["cnmf_hals_basis"][1]) == 11
    assert lib.cnmf_abi_version() == 303  # the entry points only add symbols


def test_shard_step_argument_checks_return_status():
    lib = _lib.load()
    p = 4096  # a non-null, 16-byte aligned address that no check dereferences

    def step(X=p, dt=0, W=p, Ht=p, HHt=p, parts=p, n_parts=256, counter=p, ctl=p, acc=p, n=100, F=81, k=4):
        return lib.cnmf_hals_shard_step(X, dt, W, Ht, HHt, parts, n_parts, counter, ctl, acc, n, F, k, 0.0, 0.0, None)

    for name in ("X", "W", "Ht", "HHt", "parts", "counter", "ctl", "acc"):
        assert step(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert step(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert step(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
    assert step(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert step(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert step(n=0) == -2
    assert step(dt=2) == -1 and b"bf16" in lib.cnmf_last_error()
    assert step(dt=9) == -1 and b"x_dtype 9" in lib.cnmf_last_error()
    assert step(X=p + 4) == -4 and b"aligned" in lib.cnmf_last_error()
    assert step(W=p + 8) == -4
    assert step(acc=p + 8) == -4 and b"acc must be 16-byte aligned" in lib.cnmf_last_error()
    assert step(n=1000, n_parts=1) == -1 and b"partials hold 1 rows" in lib.cnmf_last_error()


def test_basis_argument_checks_return_status():
    lib = _lib.load()
    p = 4096

    def basis(acc=p, H64=p, Ht=p, HHt=p, ctl=p, F=81, k=4, flags=1):
        return lib.cnmf_hals_basis(acc, H64, Ht, HHt, ctl, F, k, 0.0, 0.0, flags, None)

    for name in ("acc", "H64", "Ht", "HHt", "ctl"):
        assert basis(**{name: None}) == -1 and b"null" in lib.cnmf_last_error(), name
    assert basis(k=0) == -2 and b"k=0" in lib.cnmf_last_error()
    assert basis(k=17) == -3 and b"k=17" in lib.cnmf_last_error()
    assert basis(F=0) == -2 and b"F=0" in lib.cnmf_last_error()
    assert basis(F=513) == -3 and b"n_features=513" in lib.cnmf_last_error()
    assert basis(flags=2) == -1 and b"flags" in lib.cnmf_last_error()
    assert basis(flags=3) == -1
    assert basis(acc=p + 8) == -4 and b"acc must be 16-byte aligned" in lib.cnmf_last_error()


X = np.abs(np.random.RandomState(0).randn(12, 6))
W0 = np.abs(np.random.RandomState(1).randn(12, 2))
H0 = np.abs(np.random.RandomState(2).randn(2, 6))


@pytest.mark.parametrize("options, error, message", [
    (dict(weights=np.ones_like(X)), ValueError, "weights apply to solver='mu' only"),
    (dict(sum_to_one=1.0), ValueError, "sum_to_one / smoothness apply to solver='als' only"),
    (dict(smoothness=0.5), ValueError, "sum_to_one / smoothness apply to solver='als' only"),
])
def test_factorise_sharded_refusals(options, error, message):
    """Raised from the arguments alone: before the process group or a device is looked at."""
    from cnmf_amd.distributed import factorise_sharded
    with pytest.raises(error) as e:
        factorise_sharded(X, W0, H0, solver="hals", **options)
    assert message in str(e.value)


def test_factorise_sharded_refuses_bf16_and_unknown_solvers():
    import torch
    from cnmf_amd.distributed import factorise_sharded
    with pytest.raises(TypeError, match="bfloat16 X is not available for solver='hals'"):
        factorise_sharded(torch.ones(4, 3, dtype=torch.bfloat16), None, H0[:, :3], solver="hals")
    with pytest.raises(ValueError, match="W_shard=None is the update_H=False start"):
        factorise_sharded(X, None, H0, solver="hals")
    with pytest.raises(ValueError, match="solver must be 'mu', 'als' or 'hals', got 'cd'"):
        factorise_sharded(X, W0, H0, solver="cd")
    # accepted as a solver: the next check is the one every sharded fit makes
    with pytest.raises(RuntimeError, match="needs an initialised torch.distributed process group"):
        factorise_sharded(X, W0, H0, solver="hals")


def test_plan_signature_takes_a_group_and_split():
    import inspect
    from cnmf_amd.solver import HALSPlan
    params = inspect.signature(HALSPlan.__init__).parameters
    assert params["split"].default is False and params["group"].default is None
