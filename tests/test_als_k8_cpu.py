"""The constrained ALS takes 1..8 components: api._resolve's bound (no GPU needed)."""
import numpy as np
import pytest


def _resolve_k(n_components):
    from cnmf_amd.api import _resolve
    X = np.random.default_rng(0).random((40, 12)).astype(np.float32)
    return _resolve(X, None, None, n_components, "random", True, 0.0, "same", 0.0, 0, None, solver="als")


@pytest.mark.parametrize("k", [5, 8])
def test_resolve_accepts_als_up_to_8_components(k):
    X, Mw, as_torch, streamed, kk, W, H, regs = _resolve_k(k)
    assert kk == k
    assert W.shape == (40, k) and H.shape == (k, 12)


def test_resolve_refuses_als_above_8_components():
    with pytest.raises(ValueError, match=r"1\.\.8"):
        _resolve_k(9)
