"""init='spa': the successive projection algorithm (SPA; Araújo et al. 2001, Gillis & Vavasis 2014)
as a start for NMF.  SPA picks k rows of X — the "purest" spectra — as H0; every pick is one
read-only pass over X on the device (cnmf_spa_step, csrc/spa.hip), the k launches enqueued back to
back with no host round trip.  The spec is tests/spa_ref.py; DESIGN.md §3.11.

    idx = cnmf_amd.spa(X, 4)                      # the picked rows, np.int64
    W0, H0 = cnmf_amd.spa_init(X, 4)              # H0 = X[idx] (zeros -> X.mean()/100),
                                                  # W0 = max(X·pinv(H0), X.mean()/100)

SPA assumes that nearly pure rows exist in X (near-separability).  It is deterministic: there is no
random state.  float32 / float64 X on one device, n_components <= min(n, F, 16), F <= 512.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check

__all__ = ["spa", "spa_init", "SPA_STOPPED", "SPA_STEPS_DONE", "SPA_SUM_X", "SPA_YMAX", "SPA_RANK_TOL", "SPA_IDX",
           "SPA_RHO", "MAX_FEATURES", "MAX_COMPONENTS"]

# control-block slots (include/cnmf_hip.h: cnmf_spa_slots) and the row scale (cnmf_spa_norm)
SPA_STOPPED, SPA_STEPS_DONE, SPA_SUM_X, SPA_YMAX, SPA_RANK_TOL = range(5)
SPA_IDX, SPA_RHO = 8, 24
SPA_NORM_NONE, SPA_NORM_L1 = 0, 1
MAX_FEATURES, MAX_COMPONENTS = 512, 16
_WHOM = "SPA (input X)"


def _norm_flag(normalise):
    if normalise not in ("l1", None):
        raise ValueError(f"The 'normalise' parameter of spa must be 'l1' or None. Got {normalise!r} instead.")
    return SPA_NORM_L1 if normalise == "l1" else SPA_NORM_NONE


def _validate(X, n_components, normalise, rank_tol):
    """Everything that can be refused before device work; returns the checked X."""
    from .api import _check_non_negative, _check_X, _is_torch, _torch
    import numbers
    _norm_flag(normalise)
    if not isinstance(rank_tol, numbers.Real) or rank_tol < 0:
        raise ValueError(f"The 'rank_tol' parameter must be a float in the range [0, inf). Got {rank_tol!r} instead.")
    if not isinstance(n_components, numbers.Integral) or isinstance(n_components, bool) or n_components < 1:
        raise ValueError(f"The 'n_components' parameter of spa must be an int in the range [1, inf). "
                         f"Got {n_components!r} instead.")
    if _is_torch(X) and X.dtype == _torch().bfloat16:
        raise TypeError("bfloat16 X is not available for init='spa': pass float32 or float64")
    X = _check_X(X)
    _check_non_negative(X, _WHOM)
    n, F = (int(s) for s in X.shape)
    if n_components > min(n, F):
        raise ValueError(f"init='spa' picks rows of X: n_components={n_components} must be <= min(n_samples, "
                         f"n_features) = {min(n, F)}.")
    if n_components > MAX_COMPONENTS:
        raise ValueError(f"n_components={n_components} is not supported: the MI355X kernels handle 1..16.")
    if F > MAX_FEATURES:
        raise ValueError(f"X has {F} features: init='spa' handles 1..{MAX_FEATURES}.")
    return X


def _to_device(X, device):
    from .api import _is_torch, _torch
    torch = _torch()
    if device is not None:
        dev = torch.device(device)
    elif _is_torch(X) and X.device.type == "cuda":
        dev = X.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    Xd = X if _is_torch(X) else torch.from_numpy(np.ascontiguousarray(X))
    return Xd.to(dev).contiguous()


class SPAState:
    """The device buffers of one selection: Q (k x F fp64), the partial rows, the ticket word and
    the control block."""

    def __init__(self, Xd, k, normalise="l1", rank_tol=1e-12, scores=False):
        from .solver import _XDT, _ptr
        import torch
        self._ptr = _ptr
        self.lib = _lib.load()
        self.X, self.k = Xd, int(k)
        self.n_rows, self.F = (int(s) for s in Xd.shape)
        self.xdt = _XDT[Xd.dtype]
        self.norm = _norm_flag(normalise)
        dev, f64 = Xd.device, torch.float64
        self.rows = int(check(self.lib.cnmf_spa_rows(self.n_rows), "cnmf_spa_rows"))
        self.Q = torch.zeros((self.k, self.F), dtype=f64, device=dev)
        self.partials = torch.empty(max(self.rows, 1) * int(self.lib.cnmf_spa_row_doubles()), dtype=f64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        host = np.zeros(int(check(self.lib.cnmf_spa_ctl_doubles(self.k), "cnmf_spa_ctl_doubles")))
        host[SPA_RANK_TOL] = rank_tol
        self.ctl = torch.from_numpy(host).to(dev)
        self.scores = torch.zeros(self.n_rows, dtype=f64, device=dev) if scores else None

    def step(self, j):
        """Step j (a no-op once the control block's STOPPED word is set)."""
        import torch
        with torch.cuda.device(self.X.device):
            check(self.lib.cnmf_spa_step(
                self._ptr(self.X), self.xdt, self._ptr(self.Q), self._ptr(self.partials), self.rows,
                self._ptr(self.ticket), self._ptr(self.ctl), self._ptr(self.scores), self.n_rows, self.F, self.k,
                int(j), self.norm, torch.cuda.current_stream(self.X.device).cuda_stream), "cnmf_spa_step")

    def run(self):
        """The k steps back to back; one read of the control block.  Returns (idx, info)."""
        for j in range(self.k):
            self.step(j)
        return self.result()

    def result(self):
        ctl = self.ctl.cpu().numpy()
        steps = int(ctl[SPA_STEPS_DONE])
        idx = ctl[SPA_IDX:SPA_IDX + steps].astype(np.int64)
        info = dict(Q=self.Q[:steps].cpu().numpy(), rho=ctl[SPA_RHO:SPA_RHO + steps].copy(),
                    mean=float(ctl[SPA_SUM_X]) / (self.n_rows * self.F), steps=steps, ymax=float(ctl[SPA_YMAX]),
                    stopped=bool(ctl[SPA_STOPPED] != 0))
        return idx, info


def spa(X, n_components, *, normalise="l1", rank_tol=1e-12, device=None, return_info=False):
    """The rows of X that SPA picks, as np.int64 (fewer than n_components when the rank of X runs
    out: step j stops when ‖r_{p_j}‖ / max_i ‖y_i‖ <= rank_tol).

    normalise='l1' (default) scales every row to unit sum before the selection (an all-zero row
    is never picked); None takes the rows as they are, which favours the loudest.  NumPy X is
    copied to the device; a torch X on a HIP device stays there.  return_info=True: also a dict
    with Q (the orthonormal directions, steps x F fp64), rho, mean (X.mean()) and steps."""
    X = _validate(X, n_components, normalise, rank_tol)
    idx, info = SPAState(_to_device(X, device), n_components, normalise, rank_tol).run()
    return (idx, info) if return_info else idx


def start_w(Xd, M, floor, dtype=None):
    """W0 = max(X·M, floor) on the device (cnmf_spa_start_w); M: F x k fp64 (host or device)."""
    from .solver import _XDT, _ptr
    import torch
    lib = _lib.load()
    Md = torch.as_tensor(M, dtype=torch.float64).to(Xd.device).contiguous()
    n, F = (int(s) for s in Xd.shape)
    k = int(Md.shape[1])
    W = torch.empty((n, k), dtype=dtype or Xd.dtype, device=Xd.device)
    with torch.cuda.device(Xd.device):
        check(lib.cnmf_spa_start_w(_ptr(Xd), _XDT[Xd.dtype], _ptr(Md), float(floor), _ptr(W), _XDT[W.dtype], n, F, k,
                                   torch.cuda.current_stream(Xd.device).cuda_stream), "cnmf_spa_start_w")
    return W


def spa_init(X, n_components, *, normalise="l1", rank_tol=1e-12, device=None):
    """The SPA start (W0, H0) as device tensors of X's dtype: H0 = the picked rows of X with exact
    zeros replaced by floor = X.mean()/100, W0 = max(X·pinv(H0, rcond=1e-6), floor).  The k x F
    pseudo-inverse runs on the host (one synchronisation).  Raises ValueError when X has fewer than
    n_components independent rows."""
    import torch
    X = _validate(X, n_components, normalise, rank_tol)
    Xd = _to_device(X, device)
    idx, info = SPAState(Xd, n_components, normalise, rank_tol).run()
    if info["steps"] < n_components:
        raise ValueError(f"init='spa' found only {info['steps']} independent rows in X (rank_tol={rank_tol}): "
                         f"n_components={n_components} is too large for this X.")
    floor = info["mean"] / 100.0
    H0 = Xd.index_select(0, torch.from_numpy(idx).to(Xd.device))
    H0 = torch.where(H0 == 0, torch.full_like(H0, floor), H0)
    M = np.linalg.pinv(H0.cpu().numpy().astype(np.float64), rcond=1e-6)
    return start_w(Xd, M, floor), H0
