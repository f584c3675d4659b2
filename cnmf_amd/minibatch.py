"""`MiniBatchNMF`: scikit-learn 1.7.2's online multiplicative-update estimator (SKMB =
sklearn/decomposition/_nmf.py, class MiniBatchNMF) on the MI355X path, Frobenius loss.

One minibatch step — the W update of the batch's rows, the batch cost, the online H update through
the running numerator / denominator, and both of SKMB's stopping rules — is ONE launch
(cnmf_mb_step, csrc/minibatch.hip).  A stop sets a word on the device that turns every later launch
into a no-op, so `fit` enqueues a whole epoch of steps without a host round trip and reads the
control block once per epoch (never, when tol == 0 and max_no_improvement is None).

Scope: dense fp32 / fp64 X, n_components <= 16, n_features <= 512, one device.  Not available
(each raises): beta_loss other than Frobenius, fresh_restarts=True, weights, solver='als',
memory_budget, devices= / sharded fits, bf16 X.
"""
from __future__ import annotations

import math
import numbers
import warnings

import numpy as np

from . import _lib
from ._lib import check
from .api import (ConvergenceWarning, _check_init, _check_non_negative, _check_X, _compute_regularization,
                  _dtype_name, _initial_factors, _is_torch, _out, _torch, _transform_start, _validate_params)

__all__ = ["MiniBatchNMF", "MiniBatchPlan"]

# control-block slots and flags (include/cnmf_hip.h: cnmf_mb_slots, cnmf_mb_flags, cnmf_mb_stop)
(MB_STOPPED, MB_REASON, MB_STEPS_DONE, MB_LAST_COST, MB_LAST_HDIFF, MB_EWA, MB_EWA_MIN, MB_NO_IMPROVE,
 MB_HAVE_EWA, MB_HAVE_MIN, MB_RHO, MB_TOL, MB_MAX_NO_IMPROVE, MB_N_SAMPLES, MB_LOG_CAP, MB_NLOG, MB_W_ITERS,
 MB_W_DIFF) = range(18)
MB_LOG = 32
MB_UPDATE_W, MB_UPDATE_H = 1, 2
STOP_NONE, STOP_H_CHANGE, STOP_NO_IMPROVEMENT, STOP_W_CHANGE = 0, 1, 2, 3
MAX_FEATURES, MAX_COMPONENTS = 512, 16

_WHOM = "MiniBatchNMF (input X)"


def _ptr(t):
    return None if t is None else t.data_ptr()


def _gen_batches(n, batch_size):
    """sklearn.utils.gen_batches as (lo, hi) pairs."""
    out, lo = [], 0
    for _ in range(n // batch_size):
        out.append((lo, lo + batch_size))
        lo += batch_size
    if lo < n:
        out.append((lo, n))
    return out


class MiniBatchPlan:
    """The device state of one online fit and its launches: the fp64 basis (H64, Ht, HHt), the
    running numerator / denominator (Anum, Bden), the control block, and X / W when they are
    attached.  Everything is enqueued on the current stream of `device`; nothing synchronises
    except `read_ctl` and `H`."""

    def __init__(self, H, dtype, device, *, rho, tol=0.0, max_no_improvement=None, n_samples=0, log_cap=0):
        torch = _torch()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.tc = dtype
        self.xdt = _lib.F64 if dtype == torch.float64 else _lib.F32
        H = torch.as_tensor(H)
        self.k, self.F = int(H.shape[0]), int(H.shape[1])
        self.KP = check(self.lib.cnmf_padded_k(self.k), "cnmf_padded_k")
        self.row_doubles = check(self.lib.cnmf_mb_row_doubles(self.F, self.k), "cnmf_mb_row_doubles")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.H64 = H.to(**f64).contiguous().clone()
        self.Ht = torch.zeros(self.F * self.KP, **f64)
        self.HHt = torch.zeros(self.KP * self.KP, **f64)
        self.Anum = self.H64.clone()             # SKMB _components_numerator
        self.Bden = torch.ones_like(self.H64)    # SKMB _components_denominator
        self.counter = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.log_cap = int(log_cap)
        self.ctl = self.new_ctl(rho=rho, tol=tol, max_no_improvement=max_no_improvement, n_samples=n_samples,
                                log_cap=self.log_cap)
        self.partials = None
        self.X = self.W = None
        self._stage = None
        self.refresh_basis()

    # -- plumbing ------------------------------------------------------------------------------
    def _stream(self):
        return _torch().cuda.current_stream(self.device).cuda_stream

    def new_ctl(self, *, rho=1.0, tol=0.0, max_no_improvement=None, n_samples=0, log_cap=0):
        torch = _torch()
        n = check(self.lib.cnmf_mb_ctl_doubles(int(log_cap)), "cnmf_mb_ctl_doubles")
        host = np.zeros(n, dtype=np.float64)
        host[MB_RHO], host[MB_TOL], host[MB_N_SAMPLES], host[MB_LOG_CAP] = rho, tol, n_samples, log_cap
        host[MB_MAX_NO_IMPROVE] = -1.0 if max_no_improvement is None else float(max_no_improvement)
        return torch.from_numpy(host).to(self.device)

    def refresh_basis(self):
        torch = _torch()
        with torch.cuda.device(self.device):
            check(self.lib.cnmf_basis_update(None, _ptr(self.H64), _ptr(self.Ht), _ptr(self.HHt), self.F, self.k,
                                             0.0, 0.0, 0, None, self._stream()), "cnmf_basis_update")

    def attach(self, X, W):
        """The rows the steps run over: X (n × F) and W (n × k) on the device, contiguous, in the
        plan's dtype."""
        assert X.dtype == self.tc and W.dtype == self.tc and X.is_contiguous() and W.is_contiguous()
        assert X.shape[1] == self.F and W.shape[1] == self.k and X.shape[0] == W.shape[0]
        self.X, self.W = X, W

    def _partials_for(self, n_rows):
        torch = _torch()
        rows = check(self.lib.cnmf_mb_rows(n_rows), "cnmf_mb_rows")
        if self.partials is None or self.partials.numel() < rows * self.row_doubles:
            self.partials = torch.empty(rows * self.row_doubles, dtype=torch.float64, device=self.device)
        return rows

    def _window(self, lo, hi):
        """X[lo:hi], W[lo:hi] as launch arguments: the views themselves when both start 16-byte
        aligned, else aligned staging copies (the caller copies the staged W back)."""
        torch = _torch()
        Xw, Ww = self.X[lo:hi], self.W[lo:hi]
        if Xw.data_ptr() % 16 == 0 and Ww.data_ptr() % 16 == 0:
            return Xw, Ww, False
        n = hi - lo
        if self._stage is None or self._stage[0].shape[0] < n:
            self._stage = (torch.empty((n, self.F), dtype=self.tc, device=self.device),
                           torch.empty((n, self.k), dtype=self.tc, device=self.device))
        Xs, Ws = self._stage[0][:n], self._stage[1][:n]
        Xs.copy_(Xw)
        Ws.copy_(Ww)
        return Xs, Ws, True

    # -- launches ------------------------------------------------------------------------------
    def step(self, lo, hi, regs=(0.0, 0.0, 0.0, 0.0), update_W=True, update_H=True):
        """One minibatch step on rows [lo, hi); regs = (l1_W, l1_H, l2_W, l2_H) of the batch."""
        torch = _torch()
        n = hi - lo
        rows = self._partials_for(n)
        Xw, Ww, staged = self._window(lo, hi)
        flags = (MB_UPDATE_W if update_W else 0) | (MB_UPDATE_H if update_H else 0)
        with torch.cuda.device(self.device):
            check(self.lib.cnmf_mb_step(_ptr(Xw), self.xdt, _ptr(Ww), _ptr(self.H64), _ptr(self.Ht), _ptr(self.HHt),
                                        _ptr(self.Anum), _ptr(self.Bden), _ptr(self.partials), rows,
                                        _ptr(self.counter), _ptr(self.ctl), n, self.F, self.k, regs[0], regs[2],
                                        regs[1], regs[3], flags, self._stream()), "cnmf_mb_step")
        if staged and update_W:
            self.W[lo:hi].copy_(Ww)

    def solve_w(self, max_iter, tol, regs=(0.0, 0.0, 0.0, 0.0)):
        """SKMB _solve_W over all attached rows from the W already there: max_iter gated launches,
        one read.  Returns the iterations run."""
        torch = _torch()
        n = int(self.X.shape[0])
        rows = self._partials_for(n)
        ctl = self.new_ctl(tol=tol)
        Xw, Ww, staged = self._window(0, n)
        with torch.cuda.device(self.device):
            for _ in range(max_iter):
                check(self.lib.cnmf_mb_solve_w(_ptr(Xw), self.xdt, _ptr(Ww), _ptr(self.Ht), _ptr(self.HHt),
                                               _ptr(self.partials), rows, _ptr(self.counter), _ptr(ctl), n, self.F,
                                               self.k, regs[0], regs[2], self._stream()), "cnmf_mb_solve_w")
        if staged:
            self.W.copy_(Ww)
        return int(ctl[:MB_LOG].cpu()[MB_W_ITERS])

    def read_ctl(self):
        """The control block's scalars as a NumPy array (synchronises)."""
        return self.ctl[:MB_LOG].cpu().numpy()

    def read_log(self):
        """[(cost, H_diff, ewa)] of the logged steps (synchronises)."""
        host = self.ctl.cpu().numpy()
        return host[MB_LOG:MB_LOG + 3 * int(host[MB_NLOG])].reshape(-1, 3)

    def resume(self):
        """Clear a stop and its rules: the steps `partial_fit` adds to a finished fit never stop."""
        self.ctl[MB_STOPPED] = 0.0
        self.ctl[MB_TOL] = 0.0
        self.ctl[MB_MAX_NO_IMPROVE] = -1.0

    def H(self, dtype=None):
        return self.H64.to(dtype or self.tc)

    def frobenius_error(self) -> float:
        """‖X − W·H‖ of the attached rows with the library's loss pass (synchronises)."""
        torch = _torch()
        lib, n = self.lib, int(self.X.shape[0])
        with torch.cuda.device(self.device):
            nb = check(lib.cnmf_pass_blocks(n, self.F, self.k, self.xdt), "cnmf_pass_blocks")
            parts = torch.empty(nb * max(1, self.k * (self.F + self.k)), dtype=torch.float64, device=self.device)
            stage = torch.empty(check(lib.cnmf_stage_doubles(1), "cnmf_stage_doubles"), dtype=torch.float64,
                                device=self.device)
            counter = torch.zeros(int(lib.cnmf_counter_words()), dtype=torch.int32, device=self.device)
            out = torch.zeros(1, dtype=torch.float64, device=self.device)
            check(lib.cnmf_mu_sample_pass(_ptr(self.X), self.xdt, _ptr(self.W), _ptr(self.Ht), _ptr(self.HHt),
                                          _ptr(parts), n, self.F, self.k, 0.0, 0.0, _lib.PASS_LOSS, self._stream()),
                  "cnmf_mu_sample_pass")
            check(lib.cnmf_reduce_partials(_ptr(parts), nb, 1, _ptr(stage), _ptr(counter), _ptr(out),
                                           self._stream()), "cnmf_reduce_partials")
        return math.sqrt(max(float(out.item()), 0.0))


_PARAMS = ("n_components", "init", "batch_size", "beta_loss", "tol", "max_no_improvement", "max_iter", "alpha_W",
           "alpha_H", "l1_ratio", "forget_factor", "fresh_restarts", "fresh_restarts_max_iter", "transform_max_iter",
           "random_state", "verbose", "device")
# options of the full-batch API that the online fit does not offer
_REFUSED = ("weights", "solver", "memory_budget", "devices", "group", "normalise", "sum_to_one", "smoothness")


def _refuse(options):
    for name, v in options.items():
        if name not in _REFUSED:
            raise TypeError(f"MiniBatchNMF got an unexpected keyword argument {name!r}")
        if v is None or (name == "solver" and v == "mu") or (name == "smoothness" and not v):
            continue
        shown = repr(v) if isinstance(v, (str, numbers.Number)) else f"<{type(v).__name__}>"
        raise ValueError(f"{name}={shown} is not available for MiniBatchNMF: the online fit runs the unweighted "
                         "multiplicative update on one device with X in device memory.")


def _int_param(name, v, none_ok=False):
    if none_ok and v is None:
        return
    if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < 1:
        raise ValueError(f"The {name!r} parameter must be an int in the range [1, inf){' or None' if none_ok else ''}. "
                         f"Got {v!r} instead.")


class MiniBatchNMF:
    """sklearn-shaped online estimator (SKMB) on the MI355X path.

    Attributes after fit: components_, n_components_, n_iter_, n_steps_, reconstruction_err_,
    n_features_in_; after transform also n_transform_iter_ (the _solve_W iterations run).
    """

    def __init__(self, n_components="auto", *, init=None, batch_size=1024, beta_loss="frobenius", tol=1e-4,
                 max_no_improvement=10, max_iter=200, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, forget_factor=0.7,
                 fresh_restarts=False, fresh_restarts_max_iter=30, transform_max_iter=None, random_state=None,
                 verbose=0, device=None, **unsupported):
        _refuse(unsupported)
        self.n_components = n_components
        self.init = init
        self.batch_size = batch_size
        self.beta_loss = beta_loss
        self.tol = tol
        self.max_no_improvement = max_no_improvement
        self.max_iter = max_iter
        self.alpha_W = alpha_W
        self.alpha_H = alpha_H
        self.l1_ratio = l1_ratio
        self.forget_factor = forget_factor
        self.fresh_restarts = fresh_restarts
        self.fresh_restarts_max_iter = fresh_restarts_max_iter
        self.transform_max_iter = transform_max_iter
        self.random_state = random_state
        self.verbose = verbose
        self.device = device
        self._poll_steps = None  # steps between reads of the control block; None = one epoch

    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in _PARAMS}

    def set_params(self, **params):
        for k, v in params.items():
            if k not in _PARAMS:
                raise ValueError(f"Invalid parameter {k!r} for estimator MiniBatchNMF. Valid parameters are: "
                                 f"{sorted(_PARAMS)!r}.")
            setattr(self, k, v)
        return self

    # -- validation (messages follow sklearn's; nothing here touches a device) -------------------
    def _validate(self):
        _validate_params(self.n_components, self.init, "mu", self.beta_loss, self.tol, self.max_iter, self.alpha_W,
                         self.alpha_H, self.l1_ratio)
        _int_param("batch_size", self.batch_size)
        _int_param("max_no_improvement", self.max_no_improvement, none_ok=True)
        _int_param("fresh_restarts_max_iter", self.fresh_restarts_max_iter)
        _int_param("transform_max_iter", self.transform_max_iter, none_ok=True)
        ff = self.forget_factor
        if not isinstance(ff, numbers.Real) or isinstance(ff, bool) or not 0 <= ff <= 1:
            raise ValueError(f"The 'forget_factor' parameter must be a float in the range [0.0, 1.0]. Got {ff!r} instead.")
        if not isinstance(self.fresh_restarts, (bool, np.bool_)):
            raise ValueError("The 'fresh_restarts' parameter must be an instance of 'bool' or an instance of "
                             f"'numpy.bool_'. Got {self.fresh_restarts!r} instead.")
        if self.fresh_restarts:
            raise ValueError("fresh_restarts=True is not available yet: every step updates the batch's W once "
                             "(fresh_restarts=False).")

    def _check_X(self, X):
        X = _check_X(X)
        if _is_torch(X) and X.dtype == _torch().bfloat16:
            raise TypeError("MiniBatchNMF takes float32 or float64 X (bfloat16 is not available).")
        _check_non_negative(X, _WHOM)
        if X.shape[1] > MAX_FEATURES:
            raise ValueError(f"X has {X.shape[1]} features: MiniBatchNMF handles 1..{MAX_FEATURES}.")
        return X

    def _start(self, X, W, H):
        """SK _check_w_h with update_H=True: k and the starting factors (host or device arrays)."""
        n, F = X.shape
        k = self.n_components
        if k is None:
            k = F
        if self.init == "custom":
            H = _check_init(H, (k, F), "NMF (input H)")
            W = _check_init(W, (n, k), "NMF (input W)")
            if k == "auto":
                k = H.shape[0]
            if H.dtype != X.dtype or W.dtype != X.dtype:
                raise TypeError("H and W should have the same dtype as X. Got H.dtype = {} and W.dtype = {}."
                                .format(_dtype_name(H), _dtype_name(W)))
            k = int(k)
        else:
            if W is not None or H is not None:
                warnings.warn("When init!='custom', provided W or H are ignored. Set  init='custom' to use them "
                              "as initialization.", RuntimeWarning)
            k = F if k == "auto" else int(k)
        if k > MAX_COMPONENTS:
            raise ValueError(f"n_components={k} is not supported: the MI355X kernels handle 1..16.")
        if self.init != "custom":
            W, H = _initial_factors(X, k, self.init, self.random_state, self.device, _is_torch(X), None,
                                    host_only=True)
        return k, W, H

    def _device(self, X):
        torch = _torch()
        if self.device is not None:
            return torch.device(self.device)
        if _is_torch(X) and X.device.type == "cuda":
            return X.device
        return torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def _to_device(A, dev, dtype=None):
        torch = _torch()
        t = A if _is_torch(A) else torch.from_numpy(np.ascontiguousarray(A))
        return t.to(device=dev, dtype=dtype or t.dtype).contiguous()

    def _regs(self, n_rows, F):
        return _compute_regularization(n_rows, F, self.alpha_W, self.alpha_H, self.l1_ratio)

    # -- fit -----------------------------------------------------------------------------------
    def fit_transform(self, X, y=None, W=None, H=None, **unsupported):
        """SKMB fit_transform: learn the model from X in minibatches, return W."""
        _refuse(unsupported)
        self._validate()
        X = self._check_X(X)
        as_torch = _is_torch(X)
        k, W0, H0 = self._start(X, W, H)
        n, F = int(X.shape[0]), int(X.shape[1])
        bs = min(self.batch_size, n)
        per_iter = int(math.ceil(n / bs))
        n_steps = self.max_iter * per_iter
        dev = self._device(X)
        Xd = self._to_device(X, dev)
        Wd = self._to_device(W0, dev, Xd.dtype).clone()
        plan = MiniBatchPlan(H0, Xd.dtype, dev, rho=self.forget_factor ** (bs / n), tol=self.tol,
                             max_no_improvement=self.max_no_improvement, n_samples=n,
                             log_cap=n_steps if self.verbose else min(n_steps, 4096))
        plan.attach(Xd, Wd)
        batches = _gen_batches(n, bs)
        regs = [self._regs(hi - lo, F) for lo, hi in batches]
        polls = self.tol > 0 or self.max_no_improvement is not None
        poll_every = self._poll_steps or per_iter
        done = 0
        while done < n_steps:
            stretch = min(poll_every, n_steps - done) if polls else n_steps - done
            for i in range(done, done + stretch):
                b = i % per_iter
                plan.step(batches[b][0], batches[b][1], regs[b])
            done += stretch
            if polls and plan.read_ctl()[MB_STOPPED] != 0.0:
                break
        ctl = plan.read_ctl()
        self.n_steps_ = int(ctl[MB_STEPS_DONE])
        self.n_iter_ = int(math.ceil(self.n_steps_ / per_iter))
        self._stop_reason = int(ctl[MB_REASON])
        if self.verbose:
            self._print_log(plan.read_log(), n_steps, self._stop_reason)
        if self.n_iter_ == self.max_iter and self.tol > 0:
            warnings.warn(f"Maximum number of iterations {self.max_iter} reached. Increase it to improve "
                          "convergence.", ConvergenceWarning)
        self.reconstruction_err_ = plan.frobenius_error()
        self.n_components_ = k
        self.n_features_in_ = F
        self.components_ = _out(plan.H(), as_torch, X)
        self._plan = plan
        Wout = _out(Wd, as_torch, X)
        plan.X = plan.W = None  # the fitted state outlives the fit; the data does not
        return Wout

    def fit(self, X, y=None, **params):
        self.fit_transform(X, **params)
        return self

    @staticmethod
    def _print_log(log, n_steps, reason):
        for i, (cost, _, ewa) in enumerate(log, 1):
            if i == 1:
                print(f"Minibatch step {i}/{n_steps}: mean batch cost: {cost}")
            else:
                print(f"Minibatch step {i}/{n_steps}: mean batch cost: {cost}, ewa cost: {ewa}")
        if reason == STOP_H_CHANGE:
            print(f"Converged (small H change) at step {len(log)}/{n_steps}")
        elif reason == STOP_NO_IMPROVEMENT:
            print(f"Converged (lack of improvement in objective function) at step {len(log)}/{n_steps}")

    # -- transform / partial_fit -----------------------------------------------------------------
    def _check_fitted(self):
        if not hasattr(self, "components_"):
            raise ValueError("This MiniBatchNMF instance is not fitted yet. Call 'fit' with appropriate "
                             "arguments before using this estimator.")

    def _check_features(self, X):
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but MiniBatchNMF is expecting "
                             f"{self.n_features_in_} features as input.")

    def _fitted_plan(self, dtype, dev):
        """The plan that holds the fitted basis: the fit's own (its fp64 H), or one built from a
        components_ the caller set."""
        plan = getattr(self, "_plan", None)
        if plan is None or plan.tc != dtype or plan.device != dev:
            plan = MiniBatchPlan(self.components_, dtype, dev, rho=1.0)
        return plan

    def _solve_W(self, plan, Xd, max_iter):
        """SKMB _solve_W on the device: W from sqrt(X.mean() / k); returns (W, iterations run)."""
        torch = _torch()
        n = int(Xd.shape[0])
        Wd = torch.full((n, plan.k), _transform_start(Xd, True, plan.k), dtype=Xd.dtype, device=Xd.device)
        plan.attach(Xd, Wd)
        iters = plan.solve_w(max_iter, self.tol, self._regs(n, plan.F))
        return Wd, iters

    def transform(self, X):
        """SKMB transform: _solve_W over all rows with components_ fixed."""
        self._check_fitted()
        self._validate()
        X = self._check_X(X)
        self._check_features(X)
        dev = self._device(X)
        Xd = self._to_device(X, dev)
        plan = self._fitted_plan(Xd.dtype, dev)
        max_iter = self.max_iter if self.transform_max_iter is None else self.transform_max_iter
        Wd, self.n_transform_iter_ = self._solve_W(plan, Xd, max_iter)
        plan.X = plan.W = None
        return _out(Wd, _is_torch(X), X)

    def partial_fit(self, X, y=None, W=None, H=None, **unsupported):
        """SKMB partial_fit: one online step on the chunk X (its W solved afresh with
        fresh_restarts_max_iter iterations of _solve_W).  The accumulators stay on the device
        between calls."""
        _refuse(unsupported)
        self._validate()
        X = self._check_X(X)
        as_torch = _is_torch(X)
        n, F = int(X.shape[0]), int(X.shape[1])
        dev = self._device(X)
        if not hasattr(self, "components_"):
            k, _, H0 = self._start(X, W, H)
            Xd = self._to_device(X, dev)
            bs = min(self.batch_size, n)
            self._plan = MiniBatchPlan(H0, Xd.dtype, dev, rho=self.forget_factor ** (bs / n), n_samples=n,
                                       log_cap=0)
            self.n_components_, self.n_features_in_, self.n_steps_ = k, F, 0
        else:
            self._check_features(X)
            Xd = self._to_device(X, dev)
            fitted = self._fitted_plan(Xd.dtype, dev)
            if fitted is not getattr(self, "_plan", None):
                self._plan = fitted
            self._plan.resume()
        plan = self._plan
        self._solve_W(plan, Xd, self.fresh_restarts_max_iter)
        plan.step(0, n, self._regs(n, F), update_W=False, update_H=True)
        self.components_ = _out(plan.H(), as_torch, X)
        self.n_steps_ += 1
        plan.X = plan.W = None
        return self

    def inverse_transform(self, X=None, *, Xt=None):
        """W·H back in data space (SK `_BaseNMF.inverse_transform`)."""
        self._check_fitted()
        X = Xt if X is None else X
        if _is_torch(X):
            return X @ self.components_
        return np.asarray(X) @ self.components_
