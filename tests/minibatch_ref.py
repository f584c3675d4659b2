"""fp64 NumPy restatement of scikit-learn 1.7.2's MiniBatchNMF for the Frobenius loss
(SKMB = sklearn/decomposition/_nmf.py, class MiniBatchNMF): the fit loop, `_solve_W` and
`partial_fit`.  Test infrastructure only: the reference the GPU tests compare against where no
golden file holds sklearn's own answer, itself checked against every golden by
tests/test_minibatch_ref.py.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
STOP_NONE, STOP_H_CHANGE, STOP_NO_IMPROVEMENT = 0, 1, 2


def gen_batches(n, batch_size):
    """sklearn.utils.gen_batches(n, batch_size) as (lo, hi) pairs."""
    out, lo = [], 0
    for _ in range(int(n // batch_size)):
        out.append((lo, lo + batch_size))
        lo += batch_size
    if lo < n:
        out.append((lo, n))
    return out


def regularization(n_samples, n_features, alpha_W, alpha_H, l1_ratio):
    """SK `_compute_regularization` of a batch: (l1_W, l1_H, l2_W, l2_H)."""
    alpha_H = alpha_W if alpha_H == "same" else alpha_H
    return (n_features * alpha_W * l1_ratio, n_samples * alpha_H * l1_ratio,
            n_features * alpha_W * (1.0 - l1_ratio), n_samples * alpha_H * (1.0 - l1_ratio))


def update_w(X, W, H, l1_W, l2_W):
    """SK `_multiplicative_update_w` (beta_loss = 2); returns the new W."""
    num = X @ H.T
    den = W @ (H @ H.T)
    if l1_W > 0:
        den += l1_W
    if l2_W > 0:
        den = den + l2_W * W
    den[den == 0] = EPS32
    num /= den
    return W * num


def batch_cost(X, W, H, regs):
    l1_W, l1_H, l2_W, l2_H = regs
    R = X - W @ H
    return (0.5 * float(np.vdot(R, R)) + l1_W * W.sum() + l1_H * H.sum() + l2_W * (W ** 2).sum()
            + l2_H * (H ** 2).sum()) / X.shape[0]


def update_h(X, W, H, l1_H, l2_H, A, B, rho):
    """SK `_multiplicative_update_h` with the online accumulators A, B (updated in place)."""
    num = W.T @ X
    den = np.linalg.multi_dot([W.T, W, H])
    if l1_H > 0:
        den += l1_H
    if l2_H > 0:
        den = den + l2_H * H
    den[den == 0] = EPS32
    num *= H
    A *= rho
    B *= rho
    A += num
    B += den
    return A / B


def solve_w(X, H, max_iter, tol, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, log=None):
    """SKMB `_solve_W`; returns (W, iterations run).  log: a list that receives every W_diff."""
    k = H.shape[0]
    W = np.full((X.shape[0], k), np.sqrt(X.mean() / k), dtype=X.dtype)
    l1_W, _, l2_W, _ = regularization(X.shape[0], X.shape[1], alpha_W, alpha_H, l1_ratio)
    buf = W.copy()
    n = 0
    for _ in range(max_iter):
        W = update_w(X, W, H, l1_W, l2_W)
        n += 1
        diff = np.linalg.norm(W - buf) / np.linalg.norm(W)
        if log is not None:
            log.append(float(diff))
        if tol > 0 and diff <= tol:
            break
        buf[:] = W
    return W, n


class State:
    """The online state a sequence of steps shares: H, the accumulators and the stop bookkeeping."""

    def __init__(self, H, rho, tol=0.0, max_no_improvement=None, n_samples=0):
        self.H = np.array(H, dtype=np.float64)
        self.A = self.H.copy()
        self.B = np.ones_like(self.H)
        self.rho, self.tol, self.mni, self.n_samples = rho, tol, max_no_improvement, n_samples
        self.ewa = self.ewa_min = None
        self.no_improvement = 0
        self.steps = 0
        self.reason = STOP_NONE
        self.log = []      # (cost, H_diff, ewa) per step
        self.margins = []  # relative separations of every stop comparison: ('hdiff' | 'ewa', value)

    def step(self, X, W, alpha_W=0.0, alpha_H="same", l1_ratio=0.0, update_W=True, check=True):
        """SKMB `_minibatch_step` + `_minibatch_convergence` on the batch; W is updated in place.
        Returns True when the fit stops."""
        regs = regularization(X.shape[0], X.shape[1], alpha_W, alpha_H, l1_ratio)
        if update_W:
            W[:] = update_w(X, W, self.H, regs[0], regs[2])
        cost = batch_cost(X, W, self.H, regs)
        H_old = self.H
        self.H = update_h(X, W, H_old.copy(), regs[1], regs[3], self.A, self.B, self.rho)
        self.steps += 1
        hdiff = float(np.linalg.norm(self.H - H_old) / np.linalg.norm(self.H))
        if self.steps == 1 or not check:
            self.log.append((cost, hdiff, 0.0 if self.ewa is None else self.ewa))
            return False
        if self.ewa is None:
            self.ewa = cost
        else:
            alpha = min(X.shape[0] / (self.n_samples + 1), 1)
            self.ewa = self.ewa * (1 - alpha) + cost * alpha
        self.log.append((cost, hdiff, self.ewa))
        if self.tol > 0:
            self.margins.append(("hdiff", abs(hdiff - self.tol) / self.tol))
            if hdiff <= self.tol:
                self.reason = STOP_H_CHANGE
                return True
        if self.ewa_min is not None and self.mni is not None:
            self.margins.append(("ewa", abs(self.ewa - self.ewa_min) / abs(self.ewa_min)))
        if self.ewa_min is None or self.ewa < self.ewa_min:
            self.no_improvement = 0
            self.ewa_min = self.ewa
        else:
            self.no_improvement += 1
        if self.mni is not None and self.no_improvement >= self.mni:
            self.reason = STOP_NO_IMPROVEMENT
            return True
        return False


def fit(X, W0, H0, batch_size=1024, tol=1e-4, max_no_improvement=10, max_iter=200, alpha_W=0.0,
        alpha_H="same", l1_ratio=0.0, forget_factor=0.7):
    """SKMB `_fit_transform` from the custom start (W0, H0).  Returns a dict: W, H, n_iter, n_steps,
    reason, log, margins."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    W = np.array(W0, dtype=np.float64)
    bs = min(batch_size, n)
    st = State(H0, forget_factor ** (bs / n), tol, max_no_improvement, n)
    batches = gen_batches(n, bs)
    per_iter = int(math.ceil(n / bs))
    for _, (lo, hi) in zip(range(max_iter * per_iter), itertools.cycle(batches)):
        if st.step(X[lo:hi], W[lo:hi], alpha_W, alpha_H, l1_ratio):
            break
    return {"W": W, "H": st.H, "n_steps": st.steps, "n_iter": int(math.ceil(st.steps / per_iter)),
            "reason": st.reason, "log": st.log, "margins": st.margins}


def partial_fit_sequence(chunks, H0, batch_size=1024, forget_factor=0.7, tol=1e-4,
                         fresh_restarts_max_iter=30, alpha_W=0.0, alpha_H="same", l1_ratio=0.0):
    """SKMB `partial_fit` over `chunks` from the custom start H0 (rho from the first chunk, as
    SKMB's `_check_params` on the first call).  Returns (H, n_steps)."""
    first = np.asarray(chunks[0], dtype=np.float64)
    bs = min(batch_size, first.shape[0])
    st = State(H0, forget_factor ** (bs / first.shape[0]))
    for c in chunks:
        c = np.asarray(c, dtype=np.float64)
        W, _ = solve_w(c, st.H, fresh_restarts_max_iter, tol, alpha_W, alpha_H, l1_ratio)
        st.step(c, W, alpha_W, alpha_H, l1_ratio, update_W=False, check=False)
    return st.H, st.steps
