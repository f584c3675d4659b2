"""fp64 NumPy restatement of solver='whals': the coordinate-descent sweep of tests/hals_ref.py for the
weighted objective ½ Σ m_if (x_if − Σ_j w_ij h_jf)² plus sklearn's l1 / l2 terms, M ≥ 0 elementwise
(m = 0: a missing value; m = 1/σ²: an uncertainty weight).  The weights couple the features, so the
Gram matrix of a sweep is per row: G_i = Ft'·diag(m_i)·Ft.  With M = 1 every G_i is hals_ref's G and
the fit is sklearn's solver='cd' with shuffle=False.  Test infrastructure only: the spec of the
kernel and the reference of the GPU tests, itself checked by tests/test_whals_ref.py.
"""
from __future__ import annotations

import numpy as np

from hals_ref import regularization, tol_margin  # noqa: F401  (re-exported for the tests)

CHUNK = 4096  # rows whose k × k Gram matrices are held at a time


def sweep_rows(R, C, G):
    """hals_ref.sweep with a Gram matrix per row: R (n × k, updated in place), C (n × k, l1 already
    subtracted), G (n × k × k, l2 already on the diagonals).  Returns the violation Σ|pg|."""
    k = R.shape[1]
    violation = 0.0
    for t in range(k):
        grad = -C[:, t].copy()
        for r in range(k):
            grad += G[:, t, r] * R[:, r]
        pg = np.where(R[:, t] == 0, np.minimum(0.0, grad), grad)
        violation += float(np.abs(pg).sum())
        hess = G[:, t, t]
        upd = hess != 0
        R[upd, t] = np.maximum(R[upd, t] - grad[upd] / hess[upd], 0.0)
    return violation


def half_iteration(X, M, R, Ft, l1, l2):
    """One sweep of R (n × k) with the other factor Ft (f × k) fixed: per row i, G_i = Ftᵀ·diag(m_i)·Ft
    with l2 on its diagonal and c_i = Ftᵀ·(m_i ∘ x_i) − l1."""
    k = R.shape[1]
    P = (Ft[:, :, None] * Ft[:, None, :]).reshape(Ft.shape[0], k * k)  # h_a·h_b per feature
    violation = 0.0
    for r0 in range(0, R.shape[0], CHUNK):
        sl = slice(r0, r0 + CHUNK)
        G = (M[sl] @ P).reshape(-1, k, k)
        C = (M[sl] * X[sl]) @ Ft
        if l2 != 0:
            G[:, np.arange(k), np.arange(k)] += l2
        if l1 != 0:
            C -= l1
        Rc = R[sl]
        violation += sweep_rows(Rc, C, G)
        R[sl] = Rc
    return violation


def fit(X, M, W0, H0, tol=1e-4, max_iter=200, l1_W=0.0, l1_H=0.0, l2_W=0.0, l2_H=0.0, update_H=True):
    """hals_ref.fit with the weights M.  W0 None: the update_H=False start W = 0.  Returns a dict: W, H,
    n_iter, violations (violation / violation_init of every iteration run), objectives (the weighted
    ½ Σ m r² + penalties after every iteration)."""
    X = np.asarray(X, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    Xt, Mt = np.ascontiguousarray(X.T), np.ascontiguousarray(M.T)
    Ht = np.array(np.asarray(H0, dtype=np.float64).T, order="C")
    W = np.zeros((X.shape[0], Ht.shape[1])) if W0 is None else np.array(W0, dtype=np.float64, order="C")
    ratios, objectives, n_iter, violation_init = [], [], 0, 0.0
    for n_iter in range(1, max_iter + 1):
        violation = half_iteration(X, M, W, Ht, l1_W, l2_W)
        if update_H:
            violation += half_iteration(Xt, Mt, Ht, W, l1_H, l2_H)
        objectives.append(objective(X, M, W, Ht.T, l1_W, l1_H, l2_W, l2_H))
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            break
        ratios.append(violation / violation_init)
        if violation / violation_init <= tol:
            break
    return {"W": W, "H": Ht.T.copy(), "n_iter": n_iter, "violations": ratios, "violation_init": violation_init,
            "objectives": objectives}


def objective(X, M, W, H, l1_W=0.0, l1_H=0.0, l2_W=0.0, l2_H=0.0):
    """½ Σ m (x − wh)² + l1_W Σ w + l1_H Σ h + ½ l2_W Σ w² + ½ l2_H Σ h²."""
    R = X - W @ H
    return (0.5 * float((M * R * R).sum()) + l1_W * float(W.sum()) + l1_H * float(H.sum())
            + 0.5 * l2_W * float((W * W).sum()) + 0.5 * l2_H * float((H * H).sum()))


def weighted_error(X, M, W, H):
    """sqrt(Σ m (x − wh)²): what reconstruction_err_ reports for a weighted fit."""
    R = np.asarray(X, dtype=np.float64) - np.asarray(W, dtype=np.float64) @ np.asarray(H, dtype=np.float64)
    return float(np.sqrt((np.asarray(M, dtype=np.float64) * R * R).sum()))


def weights(shape, seed, zeros=0.3, lo=0.25, hi=4.0, dtype=np.float64):
    """Random weights in [lo, hi] with a share `zeros` of them zero."""
    rng = np.random.RandomState(seed)
    M = rng.uniform(lo, hi, size=shape)
    M[rng.uniform(size=shape) < zeros] = 0.0
    return M.astype(dtype)
