"""fp64 NumPy restatement of scikit-learn 1.7.2's coordinate-descent NMF solver with shuffle=False
(SKCD = `_fit_coordinate_descent`, sklearn/decomposition/_nmf.py:376-523, and `_update_cdnmf_fast`,
_cdnmf_fast.pyx), the "Fast HALS" sweep of Cichocki & Phan.  Test infrastructure only: the spec of
solver='hals' and the reference of the GPU tests where no golden file holds sklearn's own answer,
itself checked against every golden by tests/test_hals_ref.py.
"""
from __future__ import annotations

import numpy as np


def regularization(n_samples, n_features, alpha_W=0.0, alpha_H="same", l1_ratio=0.0):
    """SK `_compute_regularization`: (l1_W, l1_H, l2_W, l2_H)."""
    alpha_H = alpha_W if alpha_H == "same" else alpha_H
    return (n_features * alpha_W * l1_ratio, n_samples * alpha_H * l1_ratio,
            n_features * alpha_W * (1.0 - l1_ratio), n_samples * alpha_H * (1.0 - l1_ratio))


def sweep(R, C, G):
    """`_update_cdnmf_fast` with the identity permutation: one Gauss-Seidel sweep of the rows of R
    (n × k, updated in place) against G (k × k, l2 already on its diagonal) and C (n × k, l1 already
    subtracted).  Returns the violation Σ|projected gradient|."""
    k = R.shape[1]
    violation = 0.0
    for t in range(k):
        grad = -C[:, t].copy()
        for r in range(k):
            grad += G[t, r] * R[:, r]
        pg = np.where(R[:, t] == 0, np.minimum(0.0, grad), grad)
        violation += float(np.abs(pg).sum())
        if G[t, t] != 0:
            R[:, t] = np.maximum(R[:, t] - grad / G[t, t], 0.0)
    return violation


def half_iteration(X, R, Ft, l1, l2):
    """`_update_coordinate_descent`: sweep R (n × k) with the other factor Ft (m × k) fixed."""
    G = Ft.T @ Ft
    C = X @ Ft
    if l2 != 0:
        G.flat[::G.shape[0] + 1] += l2
    if l1 != 0:
        C -= l1
    return sweep(R, C, G)


def fit(X, W0, H0, tol=1e-4, max_iter=200, l1_W=0.0, l1_H=0.0, l2_W=0.0, l2_H=0.0, update_H=True):
    """`_fit_coordinate_descent`.  W0 None: the update_H=False start W = 0 (SK:1228-1235).  Returns a
    dict: W, H, n_iter, violations (violation / violation_init of every iteration run)."""
    X = np.asarray(X, dtype=np.float64)
    Ht = np.array(np.asarray(H0, dtype=np.float64).T, order="C")
    W = np.zeros((X.shape[0], Ht.shape[1])) if W0 is None else np.array(W0, dtype=np.float64, order="C")
    ratios, n_iter, violation_init = [], 0, 0.0
    for n_iter in range(1, max_iter + 1):
        violation = half_iteration(X, W, Ht, l1_W, l2_W)
        if update_H:
            violation += half_iteration(X.T, Ht, W, l1_H, l2_H)
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            break
        ratios.append(violation / violation_init)
        if violation / violation_init <= tol:
            break
    return {"W": W, "H": Ht.T.copy(), "n_iter": n_iter, "violations": ratios, "violation_init": violation_init}


def tol_margin(ratios, tol):
    """Closest relative approach of an iteration's violation ratio to tol (None for tol = 0)."""
    if not tol or not ratios:
        return None
    return min(abs(r - tol) / tol for r in ratios)
