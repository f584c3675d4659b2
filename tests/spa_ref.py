"""The successive projection algorithm (SPA; Araújo et al. 2001, Gillis & Vavasis 2014) and the
NMF start built on it, restated in NumPy fp64.  This file is the specification of init='spa'
(cnmf_amd/spa.py, csrc/spa.hip).

    y_i   = s_i·x_i,  s_i = 1/Σ_f x_if ('l1'; 0 for an all-zero row) or 1 (None), in fp64
    step j = 0 .. k−1:
      r_i   = y_i − Σ_{t<j} q_t (q_t·y_i)        the residual vector, formed explicitly
      p_j   = the smallest i attaining max_i ‖r_i‖²
      ρ_j   = ‖r_{p_j}‖ / max_i ‖y_i‖              stop with j rows when ρ_j <= rank_tol
      q_j   = r_{p_j}/‖r_{p_j}‖, orthogonalised against q_0 .. q_{j−1} once more and normalised
    start: floor = X.mean()/100;  H0[j] = X[p_j] with exact zeros -> floor;
           W0 = max(X·pinv(H0, rcond=1e-6), floor), rounded once to X's dtype
"""
import numpy as np

__all__ = ["row_scale", "spa_ref", "spa_start_ref", "margins"]


def row_scale(X, normalise="l1"):
    """Y = s_i·x_i in fp64."""
    if normalise not in ("l1", None):
        raise ValueError(f"normalise must be 'l1' or None, got {normalise!r}")
    X64 = np.asarray(X, dtype=np.float64)
    if normalise is None:
        return X64.copy()
    sums = X64.sum(axis=1)
    s = np.zeros_like(sums)
    np.divide(1.0, sums, out=s, where=sums > 0)
    return X64 * s[:, None]


def spa_ref(X, k, normalise="l1", rank_tol=1e-12, return_scores=False):
    """Returns (idx, info): idx the picked rows (int64, at most k), info = dict(Q, rho, mean, steps,
    ymax[, scores: the n scores of every step])."""
    X = np.asarray(X)
    n, F = X.shape
    if not 1 <= k <= min(n, F, 16):
        raise ValueError(f"k={k} must be in 1..min(n, F, 16)={min(n, F, 16)}")
    Y = row_scale(X, normalise)
    Q = np.zeros((0, F))
    idx, rho, all_scores = [], [], []
    ymax = 0.0
    for j in range(k):
        R = Y - (Y @ Q.T) @ Q
        score = np.einsum("if,if->i", R, R)
        p = int(np.argmax(score))  # the first index attaining the maximum
        nr = float(np.sqrt(score[p]))
        if j == 0:
            ymax = nr
        if return_scores:
            all_scores.append(score)
        if not nr > rank_tol * ymax:
            break
        q = R[p] / nr
        q = q - Q.T @ (Q @ q)
        q = q / np.linalg.norm(q)
        Q = np.vstack([Q, q])
        idx.append(p)
        rho.append(nr / ymax)
    info = dict(Q=Q, rho=np.asarray(rho), mean=float(np.asarray(X, dtype=np.float64).mean()), steps=len(idx),
                ymax=ymax)
    if return_scores:
        info["scores"] = all_scores
    return np.asarray(idx, dtype=np.int64), info


def margins(scores):
    """Per step (best score − second-best score) / best: how far the runner-up is from the pick."""
    out = []
    for s in scores:
        if s.size < 2:
            out.append(1.0)
            continue
        top = np.partition(s, -2)[-2:]
        out.append(float((top[1] - top[0]) / top[1]) if top[1] > 0 else 0.0)
    return out


def spa_start_ref(X, idx, dtype=None):
    """(W0, H0, M, floor) of the SPA start from the picked rows."""
    X = np.asarray(X)
    dtype = X.dtype if dtype is None else dtype
    floor = float(np.asarray(X, dtype=np.float64).mean()) / 100.0
    H0 = X[np.asarray(idx)].astype(dtype, copy=True)
    H0[H0 == 0] = floor
    M = np.linalg.pinv(H0.astype(np.float64), rcond=1e-6)  # F x k
    W0 = np.maximum(X.astype(np.float64) @ M, floor).astype(dtype)
    return W0, H0, M, floor
