"""fp64 NumPy restatement of solver='hals' over row shards (test infrastructure only): the iteration
of tests/hals_ref.py with the rows dealt to `world` ranks by cnmf_amd.distributed.shard_bounds.

Per iteration: every shard sweeps its own rows of W (hals_ref.sweep against G = HHᵀ, C = X_r Hᵀ) and
forms its A_r = W_r'ᵀX_r (k × F), B_r = W_r'ᵀW_r' (k × k) and violation; the three are summed over the
shards in rank order — the one all-reduce of the sharded fit — and ONE H-sweep (C = Aᵀ, G = B) and one
stopping rule follow, the same for every rank.  An empty shard contributes zeros.
"""
from __future__ import annotations

import numpy as np

import hals_ref as ref
from cnmf_amd.distributed import shard_bounds


def fit(X, W0, H0, world, tol=1e-4, max_iter=200, l1_W=0.0, l1_H=0.0, l2_W=0.0, l2_H=0.0, update_H=True):
    """hals_ref.fit's arguments and result, plus `world`; "bounds" lists every rank's [lo, hi)."""
    X = np.asarray(X, dtype=np.float64)
    Ht = np.array(np.asarray(H0, dtype=np.float64).T, order="C")
    k = Ht.shape[1]
    bounds = [shard_bounds(X.shape[0], world, r) for r in range(world)]
    Xs = [X[lo:hi] for lo, hi in bounds]
    Ws = [np.zeros((hi - lo, k)) if W0 is None else np.array(W0[lo:hi], dtype=np.float64, order="C")
          for lo, hi in bounds]
    ratios, n_iter, violation_init = [], 0, 0.0
    for n_iter in range(1, max_iter + 1):
        G = Ht.T @ Ht
        if l2_W != 0:
            G.flat[::k + 1] += l2_W
        A, B, violation = np.zeros((k, X.shape[1])), np.zeros((k, k)), 0.0
        for Xr, Wr in zip(Xs, Ws):  # a rank each; then the all-reduce
            C = Xr @ Ht
            if l1_W != 0:
                C -= l1_W
            violation += ref.sweep(Wr, C, G)
            A += Wr.T @ Xr
            B += Wr.T @ Wr
        if update_H:  # on every rank, from the same sums
            if l2_H != 0:
                B.flat[::k + 1] += l2_H
            C = np.array(A.T, order="C")
            if l1_H != 0:
                C -= l1_H
            violation += ref.sweep(Ht, C, B)
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            break
        ratios.append(violation / violation_init)
        if violation / violation_init <= tol:
            break
    return {"W": np.concatenate(Ws), "H": Ht.T.copy(), "n_iter": n_iter, "violations": ratios,
            "violation_init": violation_init, "bounds": bounds}
