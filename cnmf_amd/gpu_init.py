"""GPU NNDSVD / NNDSVDA / NNDSVDAR initialisation.

sklearn's default init for k <= min(N, F) is NNDSVDA (SK:296-300) over
`randomized_svd(X, k, random_state)` (extmath.py:530-604).  The host restatement
(`cnmf_amd.init`) reproduces it bit for bit but costs seconds at cfg2's 1e6 x 81 (two passes of
X @ Q and X.T @ Q per power iteration, plus an N x 14 LU each time).  Here the passes over X run on
the GPU (libcnmf_hip.so, cnmf_init_*), and only F- and r-sized algebra stays on the host:

1. C = XᵀX and the column sums of X, fp64, ONE pass (cnmf_init_gram + cnmf_reduce_partials).
2. The range finder (extmath.py:287-357) in Gram form: sklearn alternates Q <- lu(X Q),
   Q <- lu(Xᵀ Q); only span(Q) enters the result, and span(Xᵀ X Z) = span(C Z).  So with the
   same Gaussian draw Ω (F x r, r = k + 10, drawn from the same RandomState and rounded to X's
   dtype as sklearn does) Z <- qr(C Z) for the same n_iter ('auto': 7 or 4).
3. The final Q = qr(X Z), B = Qᵀ X and svd(B) (extmath.py:576-590) without forming Q: with
   ZᵀCZ = V Λ Vᵀ, Q = X Z V Λ^-1/2 is an orthonormal basis of span(X Z), B = Λ^-1/2 Vᵀ Zᵀ C,
   and U = Q Uhat = X M with M = Z V Λ^-1/2 Uhat[:, :k] — ONE more pass (cnmf_init_xm).
   Directions with λ < 1e-14 λ_max (below fp64 resolution of the Gram form) are dropped.
4. svd_flip's u-based signs (extmath.py:900-953: the entry of largest |u| of each column, first
   occurrence) and the NNDSVD positive/negative part norms of U's columns: one pass over U
   (cnmf_init_stats); H and the choice of part per component on the host (SK:336-360).
5. W from U in one pass (cnmf_init_fill): |u| for j = 0, lbd · part / ‖part‖ otherwise,
   < eps -> 0, NNDSVDA's zeros -> X.mean() (SK:362-366).  NNDSVDAR's random fill of W's zeros in
   C order (SK:367-371) is done on the host copy of W (N x k), then W goes back to the device.

The four passes sit behind one small object (`_DevicePasses`: gram, xm, stats, fill); the host
algebra (`_nndsvd`) and the cross-workgroup combine of the stats rows (`_combine_stats`) see only
that object, so tests/test_gpu_init_algebra_cpu.py runs the same algebra over NumPy passes.

Rank-deficient X: when rank(X) < k the directions dropped in step 3 leave S[j] = 0, V[j] = 0 and
U[:, j] = 0.  A component whose chosen part has zero norm (in U or in V) contributes zeros to W and
H, with no division; the `< eps -> 0 -> fill` rule then gives it X.mean() (NNDSVDA), the random
fill (NNDSVDAR) or zeros (NNDSVD), which is what sklearn arrives at from its noise-level
components.  An all-zero X keeps no direction at all and yields the fill everywhere.

Agreement with sklearn (tests/test_gpu_init.py, tests/golden/init_*.npz): the result is the same
randomized SVD up to floating point; with fp64 X the GPU init matches sklearn to ~1e-9 when the
k-th singular value of X is above ~1e-6 of the first (the Gram form squares the condition of the
trailing directions; components below X's rounding level are noise in any implementation).  With
fp32 X sklearn computes the whole SVD in fp32, so the two differ at fp32 rounding (~1e-6).
"""
from __future__ import annotations

from math import sqrt

import numpy as np
import torch
from scipy import linalg

from . import _lib
from ._lib import check
from .init import _check_random_state

__all__ = ["gpu_init_eligible", "initialize_nmf_gpu", "GPU_INIT_MAX_FEATURES", "GPU_INIT_MAX_K"]

GPU_INIT_MAX_FEATURES = 96
GPU_INIT_MAX_K = 16
_XDT = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.bfloat16: _lib.BF16}


def gpu_init_eligible(n_samples: int, n_features: int, k: int, init, dtype) -> bool:
    """The GPU path serves the NNDSVD family for N >= F (sklearn's non-transposed branch),
    F <= 96, k <= 16, fp32 / fp64 / bf16 X."""
    return (init in ("nndsvd", "nndsvda", "nndsvdar") and n_samples >= n_features
            and n_features <= GPU_INIT_MAX_FEATURES and 1 <= k <= min(GPU_INIT_MAX_K, n_features)
            and dtype in _XDT)


def _ptr(t):
    return t.data_ptr()


def _reduce(lib, parts, n_rows, n_out, dev, stream):
    out = torch.empty(n_out, dtype=torch.float64, device=dev)
    stage = torch.zeros(int(lib.cnmf_stage_doubles(n_out)), dtype=torch.float64, device=dev)
    counter = torch.zeros(int(lib.cnmf_counter_words()), dtype=torch.int32, device=dev)
    check(lib.cnmf_reduce_partials(_ptr(parts), n_rows, n_out, _ptr(stage), _ptr(counter), _ptr(out),
                                   stream), "cnmf_reduce_partials")
    return out


class _DevicePasses:
    """The four passes over X / U on the device (libcnmf_hip.so, cnmf_init_*).  `_nndsvd` below sees
    them only through gram / xm / stats / fill (and the host copy of W for NNDSVDAR), so the same
    algebra runs over any object with these methods (tests/gpu_init_ref.py: NumPy fp64)."""

    def __init__(self, lib, X, stream):
        self.lib, self.X, self.stream = lib, X, stream
        self.dev = X.device
        self.xdt = _XDT[X.dtype]
        self.N, self.F = (int(v) for v in X.shape)

    def gram(self):
        """(XᵀX as F x F, the column sums of X), fp64 on the host."""
        lib, N, F, dev = self.lib, self.N, self.F, self.dev
        g = int(check(lib.cnmf_init_gram_rows(N), "cnmf_init_gram_rows"))
        n_out = F * F + F
        parts = torch.empty((g, n_out), dtype=torch.float64, device=dev)
        check(lib.cnmf_init_gram(_ptr(self.X), self.xdt, N, F, _ptr(parts), g, self.stream), "cnmf_init_gram")
        o = _reduce(lib, parts, g, n_out, dev, self.stream).cpu().numpy()
        del parts
        return o[:F * F].reshape(F, F), o[F * F:]

    def xm(self, M):
        """U = X M (N x k fp64), kept where the passes run."""
        k = M.shape[1]
        Md = torch.from_numpy(np.ascontiguousarray(M)).to(self.dev)
        U = torch.empty((self.N, k), dtype=torch.float64, device=self.dev)
        check(self.lib.cnmf_init_xm(_ptr(self.X), self.xdt, self.N, self.F, k, _ptr(Md), _ptr(U), self.stream),
              "cnmf_init_xm")
        return U

    def stats(self, U):
        """The per-workgroup rows of cnmf_init_stats as a host array (rows, k, 5)."""
        lib, N = self.lib, self.N
        k = int(U.shape[1])
        gs = int(check(lib.cnmf_init_stats_rows(N), "cnmf_init_stats_rows"))
        st = torch.empty((gs, k * 5), dtype=torch.float64, device=self.dev)
        check(lib.cnmf_init_stats(_ptr(U), N, k, _ptr(st), gs, self.stream), "cnmf_init_stats")
        return st.cpu().numpy().reshape(gs, k, 5)

    def fill(self, U, coef, part, sign, eps, fill, np_dt):
        """W (N x k, np_dt) from U, kept where the passes run."""
        k = int(U.shape[1])
        wdt = _lib.F64 if np_dt == np.float64 else _lib.F32
        W = torch.empty((self.N, k), dtype=torch.float64 if np_dt == np.float64 else torch.float32,
                        device=self.dev)
        cd = torch.from_numpy(coef).to(self.dev)
        pd = torch.from_numpy(part).to(self.dev)
        sd = torch.from_numpy(sign).to(self.dev)
        check(self.lib.cnmf_init_fill(_ptr(U), self.N, k, _ptr(cd), _ptr(pd), _ptr(sd), float(eps), float(fill),
                                      _ptr(W), wdt, self.stream), "cnmf_init_fill")
        return W

    def w_to_host(self, W):
        return W.cpu().numpy()

    def w_from_host(self, W, Wh):
        W.copy_(torch.from_numpy(Wh))


def _combine_stats(st):
    """The workgroup rows of cnmf_init_stats (rows, k, 5) into per-column (Σ max(u,0)², Σ min(u,0)²,
    max |u|, the u attaining it, its row): the sums add up; of the rows' maxima the largest wins,
    between equal ones the lower row (np.argmax's first occurrence, as svd_flip takes it)."""
    gs, k = st.shape[0], st.shape[1]
    sp = st[:, :, 0].sum(axis=0)
    sn = st[:, :, 1].sum(axis=0)
    best, val, row = np.full(k, -1.0), np.zeros(k), np.zeros(k)
    for j in range(k):
        for b in range(gs):
            m, v, i = st[b, j, 2], st[b, j, 3], st[b, j, 4]
            if m > best[j] or (m == best[j] and i < row[j]):
                best[j], val[j], row[j] = m, v, i
    return sp, sn, best, val, row


def _nndsvd(p, N, F, k, init, eps, random_state, np_dt):
    """Steps 1-5 of the module docstring over the passes `p`.  W comes back as `p.fill` made it, H
    as a NumPy array of np_dt."""
    # 1. C = XᵀX and the column sums (one pass over X)
    C, colsum = p.gram()
    C = 0.5 * (C + C.T)
    avg = float(colsum.sum() / (N * F))  # X.mean() (sklearn: in X's dtype)

    # 2. the range finder in Gram form (extmath.py:287-357), same draw as sklearn
    rs = _check_random_state(random_state)
    r = k + 10
    n_iter = 7 if k < 0.1 * min(N, F) else 4
    Om = rs.normal(size=(F, r))
    if np_dt == np.float32:
        Om = Om.astype(np.float32)
    Z = Om.astype(np.float64)
    for _ in range(n_iter):
        Z, _ = linalg.qr(C @ Z, mode="economic")
    # 3. Q = X Z V Λ^-1/2 (never formed), B = Qᵀ X, svd(B), U = X M
    lam, Vy = linalg.eigh(Z.T @ C @ Z)
    keep = lam > lam.max() * 1e-14
    M = np.zeros((F, k))
    S = np.zeros(k)
    V = np.zeros((k, F))
    if keep.any():  # an all-zero X keeps no direction: every component stays zero
        T = Vy[:, keep] / np.sqrt(lam[keep])
        B = T.T @ (Z.T @ C)
        Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
        kk = min(k, Uhat.shape[1])
        M[:, :kk] = Z @ T @ Uhat[:, :kk]
        S[:kk] = s[:kk]
        V[:kk] = Vt[:kk]
    U = p.xm(M)

    # 4. signs (svd_flip, u-based) and the part norms of U's columns
    sp, sn, _, val, _ = _combine_stats(p.stats(U))
    sign = np.where(val != 0, np.sign(val), 1.0)
    V = V * sign[:, None]
    pos = np.where(sign > 0, sp, sn)  # ‖max(sign·u, 0)‖²
    neg = np.where(sign > 0, sn, sp)

    # NNDSVD (SK:336-360): per component the part of (u, v) with the larger norm product
    H = np.zeros((k, F))
    coef = np.zeros(k)
    part = np.zeros(k, dtype=np.int32)
    coef[0] = sqrt(S[0])
    H[0] = sqrt(S[0]) * np.abs(V[0])
    for j in range(1, k):
        y = V[j]
        y_p, y_n = np.maximum(y, 0), np.abs(np.minimum(y, 0))
        x_p_nrm, x_n_nrm = sqrt(pos[j]), sqrt(neg[j])
        y_p_nrm, y_n_nrm = sqrt(float(np.dot(y_p, y_p))), sqrt(float(np.dot(y_n, y_n)))
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            nrm, y_part, y_nrm, sigma, part[j] = x_p_nrm, y_p, y_p_nrm, m_p, 1
        else:
            nrm, y_part, y_nrm, sigma, part[j] = x_n_nrm, y_n, y_n_nrm, m_n, 2
        if nrm > 0 and y_nrm > 0:  # else a dropped direction (rank(X) <= j): zeros in W and H
            lbd = sqrt(S[j] * sigma)
            coef[j] = lbd / nrm
            H[j] = lbd * (y_part / y_nrm)
    H = H.astype(np_dt)
    H[H < eps] = 0

    # 5. W (one pass over U), the NNDSVDA / NNDSVDAR fills
    fill = avg if init == "nndsvda" else 0.0
    W = p.fill(U, coef, part, sign, eps, fill, np_dt)
    del U
    avg_x = np_dt(avg)
    if init == "nndsvda":
        H[H == 0] = avg_x
    elif init == "nndsvdar":
        rng = _check_random_state(random_state)
        Wh = p.w_to_host(W)
        Wh[Wh == 0] = abs(avg_x * rng.standard_normal(size=len(Wh[Wh == 0])) / 100)
        H[H == 0] = abs(avg_x * rng.standard_normal(size=len(H[H == 0])) / 100)
        p.w_from_host(W, Wh)
    return W, H


def initialize_nmf_gpu(X: torch.Tensor, n_components: int, init: str = "nndsvda", eps: float = 1e-6,
                       random_state=None):
    """(W, H) for the NNDSVD family from X (N x F, on a HIP device).  W: device tensor of X's
    compute dtype (fp64 for fp64 X, else fp32); H: NumPy array of the same dtype."""
    if X.device.type != "cuda":
        raise _lib.HipLibraryError("initialize_nmf_gpu needs X on a HIP device")
    N, F = (int(v) for v in X.shape)
    k = int(n_components)
    if not gpu_init_eligible(N, F, k, init, X.dtype):
        raise ValueError(f"GPU init does not serve init={init!r} for X {N}x{F} {X.dtype} k={k}")
    lib = _lib.load()
    dev = X.device
    X = X.contiguous()
    np_dt = np.float64 if X.dtype == torch.float64 else np.float32
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        W, H = _nndsvd(_DevicePasses(lib, X, stream), N, F, k, init, eps, random_state, np_dt)
        torch.cuda.current_stream(dev).synchronize()
    return W, H
