"""Plain NumPy restatements of the four GPU NNDSVD passes (cnmf_amd/csrc/init.hip: cnmf_init_gram,
_xm, _stats, _fill).  No torch.

`NumpyPasses` has the methods of `cnmf_amd.gpu_init._DevicePasses`, so `cnmf_amd.gpu_init._nndsvd`
(the product's host algebra, not a copy) runs over it without a GPU
(tests/test_gpu_init_algebra_cpu.py).  The `*_ref` functions are the per-launch references of
tests/test_gpu_init_kernels.py: they return the value in extended precision together with the
magnitude that the rounding bound of the operation scales with.

Bars (u = 2^-53, the unit roundoff of fp64): a sum of n products accumulated in any order, each
step rounded once, is within n·u·Σ|terms| of the exact sum (Higham, Accuracy and Stability of
Numerical Algorithms, §3.1, to first order in u).  The references are taken in np.longdouble, whose
own error (2^-64 per step where it is the x87 format) is far below that; where np.longdouble is
plain fp64 the bars double (`BAR_SCALE`)."""
import numpy as np

U_FP64 = 2.0 ** -53
LD = np.longdouble
BAR_SCALE = 1.0 if np.finfo(LD).eps < 2.0 ** -52 else 2.0
BLOCK_ROWS = 4096  # init.hip ig_blocks: at least 4096 rows per workgroup


def bf16_round(x):
    """fp32 values rounded to the nearest bf16 (ties to even), returned as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def block_rows(n_rows, max_blocks=None):
    """(workgroups, rows per workgroup) of cnmf_init_gram / cnmf_init_stats for n_rows (ig_blocks:
    ceil(N / 4096), at most 2 x the compute units and 1024)."""
    g = (n_rows + BLOCK_ROWS - 1) // BLOCK_ROWS
    if max_blocks is not None:
        g = min(g, max_blocks)
    g = max(1, min(g, 1024))
    return g, (n_rows + g - 1) // g


# ---- per-launch references ------------------------------------------------------------------------
def gram_ref(X):
    """(XᵀX, column sums, |X|ᵀ|X|, Σ|x| per column) of X upcast exactly, in np.longdouble."""
    Xl = np.asarray(X).astype(LD)
    C, s = Xl.T @ Xl, Xl.sum(axis=0)
    if Xl.min() >= 0:
        return C, s, C, s
    A = np.abs(Xl)
    return C, s, A.T @ A, A.sum(axis=0)


def xm_ref(X, M):
    """(X·M, Σ_f |x_f·m_fj|) in np.longdouble."""
    Xl, Ml = np.asarray(X).astype(LD), np.asarray(M).astype(LD)
    return Xl @ Ml, np.abs(Xl) @ np.abs(Ml)


def stats_ref(U):
    """Per column of U: (Σ max(u,0)², Σ min(u,0)² in np.longdouble, max |u|, the u at its first
    occurrence, that row) — the last three exactly as np.argmax(abs(u)) has them."""
    Ul = np.asarray(U).astype(LD)
    sp = (np.maximum(Ul, 0) ** 2).sum(axis=0)
    sn = (np.minimum(Ul, 0) ** 2).sum(axis=0)
    row = np.argmax(np.abs(U), axis=0)
    val = U[row, np.arange(U.shape[1])]
    return sp, sn, np.abs(val), val, row


def fill_ref(U, coef, part, sgn, eps, fill, dtype):
    """W from U as ig_fill_kernel states it: v = coef_j · part_j(sgn_j · u), v < eps -> 0, v == 0 ->
    fill, cast to dtype.  One fp64 multiply and one cast: bit-equal to the kernel."""
    u = np.asarray(sgn, dtype=np.float64)[None, :] * np.asarray(U, dtype=np.float64)
    part = np.asarray(part)[None, :]
    p = np.where(part == 0, np.abs(u), np.where(part == 1, np.where(u > 0, u, 0.0), np.where(u < 0, -u, 0.0)))
    v = np.asarray(coef, dtype=np.float64)[None, :] * p
    v[v < eps] = 0.0
    v[v == 0] = fill
    return v.astype(dtype)


# ---- the four passes for cnmf_amd.gpu_init._nndsvd ------------------------------------------------------
class NumpyPasses:
    """The passes of `cnmf_amd.gpu_init._DevicePasses` in NumPy fp64.  X: the values the device
    would read (bf16 X: fp32 holding bf16-representable values).  The stats rows come in the
    device's layout, one row per block of `block_rows(N)` rows, so `_combine_stats` has work to do."""

    def __init__(self, X):
        self.X = np.asarray(X).astype(np.float64)
        self.N, self.F = self.X.shape

    def gram(self):
        return self.X.T @ self.X, self.X.sum(axis=0)

    def xm(self, M):
        return self.X @ M

    def stats(self, U):
        g, rpb = block_rows(self.N)
        k = U.shape[1]
        st = np.zeros((g, k, 5))
        for b in range(g):
            Ub = U[b * rpb:(b + 1) * rpb]
            st[b, :, 0] = (np.maximum(Ub, 0) ** 2).sum(axis=0)
            st[b, :, 1] = (np.minimum(Ub, 0) ** 2).sum(axis=0)
            if len(Ub) == 0:  # a workgroup without rows: the kernel's start values
                st[b, :, 2] = -1.0
                continue
            row = np.argmax(np.abs(Ub), axis=0)
            val = Ub[row, np.arange(k)]
            st[b, :, 2], st[b, :, 3], st[b, :, 4] = np.abs(val), val, row + b * rpb
        return st

    def fill(self, U, coef, part, sign, eps, fill, np_dt):
        return fill_ref(U, coef, part, sign, eps, fill, np_dt)

    def w_to_host(self, W):
        return W

    def w_from_host(self, W, Wh):
        if W is not Wh:
            W[...] = Wh


_EDGE = {}


def edge_cases():
    """The edge shapes shared by the CPU algebra test and the device end-to-end test, made once:
    name -> (X as the device reads it [bf16: fp32 holding bf16 values], k, kind, bar).  Drawn from one
    RandomState(5) in this order.  N: a ragged last 64-row tile everywhere, more than one workgroup
    (N > 4096) and more than two (8200); F at and next to the 96-wide register tiling and 1; k with
    idle component groups (1, 3), one group doing two components (5) and all four doing four (16)."""
    if _EDGE:
        return _EDGE
    from cnmf_amd.synthetic import iop_spectra
    rs = np.random.RandomState(5)
    _EDGE["333x5_k3_f64"] = (rs.rand(333, 5), 3, "f64", 1e-8)
    _EDGE["65x1_k1_f64"] = (rs.rand(65, 1), 1, "f64", 1e-8)
    _EDGE["4161x96_k16_f32"] = (rs.rand(4161, 96).astype(np.float32), 16, "f32", 2e-5)
    _EDGE["4097x17_k5_f32"] = (rs.rand(4097, 17).astype(np.float32), 5, "f32", 2e-5)
    _EDGE["8200x81_k4_bf16"] = (bf16_round(iop_spectra(8200, 81, seed=5, dtype=np.float32)), 4, "bf16", 2e-5)
    _EDGE["4161x95_k16_bf16"] = (bf16_round(rs.rand(4161, 95).astype(np.float32)), 16, "bf16", 2e-5)
    return _EDGE


EDGE_NAMES = ["333x5_k3_f64", "65x1_k1_f64", "4161x96_k16_f32", "4097x17_k5_f32", "8200x81_k4_bf16",
              "4161x95_k16_bf16"]
_HOST = {}


def edge_host(name, init):
    """The host restatement (sklearn's arithmetic) on the case's values in fp64, made once."""
    if (name, init) not in _HOST:
        from cnmf_amd.init import initialize_nmf
        X, k, _, _ = edge_cases()[name]
        _HOST[name, init] = initialize_nmf(X.astype(np.float64), k, init=init, random_state=0)
    return _HOST[name, init]


def rank2_x(n_rows=500):
    """A @ B with A = rand(n_rows, 2), B = rand(2, 7) from one RandomState(0): rank 2, fp64."""
    rs = np.random.RandomState(0)
    A = rs.rand(n_rows, 2)
    return A @ rs.rand(2, 7)


def check_rank2(W, H, Wh, Hh, X, init):
    """The rank-2 X with k = 4: finite and >= 0; components 0 and 1 as the host restatement has
    them (1e-8); components 2 and 3 the fill everywhere."""
    from golden_io import rel_fro
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    assert np.all(W >= 0) and np.all(H >= 0)
    ew, eh = rel_fro(W[:, :2], Wh[:, :2]), rel_fro(H[:2], Hh[:2])
    print(f"rank-2 {init}: rel W[:, :2] {ew:.2e} rel H[:2] {eh:.2e}")
    assert ew <= 1e-8 and eh <= 1e-8, (ew, eh)
    avg = X.mean()
    for tail in (W[:, 2:], H[2:]):
        if init == "nndsvda":
            # one value everywhere: X.mean() up to the order of summation (two sums of X.size
            # non-negative terms, each within X.size·u of the exact one)
            assert np.all(tail == tail.flat[0])
            assert abs(tail.flat[0] - avg) <= 2 * X.size * U_FP64 * avg
        elif init == "nndsvd":
            assert np.all(tail == 0)
        else:
            assert np.all(tail > 0) and np.all(tail <= abs(avg))


def nndsvd_numpy(X, k, init="nndsvda", eps=1e-6, random_state=None, np_dt=None):
    """(W, H) of the GPU init's algebra over the NumPy passes.  np_dt: the compute dtype the device
    path would use (fp64 for fp64 X, else fp32)."""
    from cnmf_amd.gpu_init import _nndsvd
    X = np.asarray(X)
    if np_dt is None:
        np_dt = np.float64 if X.dtype == np.float64 else np.float32
    return _nndsvd(NumpyPasses(X), X.shape[0], X.shape[1], int(k), init, eps, random_state, np_dt)
