"""GPU: the four NNDSVD init passes (cnmf_amd/csrc/init.hip: cnmf_init_gram, _xm, _stats, _fill) one
launch at a time through the C ABI, each against its restatement in tests/gpu_init_ref.py, and the
device init end to end at the edge shapes of tests/test_gpu_init_algebra_cpu.py.

Every output buffer starts as NaN with guard rows behind the rows the pass owns: every owned
element must have been written, no guard element may have been.  X lies in [0.1, 1), so one dropped
or repeated row moves a sum by about 1/N of it, far more than the bars.

Bars (u = 2^-53; gpu_init_ref's docstring): the rounding bounds of the operation with the
reference in np.longdouble, not measured figures —
  gram   |err C_ab| <= N·u·(|X|ᵀ|X|)_ab, |err colsum_a| <= N·u·Σ|x_a|; C exactly symmetric
  xm     |err U_nj| <= (F+1)·u·Σ_f |x_nf·m_fj|
  stats  |err Σ±| <= N·u·Σu²; max |u|, its value and its row exactly np.argmax(abs(u))
  fill   bit-equal (one fp64 multiply, one cast)
Each test prints its largest error / bound."""
import numpy as np
import pytest

from golden_io import rel_fro
from gpu_init_ref import (BAR_SCALE, EDGE_NAMES, LD, U_FP64, NumpyPasses, bf16_round, check_rank2, edge_cases,
                          edge_host, fill_ref, gram_ref, rank2_x, stats_ref, xm_ref)

pytestmark = pytest.mark.gpu

GUARD = 3
KINDS = ("f32", "f64", "bf16")


def _ptr(t):
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _xdt(kind):
    from cnmf_amd import _lib
    return {"f32": _lib.F32, "f64": _lib.F64, "bf16": _lib.BF16}[kind]


def _make_x(rs, N, F, kind):
    """X in [0.1, 1) as the device will read it (bf16: fp32 holding bf16 values).  The fp64 values
    are not fp32-representable: a pass staging them through fp32 is 1e-8 off, not 1e-16."""
    X = rs.uniform(0.1, 0.99, size=(N, F))
    if kind == "f64":
        assert np.all(X != X.astype(np.float32))
        return X
    X = X.astype(np.float32)
    return bf16_round(X) if kind == "bf16" else X


def _to_dev(X, kind):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    if kind == "bf16":
        t = t.to(torch.bfloat16)
        assert np.array_equal(t.float().cpu().numpy(), X)  # the cast was exact
    return t


def _nan_buf(rows, cols, dtype=None):
    import torch
    return torch.full((rows, cols), float("nan"), dtype=dtype or torch.float64, device="cuda")


def _owned_and_guard(buf, rows):
    """Host copy of the first `rows` rows; they are all written, the rows behind them untouched."""
    import torch
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert not np.isnan(h[:rows]).any(), "an owned element was not written"
    assert np.isnan(h[rows:]).all(), "a guard element was written"
    return h[:rows]


def _ratio(got, ref, bound):
    """max |got - ref| / bound after asserting |got - ref| <= bound everywhere."""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    bound = np.asarray(bound) * BAR_SCALE
    assert np.all(err <= bound), float((err - bound).max())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- cnmf_init_gram + cnmf_reduce_partials --------------------------------------------------------------
_GRAM_N = (1, 63, 64, 65, 4096, 4097, 12293)
_GRAM_F = (1, 17, 81, 95, 96)
_GRAM_SHAPES = ([(n, 96) for n in _GRAM_N] + [(4097, f) for f in _GRAM_F if f != 96]
                + [(65, 17), (12293, 81)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,F", _GRAM_SHAPES)
def test_gram(N, F, kind):
    import torch
    from cnmf_amd._lib import check, load
    lib = load()
    X = _make_x(np.random.RandomState(N * 101 + F), N, F, kind)
    Xd = _to_dev(X, kind)
    g = int(check(lib.cnmf_init_gram_rows(N), "cnmf_init_gram_rows"))
    assert g == max(1, min((N + 4095) // 4096, 2 * _cus(), 1024))
    n_out = F * F + F
    extra = 2  # n_parts beyond the rows the pass needs: left alone
    parts = _nan_buf(g + extra + GUARD, n_out)
    check(lib.cnmf_init_gram(_ptr(Xd), _xdt(kind), N, F, _ptr(parts), g + extra, _stream()), "cnmf_init_gram")
    _owned_and_guard(parts, g)
    out = _nan_buf(1, n_out + GUARD)
    stage = torch.zeros(int(lib.cnmf_stage_doubles(n_out)), dtype=torch.float64, device="cuda")
    counter = torch.zeros(int(lib.cnmf_counter_words()), dtype=torch.int32, device="cuda")
    check(lib.cnmf_reduce_partials(_ptr(parts), g, n_out, _ptr(stage), _ptr(counter), _ptr(out), _stream()),
          "cnmf_reduce_partials")
    o = _owned_and_guard(out.reshape(-1, 1), n_out)[:, 0]
    C, cs = o[:F * F].reshape(F, F), o[F * F:]
    Cr, csr, Ca, csa = gram_ref(X)
    rc = _ratio(C, Cr, N * U_FP64 * Ca)
    rs_ = _ratio(cs, csr, N * U_FP64 * csa)
    print(f"gram N={N} F={F} {kind}: err/bound C {rc:.3f} colsum {rs_:.3f}")
    assert np.array_equal(C, C.T)


@pytest.mark.parametrize("N", [65, 4097, 12293])
def test_gram_refuses_too_few_partial_rows(N):
    from cnmf_amd._lib import HipLibraryError, check, load
    lib = load()
    Xd = _to_dev(_make_x(np.random.RandomState(0), N, 17, "f32"), "f32")
    g = int(lib.cnmf_init_gram_rows(N))
    parts = _nan_buf(g + GUARD, 17 * 17 + 17)
    with pytest.raises(HipLibraryError):
        check(lib.cnmf_init_gram(_ptr(Xd), _xdt("f32"), N, 17, _ptr(parts), g - 1, _stream()), "cnmf_init_gram")
    _owned_and_guard(parts, 0)  # nothing was launched


# ---- cnmf_init_xm ---------------------------------------------------------------------------------------
_XM_K = (1, 3, 4, 5, 16)


def _xm_once(lib, rs, N, F, k, kind):
    import torch
    from cnmf_amd._lib import check
    X = _make_x(rs, N, F, kind)
    M = rs.standard_normal((F, k))  # mixed signs: the bound scales with Σ|x·m|, not with |u|
    Xd, Md = _to_dev(X, kind), torch.from_numpy(M).cuda()
    U = _nan_buf(N + GUARD, k)
    check(lib.cnmf_init_xm(_ptr(Xd), _xdt(kind), N, F, k, _ptr(Md), _ptr(U), _stream()), "cnmf_init_xm")
    Uh = _owned_and_guard(U, N)
    Ur, Ua = xm_ref(X, M)
    return _ratio(Uh, Ur, (F + 1) * U_FP64 * Ua)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", [1, 17, 81, 96])
def test_xm(F, kind):
    from cnmf_amd._lib import load
    lib = load()
    rs = np.random.RandomState(F * 7 + len(kind))
    worst = 0.0
    for N in (1, 63, 65, 4097):
        for k in _XM_K:
            worst = max(worst, _xm_once(lib, rs, N, F, k, kind))
    print(f"xm F={F} {kind}: err/bound {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
def test_xm_grid_stride_wraps(kind):
    """More 64-row tiles than workgroups (4 per compute unit) plus a one-row last tile: the first
    workgroups take a second tile, the very first one the ragged one."""
    from cnmf_amd._lib import load
    lib = load()
    N = 64 * (4 * _cus() + 1) + 1
    rs = np.random.RandomState(17 + len(kind))
    worst = max(_xm_once(lib, rs, N, 17, k, kind) for k in (5, 16))
    print(f"xm wrap N={N} F=17 {kind}: err/bound {worst:.3f}")


# ---- cnmf_init_stats + _combine_stats -------------------------------------------------------------------
def _stats_once(lib, U):
    """(device rows (g, k, 5), combined) for U; the rows must be the blocks' own NumPy answers."""
    import torch
    from cnmf_amd._lib import check
    from cnmf_amd.gpu_init import _combine_stats
    N, k = U.shape
    Ud = torch.from_numpy(np.ascontiguousarray(U)).cuda()
    g = int(check(lib.cnmf_init_stats_rows(N), "cnmf_init_stats_rows"))
    st = _nan_buf(g + GUARD, k * 5)
    check(lib.cnmf_init_stats(_ptr(Ud), N, k, _ptr(st), g, _stream()), "cnmf_init_stats")
    st = _owned_and_guard(st, g).reshape(g, k, 5)
    if g == (N + 4095) // 4096:  # not capped by the device's size: the layout gpu_init_ref restates
        assert np.array_equal(st[:, :, 2:], NumpyPasses(np.zeros((N, 1))).stats(U)[:, :, 2:])
    sp, sn, best, val, row = _combine_stats(st)
    rsp, rsn, rbest, rval, rrow = stats_ref(U)
    assert np.array_equal(best, rbest) and np.array_equal(val, rval) and np.array_equal(row, rrow)
    assert np.array_equal(np.signbit(val), np.signbit(rval))
    bound = N * U_FP64 * (rsp + rsn)
    return max(_ratio(sp, rsp, bound), _ratio(sn, rsn, bound)), (best, val, row)


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("N", [1, 255, 257, 4097, 8200])
def test_stats(N, k):
    from cnmf_amd._lib import load
    U = np.random.RandomState(N + k).standard_normal((N, k))
    r, _ = _stats_once(load(), U)
    print(f"stats N={N} k={k}: err/bound {r:.3f}")


def test_stats_planted_columns():
    """Equal |u| of opposite signs at rows 5 and 261 (one thread, two strides) and 5000 (another
    workgroup): row 5 with its sign; an all-zero column; an all-negative column; the maximum in the
    last row; the same tie with only the far workgroup's row positive."""
    from cnmf_amd._lib import check, load
    lib = load()
    N, k = 8200, 6
    assert int(check(lib.cnmf_init_stats_rows(N), "cnmf_init_stats_rows")) == 3
    U = np.random.RandomState(3).uniform(-1, 1, size=(N, k))
    U[[5, 261, 5000], 0] = [-3.0, 3.0, 3.0]
    U[:, 1] = 0.0
    U[:, 2] = -np.abs(U[:, 2]) - 1e-3
    U[N - 1, 3] = 5.0
    U[[5, 261, 5000], 4] = [3.0, -3.0, -3.0]
    r, (best, val, row) = _stats_once(lib, U)
    print(f"stats planted: err/bound {r:.3f}")
    assert (row[0], val[0], best[0]) == (5, -3.0, 3.0)
    assert (row[1], val[1], best[1]) == (0, 0.0, 0.0)
    assert val[2] < 0 and row[2] == np.argmax(-U[:, 2])
    assert (row[3], val[3]) == (N - 1, 5.0)
    assert (row[4], val[4]) == (5, 3.0)


# ---- cnmf_init_fill -------------------------------------------------------------------------------------
EPS = 1e-6


def _fill_once(lib, rs, N, k, wkind, fill, shift, flip):
    import torch
    from cnmf_amd import _lib
    from cnmf_amd._lib import check
    part = ((np.arange(k) + shift) % 3).astype(np.int32)
    sgn = np.where(np.arange(k) % 2 == 0, 1.0, -1.0) * flip
    coef = np.where(np.arange(k) % 2 == 0, 1.0, rs.uniform(0.2, 3.0, size=k))
    U = rs.standard_normal((N, k)) * 3e-6  # values on both sides of eps, both signs
    below = np.nextafter(EPS, 0.0)
    if N >= 6:
        live = sgn * np.where(part == 2, -1.0, 1.0)  # the sign of u that its column's part keeps
        U[0], U[1] = live * EPS / coef, live * below / coef  # coef·p exactly eps / one ulp below (coef = 1)
        U[2], U[3] = -live * 1.0, 0.0  # the part's dead side (part 0: kept), and zero
        U[4], U[5] = -0.0, live * 1.0
    dt, wdt = (torch.float32, _lib.F32) if wkind == "f32" else (torch.float64, _lib.F64)
    np_dt = np.float32 if wkind == "f32" else np.float64
    Ud = torch.from_numpy(U).cuda()
    cd, pd, sd = (torch.from_numpy(a).cuda() for a in (coef, part, sgn))
    W = _nan_buf(N + GUARD, k, dt)
    check(lib.cnmf_init_fill(_ptr(Ud), N, k, _ptr(cd), _ptr(pd), _ptr(sd), EPS, fill, _ptr(W), wdt, _stream()),
          "cnmf_init_fill")
    Wh = _owned_and_guard(W, N)
    ref = fill_ref(U, coef, part, sgn, EPS, fill, np_dt)
    bits = np.uint32 if wkind == "f32" else np.uint64
    assert np.array_equal(np.ascontiguousarray(Wh).view(bits), ref.view(bits))
    if N >= 6:  # the planted rows do what they are there for (the restatement's own check)
        unit = coef == 1.0
        assert np.all(ref[0, unit] == np_dt(EPS)) and np.all(ref[1, unit] == np_dt(fill))
        assert np.all(ref[2, part != 0] == np_dt(fill)) and np.all(ref[2, part == 0] == coef[part == 0].astype(np_dt))
        assert np.all(ref[3] == np_dt(fill)) and np.all(ref[4] == np_dt(fill)) and np.all(ref[5] == coef.astype(np_dt))


@pytest.mark.parametrize("fill", [0.0, 0.123456789])
@pytest.mark.parametrize("wkind", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_fill(k, wkind, fill):
    from cnmf_amd._lib import load
    lib = load()
    rs = np.random.RandomState(k)
    for N in (1, 333):
        assert (N * k) % 256 != 0
        for shift in range(3):
            for flip in (1.0, -1.0):
                _fill_once(lib, rs, N, k, wkind, fill, shift, flip)


@pytest.mark.parametrize("wkind", ["f32", "f64"])
def test_fill_grid_stride_wraps(wkind):
    """N·k beyond 8 workgroups of 256 per compute unit: the first threads take a second element."""
    from cnmf_amd._lib import load
    k = 5
    N = 8 * _cus() * 256 // k + 77
    assert N * k > 8 * _cus() * 256 and (N * k) % 256 != 0
    _fill_once(load(), np.random.RandomState(9), N, k, wkind, 0.123456789, 1, -1.0)


# ---- end to end on the device -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_device_init_edge_shape(name):
    import torch
    from cnmf_amd.gpu_init import initialize_nmf_gpu
    X, k, kind, bar = edge_cases()[name]
    Xd = _to_dev(X, kind)
    assert Xd.dtype == {"f64": torch.float64, "f32": torch.float32, "bf16": torch.bfloat16}[kind]
    np_dt = np.float64 if kind == "f64" else np.float32
    for init in ("nndsvd", "nndsvda"):
        W, H = initialize_nmf_gpu(Xd, k, init=init, random_state=0)
        W = W.cpu().numpy()
        Wh, Hh = edge_host(name, init)
        assert W.dtype == np_dt and H.dtype == np_dt and W.shape == Wh.shape and H.shape == Hh.shape
        ew, eh = rel_fro(W, Wh), rel_fro(H, Hh)
        print(f"{name} {init}: rel W {ew:.2e} rel H {eh:.2e}")
        if init == "nndsvd":
            np.testing.assert_array_equal(W == 0, Wh == 0)
            np.testing.assert_array_equal(H == 0, Hh == 0)
        assert ew <= bar and eh <= bar, (ew, eh)


@pytest.mark.parametrize("init", ["nndsvd", "nndsvda", "nndsvdar"])
def test_device_init_rank_deficient(init):
    import torch
    from cnmf_amd.gpu_init import initialize_nmf_gpu
    from cnmf_amd.init import initialize_nmf
    X = rank2_x()
    W, H = initialize_nmf_gpu(torch.from_numpy(X).cuda(), 4, init=init, random_state=0)
    Wh, Hh = initialize_nmf(X, 4, init=init, random_state=0)
    check_rank2(W.cpu().numpy(), H, Wh, Hh, X, init)


def test_factorise_rank_deficient_tall_x_is_finite():
    """The default route of a tall fp64 X (init=None, init_device='auto': the GPU init) on a
    noise-free two-endmember mixture with k = 4."""
    import cnmf_amd
    from cnmf_amd import api
    X = rank2_x(api.GPU_INIT_MIN_ROWS)
    assert X.shape == (65536, 7) and X.dtype == np.float64
    W, H, n = cnmf_amd.factorise(X, n_components=4, max_iter=5, tol=0)
    assert n == 5 and W.shape == (65536, 4) and H.shape == (4, 7)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(W >= 0) and np.all(H >= 0)
