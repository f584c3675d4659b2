"""GPU: every kernel the MU pass dispatch can choose (tests/pass_cases.py, completeness checked by
test_pass_dispatch_cpu.py), one launch each through MUPlan, element by element against NumPy fp64 on
the same (exactly representable) inputs.

Bars, derived from the arithmetic (u = 2⁻²⁴), not from what the kernels give:
  W   VALU pass, fp32 / bf16 X: 9u - phase 1 sums 7-term fp32 FMA chains of non-negative terms and
      folds them in fp64 (7u), one rounding of the fp64 w·num/den to fp32 (u), 1u of margin for the
      fp64 steps.  F = 81 matrix-core pass: (F + 2)u, its k-ordered fp32 chain over F.  fp64: 1e-12.
  AB  against Wgᵀ·X, Wgᵀ·Wg of the GPU's own new W in fp64, so W's error does not enter: one fp32
      accumulator holds at most T = 64·ceil(n_tiles / n_parts) non-negative terms: (T + 1)u; fp64 1e-12.
  loss  fp64 arithmetic on exact inputs: 1e-12 relative.
Each test prints its worst error / bar ratios (pytest -s).
"""
import zlib

import numpy as np
import pytest

import pass_cases as pc
from golden_io import rel_fro
from oracle import mu_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL32 = 1e-5  # the project's iteration bars (test_gpu_parity.py): relative Frobenius
TOL64 = 1e-9


def _torch_dtype(dt):
    import torch
    return {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}[dt]


def _plan(dt, X, W0, H0, k, **reg):
    """An MUPlan on X (fp64 array of values dt holds exactly) with W0 / H0 loaded."""
    import torch
    from cnmf_amd.solver import MUPlan
    Xt = torch.from_numpy(X if dt == "float64" else X.astype(np.float32)).to(_torch_dtype(dt))
    assert np.array_equal(Xt.double().numpy(), X)  # the device sees the reference's values
    plan = MUPlan(Xt.cuda(), k, **reg)
    plan.set_W(torch.from_numpy(W0))
    F = X.shape[1]
    if k > 4 and F > 512:
        # the pass takes these rows, the basis kernels behind set_H stop at F = 512 for k > 4
        # (test_refusals_are_clean): load what set_H derives, Ht = Hᵀ zero-padded to KP columns and
        # HHᵀ, so that the pass is run at its own widest F
        Ht, HHt = np.zeros((F, plan.KP)), np.zeros((plan.KP, plan.KP))
        Ht[:, :k], HHt[:k, :k] = H0.T, H0 @ H0.T
        plan.H64.copy_(torch.from_numpy(H0))
        plan.Ht.copy_(torch.from_numpy(Ht))
        plan.HHt.copy_(torch.from_numpy(HHt))
    else:
        plan.set_H(torch.from_numpy(H0))
    return plan


def _update_kernel(dt, F, k, N):
    from cnmf_amd import _lib
    st, text = pc.describe(dt, F, k, _lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE)
    assert st == 0
    return sorted(pc.kernels(text, N)), text


def _w_rtol(dt, F, kernel):
    if dt == "float64":
        return 1e-12
    fam = kernel.split("<")[0]
    assert fam in ("mu_pass_kernel", "mu_pass_mfma_kernel", "mu_pass_sl_kernel"), fam
    # the sample-lane kernel (full tiles of fp32 F = 81, k = 4; its parity is test_gpu_persistent.py's):
    # however it orders its fp32 sums over F terms, (F - 1)u + the final rounding bounds them
    return 9 * U if fam == "mu_pass_kernel" else (F + 2) * U


def _ratio(got, ref, rtol):
    """max |got - ref| / (rtol·|ref|): <= 1 passes assert_allclose(rtol=rtol, atol=0)."""
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (rtol * np.abs(ref)))  # rtol: scalar or per row
    return float(r.max()) if r.size else 0.0


def _one_pass(plan, dt, F, k, X, W0, H0, kernels, reg=(0.0, 0.0)):
    """UPDATE_W | ACCUMULATE + reduce on a NaN-filled partial buffer; W and AB against NumPy fp64."""
    import torch
    from cnmf_amd import _lib
    N = X.shape[0]
    plan.partials.fill_(float("nan"))
    plan.sample_pass(_lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE)
    plan.reduce(plan.n_out, plan.AB)
    torch.cuda.synchronize()
    Wg = plan.W.cpu().numpy().astype(np.float64)
    AB = plan.AB.cpu().numpy().reshape(k, F + k)
    assert np.isfinite(AB).all(), "a workgroup left part of its partial row unwritten"
    assert np.isfinite(Wg).all()
    Wref, _, _ = mu_ref.update_w(X, W0.copy(), H0, l1_reg_W=reg[0], l2_reg_W=reg[1])
    n_tiles = (N + 63) // 64
    T = 64 * -(-n_tiles // plan.n_parts)
    # per sample the bar of the kernel that updated it: the ragged tail has its own
    w_rtol = np.empty((N, 1))
    for role, kernel in kernels:
        rows = {"grid": slice(0, N), "full": slice(0, N // 64 * 64), "tail": slice(N // 64 * 64, N)}[role]
        w_rtol[rows] = _w_rtol(dt, F, kernel)
    ab_rtol = 1e-12 if dt == "float64" else (T + 1) * U
    A, B = Wg.T @ X, Wg.T @ Wg
    rw = _ratio(Wg, Wref, w_rtol)
    ra = max(_ratio(AB[:, :F], A, ab_rtol), _ratio(AB[:, F:], B, ab_rtol))
    print(f"PASSMATRIX {dt} F={F} k={k} N={N} {kernels} n_parts={plan.n_parts} T={T} "
          f"W err/bar={rw:.3f} AB err/bar={ra:.3f}")
    assert np.array_equal(Wg == 0, Wref == 0)  # zeros stay exact zeros, nothing else becomes one
    assert (np.abs(Wg - Wref) <= w_rtol * np.abs(Wref)).all(), f"W misses its bar: worst err/bar = {rw}"
    np.testing.assert_allclose(AB[:, :F], A, rtol=ab_rtol, atol=0)
    np.testing.assert_allclose(AB[:, F:], B, rtol=ab_rtol, atol=0)


@pytest.mark.parametrize("row", pc.ROWS, ids=pc.row_id)
def test_loss_then_one_pass_match_numpy(row):
    """(b) the loss pass on (W0, H0), then (a) one updating + accumulating pass, both on partial rows
    pre-filled with NaN.  A MULTI row gives every workgroup at least two tiles (asserted)."""
    import torch
    from cnmf_amd import _lib
    dt, F, k, N, _ = row
    if N == pc.MULTI:
        with torch.cuda.device(0):
            cap = int(_lib.load().cnmf_pass_blocks(64 * 10 ** 7, F, k, pc.xdt(dt)))
        assert cap > 0
        N = 64 * (2 * cap) + 37
        assert N * F * {"float32": 4, "float64": 8, "bfloat16": 2}[dt] < 100e6
    X, W0, H0 = pc.inputs(row, N)
    kernels, text = _update_kernel(dt, F, k, N)
    plan = _plan(dt, X, W0, H0, k)
    n_tiles = (N + 63) // 64
    if row[3] == pc.MULTI:
        assert n_tiles >= 2 * plan.n_parts + 1, (n_tiles, plan.n_parts)
    else:
        assert plan.n_parts == n_tiles  # one tile per workgroup
    plan.partials.fill_(float("nan"))
    err = plan.frobenius_error()
    ref = mu_ref.frobenius_error(X, W0, H0)
    print(f"PASSMATRIX loss {pc.row_id(row)} err/bar={abs(err - ref) / ref / 1e-12:.2e}")
    assert abs(err - ref) <= 1e-12 * ref, (err, ref)
    assert np.array_equal(plan.W.cpu().numpy().astype(np.float64), W0)  # the loss pass changes nothing
    _one_pass(plan, dt, F, k, X, W0, H0, kernels)


REG_ROWS = [("float32", 301, 3), ("float32", 301, 7), ("float32", 301, 13),
            ("float64", 200, 4), ("float64", 200, 8), ("float64", 200, 16),
            ("bfloat16", 301, 5), ("float32", 17, 3),
            ("float32", 81, 5), ("bfloat16", 81, 12), ("float32", 81, 4)]


@pytest.mark.parametrize("reg", [(0.3, 0.2), (0.0, 0.0)], ids=["l1l2", "noreg"])
@pytest.mark.parametrize("dt, F, k", REG_ROWS)
def test_regularisation_and_zero_rules(dt, F, k, reg):
    """(c) l1_W / l2_W, a zero column and scattered zeros in W0, an all-zero row of H0 (its HHᵀ row is
    zero: without regularisation the denominator is 0 and becomes float32 eps, SK:620), two all-zero
    rows of X, one of them the last row of the ragged tile."""
    N = pc.RAGGED
    row = (dt, F, k, N, "zero rules")
    X, W0, H0 = pc.inputs(row)
    rng = np.random.default_rng(zlib.crc32(f"{dt}{F}{k}".encode()))
    W0[rng.random(W0.shape) < 0.1] = 0.0
    W0[:, k - 1] = 0.0
    H0[0] = 0.0
    X[70] = 0.0
    X[N - 1] = 0.0
    kernels, _ = _update_kernel(dt, F, k, N)
    plan = _plan(dt, X, W0, H0, k, l1_W=reg[0], l2_W=reg[1])
    _one_pass(plan, dt, F, k, X, W0, H0, kernels, reg)
    Wg = plan.W.cpu().numpy()
    assert not Wg[:, k - 1].any() and not Wg[70].any() and not Wg[N - 1].any()
    if reg == (0.0, 0.0):
        assert not Wg[:, 0].any()  # 0 / eps, not 0 / 0


# (d) the forms of cnmf_reduce_update: (dtype, F, k, zero column in W0)
TAIL_ROWS = [("float32", 7, 4, False), ("float32", 586, 3, False),                            # KP = 4: fused
             ("float32", 17, 5, False), ("float32", 300, 8, False), ("float32", 512, 7, False),  # KP = 8
             ("float32", 320, 16, False), ("float32", 16 * 19 + 1, 9, False),                 # KP = 16: split
             ("float32", 321, 12, False), ("float32", 479, 16, False),                        # KP = 16: one workgroup
             ("float64", 200, 6, False), ("bfloat16", 81, 8, False),
             ("float32", 100, 5, True)]


@pytest.mark.parametrize("dt, F, k, zero_col", TAIL_ROWS)
def test_iteration_tails(dt, F, k, zero_col):
    """(d) three iterations (pass, reduction, basis update) with l1_H / l2_H against the fp64 oracle.
    A zero column of W0 stays zero, so (WᵀW)·H has a zero row: without regularisation that
    denominator is 0 and becomes float32 eps (SK:706)."""
    import torch
    N = 2000 + 37
    X, W0, H0 = pc.inputs((dt, F, k, N, "tail"))
    l1_H, l2_H = (0.0, 0.0) if zero_col else (0.1, 0.05)
    if zero_col:
        W0[:, 1] = 0.0
    plan = _plan(dt, X, W0, H0, k, l1_H=l1_H, l2_H=l2_H)
    assert not plan.persistent_shape  # per-iteration launches: cnmf_mu_sample_pass + cnmf_reduce_update
    plan.iterate(3)
    torch.cuda.synchronize()
    Wr, Hr, _ = mu_ref.mu_fit(X, W0, H0, max_iter=3, tol=0.0, l1_reg_H=l1_H, l2_reg_H=l2_H)
    W, H = plan.W.cpu().numpy(), plan.H64.cpu().numpy()
    bar = TOL64 if dt == "float64" else TOL32
    ew, eh = rel_fro(W, Wr), rel_fro(H, Hr)
    print(f"PASSMATRIX tail {dt} F={F} k={k} W {ew:.2e} H {eh:.2e} (bar {bar:.0e})")
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert ew <= bar and eh <= bar, (ew, eh)
    if zero_col:
        assert not W[:, 1].any() and not H[1].any()
    Ht, HHt = plan.Ht.cpu().numpy(), plan.HHt.cpu().numpy()
    np.testing.assert_array_equal(Ht[:, :k], H.T)
    assert not Ht[:, k:].any() and not HHt[k:, :].any() and not HHt[:, k:].any()
    np.testing.assert_allclose(HHt[:k, :k], H @ H.T, rtol=1e-12)
    assert plan.counters_at_rest()


def test_refusals_are_clean():
    """(e) fp32 k = 8: the pass takes F up to 552, the basis update k > 4 up to F = 512.  Between them
    the plan is built and set_H refuses, naming the limit; one past the pass limit the constructor
    refuses.  Neither launches anything."""
    import torch
    from cnmf_amd import _lib
    from cnmf_amd.solver import MUPlan
    widest = pc.WIDEST["float32", 8]
    assert widest > 512
    rng = np.random.default_rng(5)
    X = torch.from_numpy(rng.random((64, widest), dtype=np.float32)).cuda()
    plan = MUPlan(X, 8)
    with pytest.raises(_lib.HipLibraryError, match="512"):
        plan.set_H(torch.from_numpy(rng.random((8, widest), dtype=np.float32)))
    torch.cuda.synchronize()
    assert not plan.Ht.any() and not plan.HHt.any()  # no kernel derived them
    X = torch.from_numpy(rng.random((64, widest + 1), dtype=np.float32)).cuda()
    with pytest.raises(_lib.HipLibraryError, match=f"n_features={widest + 1}"):
        MUPlan(X, 8)
    torch.cuda.synchronize()
