"""init='spa' on the GPU: cnmf_spa_step / cnmf_spa_start_w (csrc/spa.hip) against tests/spa_ref.py and
the goldens, position independence of the scores, the rank stop, determinism, and the start through
factorise / NMF / MiniBatchNMF.

Tolerances (derived, not measured): the worst-case fp64 dot-product bound k·F·2⁻⁵³ at the largest
shape (16 x 512) is 9.1e-13, so ‖q_j(device) − q_j(ref)‖ <= 1e-12/ρ_j (normalising a residual of
relative size ρ_j divides the error by ρ_j) and |‖r‖(device) − ‖r‖(ref)| <= 1e-12·‖y_{p_j}‖."""
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

pytestmark = pytest.mark.gpu

import cnmf_amd  # noqa: E402
from cnmf_amd.synthetic import iop_spectra  # noqa: E402
from spa_ref import row_scale, spa_ref, spa_start_ref  # noqa: E402
from test_spa_ref import MANIFEST, golden_x, rank2  # noqa: E402

spa_mod = importlib.import_module("cnmf_amd.spa")


def _torch():
    import torch
    return torch


def device_spa(X, k, normalise="l1", rank_tol=1e-12, scores=False):
    torch = _torch()
    st = spa_mod.SPAState(torch.from_numpy(np.ascontiguousarray(X)).cuda(), k, normalise, rank_tol, scores=scores)
    idx, info = st.run()
    return st, idx, info


def check_against(X, normalise, idx, info, ref_idx, ref):
    """The three bounds of the module docstring."""
    assert np.array_equal(idx, ref_idx) and idx.dtype == np.int64
    ynorm = np.linalg.norm(row_scale(X, normalise)[ref_idx], axis=1)
    for j, rho in enumerate(ref["rho"]):
        dq = np.linalg.norm(info["Q"][j] - ref["Q"][j])
        dr = abs(info["rho"][j] * info["ymax"] - rho * ref["ymax"])
        print(f"step {j}: rho {rho:.3e} |dq| {dq:.3e} (bound {1e-12 / rho:.3e}) |dr| {dr:.3e} (bound {1e-12 * ynorm[j]:.3e})")
        assert dq <= 1e-12 / rho
        assert dr <= 1e-12 * ynorm[j]
    assert abs(info["mean"] - ref["mean"]) <= 1e-12 * ref["mean"]


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MANIFEST))
@pytest.mark.parametrize("normalise", ["l1", None])
def test_golden(name, normalise):
    X, g = golden_x(name)
    tag = "l1" if normalise == "l1" else "none"
    ref = dict(Q=g[f"Q_{tag}"], rho=g[f"rho_{tag}"], ymax=float(g[f"ymax_{tag}"]), mean=float(g[f"mean_{tag}"]))
    _, idx, info = device_spa(X, int(g["k"]), normalise)
    assert info["steps"] == int(g["k"]) and info["stopped"]
    check_against(X, normalise, idx, info, g[f"idx_{tag}"], ref)


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, F, k, dtype, seed", [
    (32805, 83, 5, np.float32, 5),   # several workgroups, a ragged last tile, rows no multiple of 16 bytes
    (337, 81, 9, np.float64, 2),     # the float32 values widened: float64 spectra have rank ~11, see the goldens
    (337, 512, 16, np.float32, 9),
])
def test_tile_loop(n, F, k, dtype, seed):
    X = iop_spectra(n, F, seed=seed, dtype=np.float32).astype(dtype)
    ref_idx, ref = spa_ref(X, k)
    assert len(ref_idx) == k
    _, idx, info = device_spa(X, k)
    check_against(X, "l1", idx, info, ref_idx, ref)


# 3 ------------------------------------------------------------------------------------------------
def test_ties_and_position_independence():
    X0 = iop_spectra(32805, 81, seed=5)
    per_wg = 192  # rows per workgroup at this n (cnmf_spa_rows(32805) == 171)
    for normalise in ("l1", None):
        X = X0.copy()
        p = int(spa_ref(X, 1, normalise=normalise)[0][0])
        # a copy in another workgroup's range on either side (wrapping), at another place in its tile
        lo, hi = (p + 40 * per_wg + 7) % 32805, (p + 90 * per_wg + 133) % 32805
        rows = sorted({p, lo, hi})
        assert len(rows) == 3 and len({r // per_wg for r in rows}) == 3
        X[lo] = X[p]
        X[hi] = X[p]
        st, idx, info = device_spa(X, 1, normalise, scores=True)
        sc = st.scores.cpu().numpy()
        assert idx[0] == rows[0]
        assert sc[rows[0]].tobytes() == sc[rows[1]].tobytes() == sc[rows[2]].tobytes()
        assert sc[rows[0]] == sc.max()
        # and at a later step, with coefficients in play: identical rows keep identical scores
        st, idx, info = device_spa(X, 3, normalise, scores=True)
        sc = st.scores.cpu().numpy()
        assert sc[rows[0]].tobytes() == sc[rows[1]].tobytes() == sc[rows[2]].tobytes()


# 4 ------------------------------------------------------------------------------------------------
def test_zero_rows_and_tiny_shapes():
    X = iop_spectra(337, 81, seed=2)
    X[::9] = 0
    for normalise in ("l1", None):
        ref_idx, ref = spa_ref(X, 4, normalise=normalise)
        _, idx, info = device_spa(X, 4, normalise)
        check_against(X, normalise, idx, info, ref_idx, ref)
        assert np.all(idx % 9 != 0)
    for X in (np.array([[3.0]]), np.array([[2.0, 0.0, 1.0]], dtype=np.float32), np.array([[1.0], [4.0], [2.0]]),
              iop_spectra(70, 5, seed=7)):
        for normalise in ("l1", None):
            ref_idx, ref = spa_ref(X, 1, normalise=normalise)
            _, idx, info = device_spa(X, 1, normalise)
            check_against(X, normalise, idx, info, ref_idx, ref)
    _, idx, info = device_spa(np.zeros((5, 4)), 2)  # nothing to pick: stopped at step 0
    assert len(idx) == 0 and info["stopped"] and info["mean"] == 0.0


# 5 ------------------------------------------------------------------------------------------------
def test_rank_two_matrix():
    torch = _torch()
    X = rank2()
    st, idx, info = device_spa(X, 4)
    ref_idx, ref = spa_ref(X, 4)
    assert info["steps"] == 2 and info["stopped"] and np.array_equal(idx, ref_idx)
    before = [t.clone() for t in (st.Q, st.ctl, st.ticket)]
    st.step(2)
    st.step(3)
    torch.cuda.synchronize()
    for a, b in zip(before, (st.Q, st.ctl, st.ticket)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert int(st.ticket.item()) == 0
    assert len(cnmf_amd.spa(X, 4)) == 2
    with pytest.raises(ValueError, match="found only 2 independent rows"):
        cnmf_amd.factorise(X, init="spa", n_components=4)


# 6 ------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    X = iop_spectra(32805, 83, seed=5)
    runs = []
    for _ in range(2):
        st, idx, info = device_spa(X, 5, scores=True)
        runs.append([t.cpu().numpy().tobytes() for t in (st.Q, st.ctl, st.ticket, st.scores)])
    assert runs[0] == runs[1]
    a, b = (cnmf_amd.spa_init(X, 5) for _ in range(2))
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, F, k, seed", [(337, 81, 8, 2), (200, 300, 16, 3)])
@pytest.mark.parametrize("xdtype, wdtype", [(np.float32, np.float32), (np.float64, np.float64),
                                            (np.float32, np.float64)])
def test_start_w(n, F, k, seed, xdtype, wdtype):
    torch = _torch()
    X = iop_spectra(n, F, seed=seed, dtype=np.float32).astype(xdtype)
    idx = spa_ref(X, k)[0]
    _, _, M, floor = spa_start_ref(X, idx)
    X64 = X.astype(np.float64)
    ref = np.maximum(X64 @ M, floor)
    bound = 2 * F * 2.0 ** -53 * (np.abs(X64) @ np.abs(M))
    if wdtype == np.float32:
        bound = bound + 2.0 ** -24 * np.abs(ref)
    W = spa_mod.start_w(torch.from_numpy(X).cuda(), M, floor, dtype=torch.from_numpy(np.zeros(1, wdtype)).dtype)
    W = W.cpu().numpy()
    assert W.dtype == wdtype and W.shape == (n, k)
    err = np.abs(W.astype(np.float64) - ref)
    print("max err / bound:", float((err / bound).max()))
    assert np.all(err <= bound)


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["mu", "hals", "als"])
def test_end_to_end_equals_the_custom_start(solver):
    X = iop_spectra(2000, 81, seed=1)
    W0, H0 = cnmf_amd.spa_init(X, 4)
    assert W0.dtype == _torch().float32 and tuple(W0.shape) == (2000, 4) and tuple(H0.shape) == (4, 81)
    W0, H0 = W0.cpu().numpy(), H0.cpu().numpy()
    ref_idx = spa_ref(X, 4)[0]
    Wr, Hr, _, _ = spa_start_ref(X, ref_idx)
    assert np.array_equal(H0, Hr)
    np.testing.assert_allclose(W0, Wr, rtol=1e-5, atol=1e-7)
    a = cnmf_amd.factorise(X, init="spa", n_components=4, solver=solver, tol=0, max_iter=20, random_state=7)
    b = cnmf_amd.factorise(X, W0, H0, init="custom", n_components=4, solver=solver, tol=0, max_iter=20)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == 20


def test_mu_matches_the_oracle_from_the_reference_start():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import mu_ref
    X = iop_spectra(2000, 81, seed=1)
    W0, H0, _, _ = spa_start_ref(X, spa_ref(X, 4)[0])
    # the project's bar (tests/test_gpu_parity.py): the fp64 oracle on identical inputs
    Wr, Hr = mu_ref.mu_fit(X.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), max_iter=20, tol=0)[:2]
    W, H, _ = cnmf_amd.factorise(X, init="spa", n_components=4, tol=0, max_iter=20)
    for got, want in ((W, Wr), (H, Hr)):
        rel = np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want)
        print("relative Frobenius:", rel)
        assert rel <= 1e-5


def test_estimators_run():
    X = iop_spectra(2000, 81, seed=1)
    est = cnmf_amd.NMF(n_components=4, init="spa", max_iter=20).fit(X)
    assert np.isfinite(est.reconstruction_err_) and est.components_.shape == (4, 81)
    mb = cnmf_amd.MiniBatchNMF(n_components=4, init="spa", batch_size=64, max_iter=2).fit(X)
    assert np.isfinite(mb.reconstruction_err_) and mb.components_.shape == (4, 81)
    Xd = _torch().from_numpy(X).cuda()
    W, H, _ = cnmf_amd.factorise(Xd, init="spa", n_components=4, max_iter=5)
    assert W.device == Xd.device and H.device == Xd.device
    idx, info = cnmf_amd.spa(Xd, 4, return_info=True)
    assert set(("Q", "rho", "mean", "steps")) <= set(info) and info["steps"] == 4
