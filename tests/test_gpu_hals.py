"""solver='hals' on the GPU against sklearn 1.7.2's solver='cd' answers (tests/golden/hals_*.npz) and the
fp64 restatement (tests/hals_ref.py).  Bars: float64 X — equal n_iter, W and H within 1e-9 relative
Frobenius (only the summation order differs); float32 X — equal n_iter and the project's 1e-5 against
the restatement run in fp64 from the rounded inputs.  Also the tile loop at ragged and misaligned
shapes, the shape limits, the device gate, independence from how often the host reads the control
block, and bit-for-bit repeatability."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

import hals_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)
CASES = ["k4", "k8", "k16", "f17", "tol0", "reg", "dead", "k1", "transform"]
FIT_CASES = [c for c in CASES if c != "transform"]
BAR = {np.float64: 1e-9, np.float32: 1e-5}
DTYPES = [np.float64, np.float32]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def load(name):
    g = np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))
    return {k: g[k] for k in g.files}


def regs(name):
    c = MANIFEST["cases"][name]
    kw = {a: c["kwargs"][a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in c["kwargs"]}
    return ref.regularization(*c["shape"], **kw)


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """sklearn's own answer for float64; for float32 the restatement in fp64 from the rounded inputs."""
    g, c = load(name), MANIFEST["cases"][name]
    if dtype is np.float64:
        return g["W"], g["H"], int(g["n_iter"])
    l1_W, l1_H, l2_W, l2_H = regs(name)
    W0 = g["W0"].astype(dtype).astype(np.float64) if c["update_H"] else None
    r = ref.fit(g["X"].astype(dtype).astype(np.float64), W0, g["H0"].astype(dtype).astype(np.float64),
                tol=c["kwargs"]["tol"], max_iter=c["kwargs"]["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H,
                update_H=c["update_H"])
    return r["W"], r["H"], r["n_iter"]


@functools.lru_cache(maxsize=None)
def gpu_fit(name, dtype):
    from cnmf_amd import factorise
    g, c = load(name), MANIFEST["cases"][name]
    W0 = g["W0"].astype(dtype) if c["update_H"] else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return factorise(g["X"].astype(dtype), W0, g["H0"].astype(dtype), n_components=c["k"], init="custom",
                         update_H=c["update_H"], solver="hals", device="cuda:0", **c["kwargs"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_factorise_matches_sklearn(name, dtype):
    W, H, n_iter = gpu_fit(name, dtype)
    We, He, ne = expected(name, dtype)
    ew, eh = rel(W, We), rel(H, He)
    print(f"{name} {dtype.__name__}: n_iter {n_iter} ({ne}) relW {ew:.2e} relH {eh:.2e}")
    assert n_iter == ne == MANIFEST["cases"][name]["n_iter"]
    assert ew <= BAR[dtype] and eh <= BAR[dtype]
    assert W.dtype == dtype and H.dtype == dtype
    if name == "dead":  # both hess == 0 branches: the component stays exactly as it is
        assert not W[:, 2].any() and not H[2].any() and not W[::9].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", FIT_CASES)
def test_estimator_matches_sklearn(name, dtype):
    from cnmf_amd import NMF
    g, c = load(name), MANIFEST["cases"][name]
    est = NMF(n_components=c["k"], init="custom", solver="hals", device="cuda:0", **c["kwargs"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = est.fit_transform(g["X"].astype(dtype), W=g["W0"].astype(dtype), H=g["H0"].astype(dtype))
    We, He, ne = expected(name, dtype)
    err = np.linalg.norm(g["X"].astype(np.float64) - W.astype(np.float64) @ est.components_.astype(np.float64))
    er = abs(est.reconstruction_err_ - err) / err
    print(f"{name} {dtype.__name__}: n_iter {est.n_iter_} relW {rel(W, We):.2e} relH {rel(est.components_, He):.2e} "
          f"reconstruction_err_ off by {er:.2e}")
    assert est.n_iter_ == ne and est.n_components_ == c["k"] and est.n_features_in_ == c["shape"][1]
    assert rel(W, We) <= BAR[dtype] and rel(est.components_, He) <= BAR[dtype]
    assert er <= BAR[dtype]
    Wf, Hf, _ = gpu_fit(name, dtype)
    assert np.array_equal(W, Wf) and np.array_equal(est.components_, Hf)  # the same launches


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_transform_matches_sklearn(dtype):
    """NMF.transform: update_H=False from W = 0 against fixed components."""
    from cnmf_amd import NMF
    g, c = load("transform"), MANIFEST["cases"]["transform"]
    k4 = load("k4")
    est = NMF(n_components=4, init="custom", solver="hals", device="cuda:0", **c["kwargs"])
    est.fit(k4["X"].astype(dtype), W=k4["W0"].astype(dtype), H=k4["H0"].astype(dtype))
    assert rel(est.components_, g["H0"].astype(np.float64)) <= 2 * BAR[np.float32]  # the case's H: this fit's, rounded
    est.components_ = g["H0"].astype(dtype)
    Wt = est.transform(g["X"].astype(dtype))
    We = expected("transform", dtype)[0]
    print(f"transform {dtype.__name__}: relW {rel(Wt, We):.2e}")
    assert Wt.shape == (100, 4) and Wt.dtype == dtype and rel(Wt, We) <= BAR[dtype]
    assert np.array_equal(Wt, gpu_fit("transform", dtype)[0])
    back = est.inverse_transform(Wt)
    assert back.shape == g["X"].shape and np.array_equal(back, Wt @ est.components_)


def plan_fit(X, W0, H0, max_iter, tol=0.0, regs=(0.0, 0.0, 0.0, 0.0), stretch=None):
    """HALSPlan + run_hals on cuda:0; regs = (l1_W, l1_H, l2_W, l2_H).  Returns (plan, n_iter)."""
    import torch
    from cnmf_amd.solver import HALSPlan, run_hals
    dev = torch.device("cuda:0")
    plan = HALSPlan(torch.from_numpy(X).to(dev), H0.shape[0], regs[0], regs[2], regs[1], regs[3])
    plan.set_W(torch.from_numpy(W0))
    plan.set_H(torch.from_numpy(H0))
    return plan, run_hals(plan, max_iter=max_iter, tol=tol, stretch=stretch)


def against_ref(X, W0, H0, n_iter, regs=(0.0, 0.0, 0.0, 0.0)):
    plan, n = plan_fit(X, W0, H0, n_iter, regs=regs)
    r = ref.fit(X.astype(np.float64), W0, H0, tol=0.0, max_iter=n_iter, l1_W=regs[0], l1_H=regs[1], l2_W=regs[2],
                l2_H=regs[3])
    ew, eh = rel(plan.W.cpu().numpy(), r["W"]), rel(plan.H64.cpu().numpy(), r["H"])
    ctl = plan.read_ctl()
    ev = abs(ctl[3] / ctl[2] - r["violations"][-1]) / r["violations"][-1]
    print(f"{X.shape[0]}x{X.shape[1]} k={H0.shape[0]} {X.dtype}: relW {ew:.2e} relH {eh:.2e} violation ratio off by {ev:.2e}")
    bar = BAR[X.dtype.type]
    assert n == n_iter == r["n_iter"] and ctl[0] == 0.0
    # the violation ratio: within the 0.1 % by which every golden's stop is separated from tol
    assert ew <= bar and eh <= bar and ev <= 1e-3
    assert int(plan.ticket.item()) == 0  # the ticket word is left zero
    return plan


def test_every_workgroup_loops_over_tiles_and_the_last_is_ragged():
    from cnmf_amd import _lib
    from cnmf_amd.synthetic import iop_spectra, random_init
    lib = _lib.load()
    cap = lib.cnmf_hals_rows(10 ** 9)
    n = 64 * 2 * cap + 37
    assert cap == 256 and lib.cnmf_hals_rows(n) > 100 and n // lib.cnmf_hals_rows(n) >= 128
    X = iop_spectra(n, 81, seed=31)
    W0, H0 = random_init(X, 4, 31)
    against_ref(X, W0, H0, 10)


@pytest.mark.parametrize("F, k, dtype", [(83, 5, np.float32),   # rows and W no multiple of 16 bytes
                                         (81, 9, np.float64)])  # KP = 16 with idle components
def test_misaligned_rows(F, k, dtype):
    from cnmf_amd.synthetic import iop_spectra, random_init
    n = 64 * 5 + 17
    X = iop_spectra(n, F, seed=32, dtype=dtype)
    assert (F * X.itemsize) % 16 != 0 and (k * X.itemsize) % 16 != 0
    W0, H0 = random_init(X, k, 32)
    against_ref(X, W0, H0, 10, regs=(0.01, 0.02, 0.03, 0.04))


def test_shape_limits():
    from cnmf_amd import _lib, factorise
    rng = np.random.RandomState(33)
    X = np.abs(rng.randn(337, 512)).astype(np.float32)
    W0 = np.abs(rng.randn(337, 16)).astype(np.float32)
    H0 = np.abs(rng.randn(16, 512)).astype(np.float32)
    against_ref(X, W0, H0, 5)
    Xw = np.abs(rng.randn(20, 513)).astype(np.float32)
    with pytest.raises(_lib.HipLibraryError, match=r"n_features=513 \(1..512\)"):
        factorise(Xw, n_components=4, init="random", random_state=0, solver="hals", device="cuda:0")


def _state(plan):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in (plan.W, plan.H64, plan.Ht, plan.HHt, plan.ctl, plan.ticket)]


def test_gate_turns_later_launches_into_no_ops():
    import torch
    from cnmf_amd.solver import HALS_ITERS_DONE, HALS_STOPPED
    g = load("k4")
    plan, n = plan_fit(g["X"], g["W0"], g["H0"], 200, tol=1e-4)
    before = _state(plan)
    assert n == 61 and before[4][HALS_STOPPED] == 1.0 and before[4][HALS_ITERS_DONE] == 61
    assert n % 16 != 0  # the stop fell inside a stretch: no-op launches already followed it
    for _ in range(3):
        plan.step()
    for a, b in zip(before, _state(plan)):
        assert torch.equal(a, b)
    assert int(plan.ticket.item()) == 0


def test_result_does_not_depend_on_polling():
    import torch
    g = load("k4")
    per_stretch, n1 = plan_fit(g["X"], g["W0"], g["H0"], 200, tol=1e-4)
    per_launch, n2 = plan_fit(g["X"], g["W0"], g["H0"], 200, tol=1e-4, stretch=1)
    assert n1 == n2 == 61
    for a, b in zip(_state(per_stretch), _state(per_launch)):
        assert torch.equal(a, b)


def test_tol_zero_runs_exactly_max_iter():
    from cnmf_amd.solver import HALS_ITERS_DONE, HALS_STOPPED, HALS_VIOL_LAST
    g = load("tol0")
    plan, n = plan_fit(g["X"], g["W0"], g["H0"], 30, tol=0.0)
    ctl = plan.read_ctl()
    assert n == 30 and ctl[HALS_ITERS_DONE] == 30 and ctl[HALS_STOPPED] == 0.0 and ctl[HALS_VIOL_LAST] > 0.0
    plan, n = plan_fit(g["X"], g["W0"], g["H0"], 17, tol=0.0)  # a stretch and one launch
    assert n == 17


def test_same_fit_twice_is_bit_identical():
    gpu_fit.cache_clear()
    W1, H1, n1 = gpu_fit("k16", np.float32)
    gpu_fit.cache_clear()
    W2, H2, n2 = gpu_fit("k16", np.float32)
    assert W1 is not W2 and n1 == n2 and np.array_equal(W1, W2) and np.array_equal(H1, H2)


def test_normalise_l2():
    from cnmf_amd import factorise
    g, c = load("k4"), MANIFEST["cases"]["k4"]
    W, H, n = factorise(g["X"], g["W0"], g["H0"], n_components=4, init="custom", solver="hals", normalise="l2",
                        device="cuda:0", **c["kwargs"])
    Wp, Hp, n_plain = gpu_fit("k4", np.float32)
    norms = np.linalg.norm(H.astype(np.float64), axis=1)
    e = rel(W.astype(np.float64) @ H.astype(np.float64), Wp.astype(np.float64) @ Hp.astype(np.float64))
    print(f"normalise: row norms {norms}, W.H off by {e:.2e}")
    assert n == n_plain and np.allclose(norms, 1.0, atol=1e-6) and e <= 1e-6


def test_device_tensors_stay_on_the_device():
    import torch
    from cnmf_amd import factorise
    g, c = load("k4"), MANIFEST["cases"]["k4"]
    dev = torch.device("cuda:0")
    W, H, n = factorise(torch.from_numpy(g["X"]).to(dev), torch.from_numpy(g["W0"]).to(dev),
                        torch.from_numpy(g["H0"]).to(dev), n_components=4, init="custom", solver="hals", **c["kwargs"])
    assert isinstance(W, torch.Tensor) and W.is_cuda and H.is_cuda and W.dtype == torch.float32
    Wp, Hp, n_plain = gpu_fit("k4", np.float32)
    assert n == n_plain and np.array_equal(W.cpu().numpy(), Wp) and np.array_equal(H.cpu().numpy(), Hp)


def test_convergence_warning_and_verbose(capsys):
    from cnmf_amd import ConvergenceWarning, factorise
    g, c = load("k8"), MANIFEST["cases"]["k8"]
    with pytest.warns(ConvergenceWarning, match="Maximum number of iterations 200 reached"):
        factorise(g["X"], g["W0"], g["H0"], n_components=8, init="custom", solver="hals", device="cuda:0", **c["kwargs"])
    g, c = load("k1"), MANIFEST["cases"]["k1"]
    capsys.readouterr()
    _, _, n = factorise(g["X"], g["W0"], g["H0"], n_components=1, init="custom", solver="hals", device="cuda:0", verbose=1,
                        **c["kwargs"])
    out = capsys.readouterr().out.splitlines()
    assert n == c["n_iter"] and [ln.split(":")[0] for ln in out] == ["violation"] * n + [f"Converged at iteration {n + 1}"]
    assert float(out[0].split(":")[1]) == 1.0
