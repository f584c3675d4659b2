"""solver='whals' on the GPU.  Unit weights: sklearn 1.7.2's solver='cd' answers (tests/golden/hals_*.npz,
k <= 8) — the bars of solver='hals': float64 X equal n_iter, W and H within 1e-9 relative Frobenius;
float32 X equal n_iter and 1e-5 against the restatement run in fp64 from the rounded inputs.  Weighted:
the same bars against tests/whals_ref.py on the cases of tests/whals_cases.py (ragged and misaligned
shapes, the envelope's corners, many workgroups).  Masks: rows and columns masked whole keep their
start bit for bit and leave the unweighted fit of the submatrix; values under zero weights change no
bit.  Mechanics: the device gate, independence from how often the host reads the control block,
bit-for-bit repeatability, the refusal of a shape outside the envelope."""
import functools
import json
import os
import warnings

import numpy as np
import pytest

import hals_ref
import whals_cases as cases
import whals_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)
GOLDENS = ["k4", "k8", "f17", "tol0", "reg", "dead", "k1", "transform"]  # every golden with k <= 8
BAR = {np.float64: 1e-9, np.float32: 1e-5}
DTYPES = [np.float64, np.float32]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def load(name):
    g = np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def golden_expected(name, dtype):
    """sklearn's own answer for float64; for float32 the restatement in fp64 from the rounded inputs."""
    g, c = load(name), MANIFEST["cases"][name]
    if dtype is np.float64:
        return g["W"], g["H"], int(g["n_iter"])
    kw = {a: c["kwargs"][a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in c["kwargs"]}
    l1_W, l1_H, l2_W, l2_H = hals_ref.regularization(*c["shape"], **kw)
    W0 = g["W0"].astype(dtype).astype(np.float64) if c["update_H"] else None
    r = hals_ref.fit(g["X"].astype(dtype).astype(np.float64), W0, g["H0"].astype(dtype).astype(np.float64),
                     tol=c["kwargs"]["tol"], max_iter=c["kwargs"]["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W,
                     l2_H=l2_H, update_H=c["update_H"])
    return r["W"], r["H"], r["n_iter"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", GOLDENS)
def test_unit_weights_match_sklearn(name, dtype):
    from cnmf_amd import NMF, factorise
    g, c = load(name), MANIFEST["cases"][name]
    X = g["X"].astype(dtype)
    ones = np.ones_like(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if c["update_H"]:
            est = NMF(n_components=c["k"], init="custom", solver="whals", device="cuda:0", **c["kwargs"])
            W = est.fit_transform(X, W=g["W0"].astype(dtype), H=g["H0"].astype(dtype), weights=ones)
            H, n_iter, err = est.components_, est.n_iter_, est.reconstruction_err_
        else:
            W, H, n_iter = factorise(X, None, g["H0"].astype(dtype), n_components=c["k"], init="custom",
                                     update_H=False, solver="whals", weights=ones, device="cuda:0", **c["kwargs"])
            err = None
    We, He, ne = golden_expected(name, dtype)
    ew, eh = rel(W, We), rel(H, He)
    print(f"{name} {dtype.__name__}: n_iter {n_iter} ({ne}) relW {ew:.2e} relH {eh:.2e}")
    assert n_iter == ne == c["n_iter"]
    assert ew <= BAR[dtype] and eh <= BAR[dtype]
    assert W.dtype == dtype and H.dtype == dtype
    if err is not None:
        host = np.linalg.norm(X.astype(np.float64) - W.astype(np.float64) @ H.astype(np.float64))
        print(f"    reconstruction_err_ off by {abs(err - host) / host:.2e}")
        assert abs(err - host) / host <= BAR[dtype]
    if name == "dead":  # both hess == 0 branches: the component stays exactly as it is
        assert not W[:, 2].any() and not H[2].any() and not W[::9].any()


@functools.lru_cache(maxsize=None)
def gpu_fit(name, dt, junk=False):
    """factorise(..., solver='whals') on the case; junk: large values written under the zero weights."""
    from cnmf_amd import factorise
    c = cases.CASES[name]
    X, M, W0, H0 = cases.inputs(name, dt)
    if junk:
        X = X.copy()
        X[M == 0] = (1e3 * np.random.RandomState(9).uniform(1.0, 2.0, size=int((M == 0).sum()))).astype(X.dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return factorise(X, W0, H0, n_components=c["k"], init="custom", update_H=c.get("update_H", True),
                         solver="whals", weights=M, tol=c["tol"], max_iter=c["max_iter"], device="cuda:0",
                         **c.get("reg", {}))


@pytest.mark.parametrize("name, dt", [p for p in cases.PARAMS if p[0] != "masked"])
def test_weighted_fit_matches_the_restatement(name, dt):
    c = cases.CASES[name]
    W, H, n_iter = gpu_fit(name, dt)
    r = cases.expected(name, dt)
    bar = BAR[cases.DTYPE[dt]]
    ew, eh = rel(W, r["W"]), rel(H, r["H"])
    print(f"{name} {dt} {c['shape']} k={c['k']}: n_iter {n_iter} ({r['n_iter']}) relW {ew:.2e} relH {eh:.2e}")
    assert n_iter == r["n_iter"]
    assert ew <= bar and eh <= bar
    assert W.dtype == cases.DTYPE[dt] and H.dtype == cases.DTYPE[dt]
    if not c.get("update_H", True):
        assert np.array_equal(H, cases.inputs(name, dt)[3])


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rows_and_columns_masked_whole(dt):
    from cnmf_amd import factorise
    c = cases.CASES["masked"]
    X, M, W0, H0 = cases.inputs("masked", dt)
    kr, kc = cases.kept("masked")
    W, H, n_iter = gpu_fit("masked", dt)
    sub = cases.expected_submatrix("masked", dt)
    bar = BAR[cases.DTYPE[dt]]
    ew, eh = rel(W[kr], sub["W"]), rel(H[:, kc], sub["H"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, n_hals = factorise(np.ascontiguousarray(X[kr][:, kc]), np.ascontiguousarray(W0[kr]),
                                 np.ascontiguousarray(H0[:, kc]), n_components=c["k"], init="custom", solver="hals",
                                 tol=c["tol"], max_iter=c["max_iter"], device="cuda:0")
    print(f"masked {dt}: n_iter {n_iter} (submatrix: restatement {sub['n_iter']}, 'hals' {n_hals}) relW {ew:.2e} relH {eh:.2e}")
    assert np.array_equal(W[~kr], W0[~kr]) and np.array_equal(H[:, ~kc], H0[:, ~kc])  # bit for bit
    assert n_iter == sub["n_iter"] == n_hals
    assert ew <= bar and eh <= bar


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_values_under_zero_weights_change_no_bit(dt):
    W, H, n = gpu_fit("w30", dt)
    Wj, Hj, nj = gpu_fit("w30", dt, junk=True)
    assert W is not Wj and n == nj and np.array_equal(W, Wj) and np.array_equal(H, Hj)


def plan_fit(name, dt, stretch=None):
    """WeightedHALSPlan + run_hals on cuda:0.  Returns (plan, n_iter)."""
    import torch
    from cnmf_amd.solver import WeightedHALSPlan, run_hals
    c = cases.CASES[name]
    X, M, W0, H0 = cases.inputs(name, dt)
    dev = torch.device("cuda:0")
    l1_W, l1_H, l2_W, l2_H = cases.regs(name)
    plan = WeightedHALSPlan(torch.from_numpy(X.copy()).to(dev), torch.from_numpy(M.copy()).to(dev), c["k"], l1_W, l2_W,
                            l1_H, l2_H)
    plan.set_W(torch.from_numpy(W0.copy()))
    plan.set_H(torch.from_numpy(H0.copy()))
    return plan, run_hals(plan, max_iter=c["max_iter"], tol=c["tol"], stretch=stretch)


def _state(plan):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in (plan.W, plan.H64, plan.Ht, plan.ctl, plan.ticket)]


def test_gate_turns_later_launches_into_no_ops():
    import torch
    from cnmf_amd.solver import HALS_ITERS_DONE, HALS_STOPPED
    plan, n = plan_fit("w30", "f32")
    before = _state(plan)
    ne = cases.expected("w30", "f32")["n_iter"]
    assert n == ne and before[3][HALS_STOPPED] == 1.0 and before[3][HALS_ITERS_DONE] == ne
    assert n % 16 != 0  # the stop fell inside a stretch: no-op launches already followed it
    for _ in range(3):
        plan.step()
    for a, b in zip(before, _state(plan)):
        assert torch.equal(a, b)
    assert int(plan.ticket.item()) == 0
    W, H, nf = gpu_fit("w30", "f32")  # the plan is what factorise runs
    assert nf == n and np.array_equal(plan.W.cpu().numpy(), W)
    err = plan.frobenius_error()
    host = ref.weighted_error(*cases.inputs("w30", "f32")[:2], plan.W.cpu().numpy(), plan.H64.cpu().numpy())
    assert abs(err - host) / host <= 1e-9  # the loss launch: fp64 from the stored factors


def test_result_does_not_depend_on_polling():
    import torch
    per_stretch, n1 = plan_fit("w30reg", "f64")
    per_launch, n2 = plan_fit("w30reg", "f64", stretch=1)
    assert n1 == n2 == cases.expected("w30reg", "f64")["n_iter"]
    for a, b in zip(_state(per_stretch), _state(per_launch)):
        assert torch.equal(a, b)


def test_same_fit_twice_is_bit_identical():
    gpu_fit.cache_clear()
    W1, H1, n1 = gpu_fit("k8f81", "f64")
    gpu_fit.cache_clear()
    W2, H2, n2 = gpu_fit("k8f81", "f64")
    assert W1 is not W2 and n1 == n2 and np.array_equal(W1, W2) and np.array_equal(H1, H2)


def test_a_shape_outside_the_envelope_is_refused_without_a_launch():
    import torch
    from cnmf_amd import factorise
    from cnmf_amd.solver import WeightedHALSPlan
    dev = torch.device("cuda:0")
    X = torch.ones(20, 193, device=dev)
    with pytest.raises(ValueError, match="k=5 with n_features F=193"):
        WeightedHALSPlan(X, torch.ones_like(X), 5)
    Xh = np.ones((20, 513), dtype=np.float32)
    with pytest.raises(ValueError, match="k=4 with n_features F=513"):
        factorise(Xh, n_components=4, init="random", random_state=0, solver="whals", weights=np.ones_like(Xh),
                  device="cuda:0")


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_estimator_reports_the_weighted_error(dt):
    from cnmf_amd import NMF
    c = cases.CASES["w30"]
    X, M, W0, H0 = cases.inputs("w30", dt)
    est = NMF(n_components=c["k"], init="custom", solver="whals", tol=c["tol"], max_iter=c["max_iter"], device="cuda:0")
    assert est.fit(X, W=W0, H=H0, weights=M) is est
    Wf, Hf, nf = gpu_fit("w30", dt)
    assert est.n_iter_ == nf == cases.expected("w30", dt)["n_iter"] and est.n_components_ == c["k"]
    assert np.array_equal(est.components_, Hf) and est.n_features_in_ == 81
    W = est.fit_transform(X, W=W0, H=H0, weights=M)
    assert np.array_equal(W, Wf)
    host = ref.weighted_error(X, M, W, est.components_)
    er = abs(est.reconstruction_err_ - host) / host
    print(f"{dt}: reconstruction_err_ {est.reconstruction_err_:.6f} (host {host:.6f}), off by {er:.2e}")
    assert er <= BAR[cases.DTYPE[dt]]
    # transform takes no weights and runs the 'hals' transform: unit weights are the same algorithm, so
    # the weighted kernels with M = 1 give it to the bar (both sides are within it of the restatement)
    from cnmf_amd import factorise
    Wt = est.transform(X)
    Wu, Hu, _ = factorise(X, H=est.components_, update_H=False, weights=np.ones_like(X), solver="whals",
                          n_components=c["k"], tol=c["tol"], max_iter=c["max_iter"], device="cuda:0")
    print(f"{dt}: transform against the unit-weight 'whals' fit: {rel(Wt, Wu.astype(np.float64)):.2e}")
    assert Wt.dtype == Wu.dtype == X.dtype and np.array_equal(Hu, est.components_)
    assert rel(Wt, Wu.astype(np.float64)) <= BAR[cases.DTYPE[dt]]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("init", ["random", "nndsvda", None])
def test_generated_starts_reach_the_launch(init, dt):
    """init=None / 'random' / 'nndsvda' with weights: the start comes from _initial_factors, the fit from
    the weighted launches.  Without regularisation an iteration never increases Σ m r², so the weighted
    error after 20 iterations is finite and no larger than after 5, which is no larger than after 1."""
    from cnmf_amd import NMF
    X, M, _, _ = cases.inputs("w30", dt)
    errs = []
    for n_it in (1, 5, 20):
        est = NMF(n_components=4, init=init, random_state=3, solver="whals", tol=0.0, max_iter=n_it, device="cuda:0")
        W = est.fit_transform(X, weights=M)
        assert est.n_iter_ == n_it and W.dtype == X.dtype and est.components_.dtype == X.dtype
        assert np.isfinite(W).all() and np.isfinite(est.components_).all() and (W >= 0).all()
        host = ref.weighted_error(X, M, W, est.components_)
        assert abs(est.reconstruction_err_ - host) / host <= BAR[cases.DTYPE[dt]]
        errs.append(est.reconstruction_err_)
    print(f"init={init} {dt}: weighted error after 1 / 5 / 20 iterations {errs}")
    assert np.isfinite(errs).all() and errs[2] <= errs[1] <= errs[0]
