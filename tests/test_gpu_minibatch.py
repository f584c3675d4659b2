"""MiniBatchNMF on the GPU against sklearn 1.7.2's own answers (tests/golden/mb_*.npz) and the fp64
restatement (tests/minibatch_ref.py): the project's parity bar of 1e-5 relative Frobenius, equal
step / iteration counts, the device gate, and independence from how often the host polls."""
import json
import math
import os
import warnings

import numpy as np
import pytest

import minibatch_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_minibatch.json")) as f:
    MANIFEST = json.load(f)
FIT_CASES = ["hstop", "noimp", "tol0", "b301", "bigbatch", "reg20x10", "k8", "k16", "f17", "zerorows"]
BAR = 1e-5


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def load(name):
    return np.load(os.path.join(GOLDEN, f"mb_{name}.npz"))


def estimator(name, **extra):
    from cnmf_amd import MiniBatchNMF
    c = MANIFEST["cases"][name]
    return MiniBatchNMF(n_components=c["k"], init="custom", device="cuda:0", **{**c["kwargs"], **extra})


def fit(name, **extra):
    g = load(name)
    est = estimator(name, **extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W = est.fit_transform(g["X"], W=g["W0"], H=g["H0"])
    return est, W, g


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_matches_sklearn(name):
    est, W, g = fit(name)
    eh, ew = rel(est.components_, g["H"]), rel(W, g["W"])
    er = abs(est.reconstruction_err_ - float(g["reconstruction_err"])) / float(g["reconstruction_err"])
    print(f"{name}: n_steps {est.n_steps_} ({int(g['n_steps'])}) n_iter {est.n_iter_} relH {eh:.2e} relW {ew:.2e} "
          f"rel err {er:.2e}")
    assert est.n_steps_ == int(g["n_steps"]) and est.n_iter_ == int(g["n_iter"])
    assert est._stop_reason == int(g["reason"])
    assert eh <= BAR and ew <= BAR and er <= BAR
    assert W.dtype == g["X"].dtype and est.components_.dtype == g["X"].dtype
    assert est.n_components_ == g["H"].shape[0] and est.n_features_in_ == g["X"].shape[1]


def test_misaligned_windows_take_the_staging_path():
    import torch
    from cnmf_amd.minibatch import MiniBatchPlan
    g = load("b301")
    dev = torch.device("cuda:0")
    plan = MiniBatchPlan(g["H0"], torch.float32, dev, rho=0.9)
    plan.attach(torch.from_numpy(g["X"]).to(dev), torch.from_numpy(g["W0"]).to(dev))
    assert plan._window(0, 301)[2] is False and plan._window(301, 602)[2] is True


def _state(plan):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in (plan.W, plan.H64, plan.Ht, plan.HHt, plan.Anum, plan.Bden, plan.ctl)]


def test_gate_turns_later_launches_into_no_ops():
    import torch
    from cnmf_amd.minibatch import MB_STEPS_DONE, MB_STOPPED
    est, W, g = fit("noimp")
    plan = est._plan
    plan.attach(torch.from_numpy(g["X"]).to(plan.device), torch.from_numpy(W).to(plan.device))
    before = _state(plan)
    assert before[-1][MB_STOPPED] == 1.0 and before[-1][MB_STEPS_DONE] == est.n_steps_
    for lo, hi in ((0, 256), (256, 512), (1792, 2048)):
        plan.step(lo, hi)
    after = _state(plan)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert int(plan.counter.abs().sum()) == 0


def test_result_does_not_depend_on_polling():
    every_epoch, W1, g = fit("noimp")
    every_step = estimator("noimp")
    every_step._poll_steps = 1
    W2 = every_step.fit_transform(g["X"], W=g["W0"], H=g["H0"])
    assert every_step.n_steps_ == every_epoch.n_steps_ == int(g["n_steps"])
    assert every_step.n_steps_ % 8 != 0  # the stop fell inside an epoch: no-op launches followed it
    assert np.array_equal(every_step.components_, every_epoch.components_) and np.array_equal(W1, W2)


def test_fixed_number_of_steps_without_polling():
    g = load("hstop")
    kw = dict(batch_size=256, tol=0.0, max_no_improvement=None, max_iter=4)
    est = estimator("hstop", **kw)
    W = est.fit_transform(g["X"], W=g["W0"], H=g["H0"])
    r = ref.fit(g["X"].astype(np.float64), g["W0"], g["H0"], **kw)
    assert est.n_steps_ == 4 * math.ceil(1000 / 256) == r["n_steps"] and est.n_iter_ == 4
    print(f"relH {rel(est.components_, r['H']):.2e} relW {rel(W, r['W']):.2e}")
    assert rel(est.components_, r["H"]) <= BAR and rel(W, r["W"]) <= BAR
    log = est._plan.read_log()
    costs = np.array([c for c, _, _ in r["log"]])
    print("batch costs, relative difference:", np.abs(log[:, 0] - costs) / costs)
    assert len(log) == 16 and abs(log[0, 0] - costs[0]) <= 1e-9 * costs[0]  # the first cost: exact inputs


@pytest.mark.parametrize("k", [4, 8])
def test_one_step_over_many_partial_rows(k):
    """65,536 + 37 rows: many workgroups, several tiles each, a ragged last tile."""
    import torch
    from cnmf_amd.minibatch import MB_LAST_COST, MB_STEPS_DONE, MiniBatchPlan
    from cnmf_amd.synthetic import iop_spectra, random_init
    n = 65536 + 37
    X = iop_spectra(n, 81, seed=21, dtype=np.float32)
    W0, H0 = random_init(X, k, 21)
    dev = torch.device("cuda:0")
    plan = MiniBatchPlan(H0, torch.float32, dev, rho=0.7, n_samples=n, log_cap=4)
    assert plan.lib.cnmf_mb_rows(n) > 100
    plan.attach(torch.from_numpy(X).to(dev), torch.from_numpy(W0).to(dev))
    plan.step(0, n)
    ctl = plan.read_ctl()
    st = ref.State(H0, 0.7, n_samples=n)
    W = W0.astype(np.float64)
    st.step(X.astype(np.float64), W)
    got = {"H": plan.H64, "Anum": plan.Anum, "Bden": plan.Bden, "W": plan.W}
    want = {"H": st.H, "Anum": st.A, "Bden": st.B, "W": W}
    for name in got:
        e = rel(got[name].cpu().numpy(), want[name])
        print(f"k={k} {name}: {e:.2e}")
        assert e <= BAR, name
    cost = st.log[0][0]
    print(f"k={k} batch cost {ctl[MB_LAST_COST]!r} vs {cost!r}")
    assert abs(ctl[MB_LAST_COST] - cost) <= 1e-9 * cost
    assert ctl[MB_STEPS_DONE] == 1 and int(plan.counter.abs().sum()) == 0


@pytest.mark.parametrize("n, F, k, dtype", [(1024, 300, 4, np.float32),    # two teams of a workgroup, 32-row tiles
                                             (200, 512, 16, np.float64),    # the widest basis: the largest LDS layout
                                             (130, 1, 1, np.float32),       # the narrowest
                                             (333, 129, 9, np.float64)])    # odd sizes, two feature slots per lane, KP = 16
def test_one_step_at_the_shape_limits(n, F, k, dtype):
    import torch
    from cnmf_amd.minibatch import MB_LAST_COST, MiniBatchPlan
    rng = np.random.RandomState(n + F + k)
    X = np.abs(rng.randn(n, F)).astype(dtype)
    W0 = np.abs(rng.randn(n, k)).astype(dtype)
    H0 = np.abs(rng.randn(k, F)).astype(dtype)
    dev = torch.device("cuda:0")
    plan = MiniBatchPlan(H0, torch.from_numpy(X).dtype, dev, rho=0.8, n_samples=n)
    plan.attach(torch.from_numpy(X).to(dev), torch.from_numpy(W0).to(dev))
    regs = (0.3, 0.2, 0.1, 0.4)  # l1_W, l1_H, l2_W, l2_H
    plan.step(0, n, regs)
    plan.step(0, n, regs)
    ctl = plan.read_ctl()
    st = ref.State(H0, 0.8, n_samples=n)
    W = W0.astype(np.float64)
    X64 = X.astype(np.float64)
    for _ in range(2):
        W[:] = ref.update_w(X64, W, st.H, regs[0], regs[2])
        cost = ref.batch_cost(X64, W, st.H, regs)
        st.H = ref.update_h(X64, W, st.H.copy(), regs[1], regs[3], st.A, st.B, st.rho)
    for name, got, want in (("H", plan.H64, st.H), ("Anum", plan.Anum, st.A), ("Bden", plan.Bden, st.B),
                            ("W", plan.W, W)):
        e = rel(got.cpu().numpy(), want)
        print(f"{n}x{F} k={k} {name}: {e:.2e}")
        assert e <= BAR, name
    assert abs(ctl[MB_LAST_COST] - cost) <= BAR * cost and int(plan.counter.abs().sum()) == 0


def test_transform_matches_sklearn():
    g = load("transform")
    c = MANIFEST["cases"]["transform"]
    est = estimator("transform", transform_max_iter=c["transform_max_iter"])
    from cnmf_amd import ConvergenceWarning
    with pytest.warns(ConvergenceWarning, match="Maximum number of iterations 3 reached"):  # SKMB's rule
        est.fit(g["X"], W=g["W0"], H=g["H0"])
    assert est.n_steps_ == int(g["n_steps"]) and rel(est.components_, g["H"]) <= BAR
    Wt = est.transform(g["Xt"])
    _, n_ref = ref.solve_w(g["Xt"].astype(np.float64), g["H"], c["transform_max_iter"], c["kwargs"]["tol"])
    print(f"transform: {est.n_transform_iter_} iterations ({n_ref}), relW {rel(Wt, g['Wt']):.2e}")
    assert est.n_transform_iter_ == n_ref == int(g["w_iters"])
    assert rel(Wt, g["Wt"]) <= BAR and Wt.shape == (600, 4)


def test_partial_fit_over_four_chunks():
    g = load("partial")
    est = estimator("partial")
    X = g["X"]
    for i in range(4):
        est.partial_fit(X[250 * i:250 * (i + 1)], W=g["W0"], H=g["H0"])
    print(f"partial_fit: relH {rel(est.components_, g['H']):.2e}")
    assert est.n_steps_ == int(g["n_steps"]) == 4
    assert rel(est.components_, g["H"]) <= BAR
    assert est._plan.Anum.is_cuda  # the accumulators stayed on the device between the calls
