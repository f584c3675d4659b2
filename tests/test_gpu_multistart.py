"""factorise_multistart on the GPU against sklearn 1.7.2's solver='cd' answers for every start
(tests/golden/ms_*.npz) and the fp64 restatement (tests/hals_ref.py).  Bars, those of
tests/test_gpu_hals.py: float64 X — equal n_iter per start, W, H and the errors within 1e-9 relative
(only the summation order differs); float32 X — equal n_iter and the project's 1e-5 against the
restatement run in fp64 from the rounded inputs.  A start of init='random' is drawn in X's dtype, so
the float64 runs are held to sklearn's answers from the float64 starts (the golden's *_64 arrays)
and the float32 runs to the float32 starts.  Also: custom starts give the same bits, a start's bits
do not depend on what shares its launches, the single-start path, the tile loop at ragged shapes,
the device gate, repeatability and the shape of the result.

On the product library a launch takes one start and is cnmf_hals_step's (cnmf_ms_batch is 1: the
batched form was measured slower).  The batched form — several starts on one staged tile — lives in the
diagnostic library behind CNMF_MS_TEAMS; its cases run in a child process on that library, as
tests/test_gpu_mf8.py runs the layouts kept out of the product."""
import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import hals_ref as ref

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIAG = os.path.join(_ROOT, "cnmf_amd", "libcnmf_hip_diag.so")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_multistart.json")) as f:
    MANIFEST = json.load(f)
CASES = ["k4", "k8", "k16", "f17", "k1", "reg", "zero"]
BAR = {np.float64: 1e-9, np.float32: 1e-5}
DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
SUFFIX = {np.float64: "_64", np.float32: ""}


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def load(name):
    g = np.load(os.path.join(GOLDEN, f"ms_{name}.npz"))
    return {k: g[k] for k in g.files}


def regs(shape, kw):
    return ref.regularization(*shape, **{a: kw[a] for a in ("alpha_W", "alpha_H", "l1_ratio") if a in kw})


def restate(X, W0, H0, kw):
    """hals_ref.fit in fp64 from the given (already rounded) inputs: W, H, n_iter, ‖X − WH‖."""
    l1_W, l1_H, l2_W, l2_H = regs(X.shape, kw)
    X64 = X.astype(np.float64)
    r = ref.fit(X64, W0.astype(np.float64), H0.astype(np.float64), tol=kw["tol"], max_iter=kw["max_iter"],
                l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H)
    return r["W"], r["H"], r["n_iter"], float(np.linalg.norm(X64 - r["W"] @ r["H"]))


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """Per start (W, H, n_iter, error): sklearn's own answer from the float64 starts for float64 X;
    for float32 X the restatement in fp64 from the float32 X and starts."""
    g, c = load(name), MANIFEST["cases"][name]
    if dtype is np.float64:
        return [(g["W_64"][r], g["H_64"][r], int(g["n_iter_64"][r]), float(g["errors_64"][r]))
                for r in range(len(c["seeds"]))]
    return [restate(g["X"], g["W0"][r], g["H0"][r], c["kwargs"]) for r in range(len(c["seeds"]))]


def fit(name, dtype, seeds=None, **options):
    from cnmf_amd import factorise_multistart
    g, c = load(name), MANIFEST["cases"][name]
    seeds = c["seeds"] if seeds is None else seeds
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return factorise_multistart(g["X"].astype(dtype), c["k"], n_init=len(seeds), init="random",
                                    random_state=list(seeds), keep="all", device="cuda:0", **c["kwargs"], **options)


@functools.lru_cache(maxsize=None)
def full(name, dtype):
    return fit(name, dtype)


def same_bits(a, b, r, s):
    """start r of result a and start s of result b"""
    return (np.array_equal(a.W_all[r], b.W_all[s]) and np.array_equal(a.H_all[r], b.H_all[s])
            and a.n_iters[r] == b.n_iters[s] and a.errors[r] == b.errors[s])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_every_start_matches_sklearn(name, dtype):
    res, c, exp = full(name, dtype), MANIFEST["cases"][name], expected(name, dtype)
    assert res.seeds == c["seeds"] and len(exp) == len(c["seeds"])
    worst = [0.0, 0.0, 0.0]
    for r, (We, He, ne, ee) in enumerate(exp):
        ew, eh, er = rel(res.W_all[r], We), rel(res.H_all[r], He), abs(res.errors[r] - ee) / ee
        worst = [max(a, b) for a, b in zip(worst, (ew, eh, er))]
        print(f"{name} {dtype.__name__} start {r}: n_iter {res.n_iters[r]} ({ne}) relW {ew:.2e} relH {eh:.2e} "
              f"error {res.errors[r]:.6f} off by {er:.2e}")
        assert res.n_iters[r] == ne == c["n_iter" + SUFFIX[dtype]][r]
        assert ew <= BAR[dtype] and eh <= BAR[dtype] and er <= BAR[dtype]
    print(f"{name} {dtype.__name__}: worst relW {worst[0]:.2e} relH {worst[1]:.2e} error {worst[2]:.2e}")
    best = int(np.argmin(res.errors))
    assert res.best == best and res.n_iter == res.n_iters[best]
    assert np.array_equal(res.W, res.W_all[best]) and np.array_equal(res.H, res.H_all[best])
    if c["best_gap" + SUFFIX[dtype]] > MANIFEST["best_gap"]:
        assert res.best == c["best" + SUFFIX[dtype]]
    if name == "k1":  # the three starts reach the same error: the tie rule
        assert res.best == 0
    assert res.W_all.dtype == dtype and res.H_all.dtype == dtype and res.W.dtype == dtype
    if name == "zero":
        assert not res.W_all[:, ::9].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_custom_starts_give_the_same_bits(name, dtype):
    from cnmf_amd import factorise_multistart
    g, c = load(name), MANIFEST["cases"][name]
    X = g["X"].astype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = factorise_multistart(X, c["k"], init="custom", W=g["W0" + SUFFIX[dtype]], H=g["H0" + SUFFIX[dtype]],
                                   keep="all", device="cuda:0", **c["kwargs"])
    a = full(name, dtype)
    assert res.seeds is None and res.best == a.best
    for r in range(len(c["seeds"])):
        assert same_bits(res, a, r, r), (name, r)
    if dtype is np.float64:  # the float32 starts given as float64: sklearn's answer from exactly these values
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = factorise_multistart(X, c["k"], init="custom", W=g["W0"].astype(dtype), H=g["H0"].astype(dtype),
                                       keep="all", device="cuda:0", **c["kwargs"])
        for r in range(len(c["seeds"])):
            ew, eh = rel(res.W_all[r], g["W"][r]), rel(res.H_all[r], g["H"][r])
            er = abs(res.errors[r] - g["errors"][r]) / g["errors"][r]
            print(f"{name} start {r} from the float32 start: relW {ew:.2e} relH {eh:.2e} error off by {er:.2e}")
            assert res.n_iters[r] == g["n_iter"][r] and max(ew, eh, er) <= BAR[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["k4", "k16"])
def test_a_start_does_not_depend_on_its_company(name, dtype):
    """On the product library a launch takes one start (cnmf_ms_batch is 1), so the forced batch
    sizes give the same launches and this holds the driver and the layout to account: the order of
    the starts, the per-batch arrays, a stopped start left alone.  The kernel's side of the claim —
    starts that share a launch — is test_batched_form_on_the_diagnostic_library."""
    c, a = MANIFEST["cases"][name], full(name, dtype)
    seeds = c["seeds"]
    for r, seed in enumerate(seeds):  # alone: R = 1
        solo = fit(name, dtype, seeds=[seed])
        assert same_bits(solo, a, 0, r), (name, "solo", r)
    back = fit(name, dtype, seeds=seeds[::-1])
    small = fit(name, dtype, _max_batch=2)
    one = fit(name, dtype, _max_batch=1)
    for r in range(len(seeds)):
        assert same_bits(back, a, len(seeds) - 1 - r, r), (name, "reversed", r)
        assert same_bits(small, a, r, r), (name, "batches of two", r)
        assert same_bits(one, a, r, r), (name, "batches of one", r)
    if name == "k4":  # seed 1 stops at 61 while the others run on: it is never written again
        assert a.n_iters.tolist() == [200, 61, 200, 200, 200, 200]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["k4", "k8"])
def test_against_the_single_start_path(name, dtype):
    from cnmf_amd import factorise
    g, c, a = load(name), MANIFEST["cases"][name], full(name, dtype)
    X = g["X"].astype(dtype)
    worst, identical = 0.0, True
    for r in range(len(c["seeds"])):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W, H, n_iter = factorise(X, g["W0" + SUFFIX[dtype]][r], g["H0" + SUFFIX[dtype]][r], n_components=c["k"],
                                     init="custom", solver="hals", device="cuda:0", **c["kwargs"])
        ew, eh = rel(a.W_all[r], W.astype(np.float64)), rel(a.H_all[r], H.astype(np.float64))
        worst = max(worst, ew, eh)
        identical = identical and np.array_equal(W, a.W_all[r]) and np.array_equal(H, a.H_all[r])
        assert n_iter == a.n_iters[r]
        assert ew <= BAR[dtype] and eh <= BAR[dtype]
    print(f"{name} {dtype.__name__}: largest difference to factorise(solver='hals') {worst:.2e}; "
          f"bit-identical: {identical}")


@pytest.mark.parametrize("F, k, dtype", [(146, 4, np.float32), (74, 3, np.float64), (482, 7, np.float32)],
                         ids=["146-k4-f32", "74-k3-f64", "482-k7-f32"])
def test_single_start_bits_at_the_widths_where_lds_decides_the_teams(F, k, dtype):
    """Widths at which one more team just fits or just does not fit the LDS, with enough tiles per
    workgroup for the most teams: every start is factorise(solver='hals') bit for bit."""
    from cnmf_amd import factorise, factorise_multistart
    from cnmf_amd.synthetic import iop_spectra
    X = iop_spectra(66000, F, seed=12).astype(dtype)
    kw = dict(tol=0.0, max_iter=3)
    res = factorise_multistart(X, k, n_init=2, random_state=5, keep="all", device="cuda:0", **kw)
    for r, seed in enumerate(res.seeds):
        W, H, n_iter = factorise(X, n_components=k, init="random", random_state=seed, solver="hals", device="cuda:0", **kw)
        assert n_iter == res.n_iters[r] == 3
        assert np.array_equal(W, res.W_all[r]) and np.array_equal(H, res.H_all[r])


RAGGED = [
    # n, F, k, R, dtypes, iterations
    (32805, 81, 4, 3, [np.float32], 5),            # 171 workgroups of three tiles, the last tile ragged
    (337, 83, 5, 3, [np.float32], 4),              # rows no multiple of 16 bytes
    (337, 81, 9, 2, [np.float64], 4),              # rows no multiple of 16 bytes
    (337, 512, 16, 2, [np.float64, np.float32], 4),  # the widest row the step serves
    (65, 5, 1, 2, [np.float64, np.float32], 4),    # one row past a tile
]


@pytest.mark.parametrize("n, F, k, R, dtype, iters",
                         [(n, F, k, R, dt, it) for n, F, k, R, dts, it in RAGGED for dt in dts],
                         ids=[f"{n}x{F}-k{k}-{'f64' if dt is np.float64 else 'f32'}"
                              for n, F, k, R, dts, it in RAGGED for dt in dts])
def test_tile_loop_and_ragged_shapes(n, F, k, R, dtype, iters):
    from cnmf_amd import factorise_multistart
    from cnmf_amd.synthetic import iop_spectra, random_init
    X = iop_spectra(n, F, seed=11).astype(dtype)
    kw = dict(tol=0.0, max_iter=iters)
    res = factorise_multistart(X, k, n_init=R, random_state=3, keep="all", device="cuda:0", **kw)
    assert res.seeds == list(range(3, 3 + R)) and res.n_iters.tolist() == [iters] * R
    for r, seed in enumerate(res.seeds):
        W0, H0 = random_init(X, k, seed)
        We, He, ne, ee = restate(X, W0, H0, kw)
        ew, eh, er = rel(res.W_all[r], We), rel(res.H_all[r], He), abs(res.errors[r] - ee) / ee
        print(f"{n}x{F} k={k} {dtype.__name__} start {r}: relW {ew:.2e} relH {eh:.2e} error off by {er:.2e}")
        assert ne == iters and max(ew, eh, er) <= BAR[dtype]


def _snapshot(plan):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in (plan.W, plan.H64, plan.Ht, plan.HHt, plan.ctl, plan.ticket)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name, tol", [("k1", 1e-4), ("k4", 1.0)])
def test_launches_after_the_stop_write_nothing(name, tol, dtype):
    """k1: the starts stop by the rule at 4, 4 and 5; k4 with tol = 1: every start stops after its
    first iteration (six workgroups).  Three more launches per batch change no bit."""
    import torch
    from cnmf_amd.multistart import MS_ITERS_DONE, MS_STOPPED, MultiStartPlan, run_multistart
    g, c = load(name), MANIFEST["cases"][name]
    R = len(c["seeds"])
    plan = MultiStartPlan(torch.from_numpy(g["X"].astype(dtype)).to("cuda:0"), c["k"], R)
    for r in range(R):
        plan.set_start(r, g["W0" + SUFFIX[dtype]][r], g["H0" + SUFFIX[dtype]][r])
    n_iters = run_multistart(plan, max_iter=c["kwargs"]["max_iter"], tol=tol)
    host = plan.read_ctl()
    assert (host[:, MS_STOPPED] == 1.0).all() and (host[:, MS_ITERS_DONE] == n_iters).all()
    assert n_iters.tolist() == (c["n_iter" + SUFFIX[dtype]] if name == "k1" else [1] * R)
    before = _snapshot(plan)
    for _ in range(3):
        for b in range(len(plan.batches)):
            plan.step(b)
    after = _snapshot(plan)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert int(plan.ticket.item()) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_same_call_twice_gives_the_same_bits(dtype):
    a, b = full("k8", dtype), fit("k8", dtype)
    for r in range(len(a.seeds)):
        assert same_bits(a, b, r, r)
    assert a.best == b.best and np.array_equal(a.W, b.W) and np.array_equal(a.H, b.H)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_result_shapes_types_and_the_warning(dtype):
    import torch
    from cnmf_amd import ConvergenceWarning, MultiStartResult, factorise_multistart
    g, c = load("f17"), MANIFEST["cases"]["f17"]
    X, R, k = g["X"].astype(dtype), len(c["seeds"]), c["k"]
    n, F = X.shape
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = factorise_multistart(X, k, n_init=R, random_state=c["seeds"], keep="all", device="cuda:0", **c["kwargs"])
    told = [w for w in caught if issubclass(w.category, ConvergenceWarning)]
    at_cap = sum(i == c["kwargs"]["max_iter"] for i in c["n_iter" + SUFFIX[dtype]])
    assert len(told) == 1 and f"reached by {at_cap} of {R} starts" in str(told[0].message) and at_cap == 2
    assert isinstance(res, MultiStartResult)
    assert res.W_all.shape == (R, n, k) and res.H_all.shape == (R, k, F) and res.W.shape == (n, k) and res.H.shape == (k, F)
    assert isinstance(res.W_all, np.ndarray) and res.W_all.dtype == dtype and res.H_all.dtype == dtype
    assert res.errors.shape == (R,) and res.errors.dtype == np.float64 and res.n_iters.shape == (R,)
    assert isinstance(res.best, int) and isinstance(res.n_iter, int) and res.seeds == c["seeds"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        best = factorise_multistart(X, k, n_init=R, random_state=c["seeds"], device="cuda:0", **c["kwargs"])
        Xt = torch.from_numpy(X).to("cuda:0")
        tres = factorise_multistart(Xt, k, n_init=R, random_state=c["seeds"], keep="all", **c["kwargs"])
    assert best.W_all is None and best.H_all is None and best.best == res.best
    assert np.array_equal(best.W, res.W) and np.array_equal(best.H, res.H)
    tdt = torch.float64 if dtype is np.float64 else torch.float32
    for t in (tres.W, tres.H, tres.W_all, tres.H_all):
        assert isinstance(t, torch.Tensor) and t.device == Xt.device and t.dtype == tdt
    assert np.array_equal(tres.W_all.cpu().numpy(), res.W_all) and np.array_equal(tres.H_all.cpu().numpy(), res.H_all)
    with warnings.catch_warnings(record=True) as caught:  # tol = 0: running to max_iter is what was asked
        warnings.simplefilter("always")
        factorise_multistart(X, k, n_init=2, random_state=0, tol=0.0, max_iter=3, device="cuda:0")
    assert not [w for w in caught if issubclass(w.category, ConvergenceWarning)]


# ---- the batched form (diagnostic library, CNMF_MS_TEAMS): several starts share a staged tile
def _in_diag(call: str, teams: int):
    """Run `call` (an expression over this module, imported as m) in a child on the diagnostic library."""
    code = (f"import sys; sys.path[:0] = [{_ROOT!r}, {os.path.join(_ROOT, 'tests')!r}]; "
            f"import test_gpu_multistart as m; {call}")
    r = subprocess.run([sys.executable, "-u", "-c", code], cwd=_ROOT, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, CNMF_HIP_LIB=_DIAG, CNMF_MS_TEAMS=str(teams)))
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])


def case_batched(name, dtype_name, min_batch):
    """In the child: the golden bars of every start, then the bits of every start from the full run,
    alone, in reversed order and in batches of two and of one; launches after the stop write nothing."""
    import torch
    from cnmf_amd import _lib
    from cnmf_amd.multistart import MultiStartPlan, run_multistart
    dtype = {"f64": np.float64, "f32": np.float32}[dtype_name]
    g, c = load(name), MANIFEST["cases"][name]
    F, k, seeds = c["shape"][1], c["k"], c["seeds"]
    rb = _lib.load().cnmf_ms_batch(F, k, _lib.F64 if dtype is np.float64 else _lib.F32)
    print(f"{name} {dtype_name}: {rb} starts per launch")
    assert rb >= min_batch
    a = fit(name, dtype)
    for r, (We, He, ne, ee) in enumerate(expected(name, dtype)):
        ew, eh, er = rel(a.W_all[r], We), rel(a.H_all[r], He), abs(a.errors[r] - ee) / ee
        print(f"{name} {dtype_name} start {r}: n_iter {a.n_iters[r]} ({ne}) relW {ew:.2e} relH {eh:.2e} error off by {er:.2e}")
        assert a.n_iters[r] == ne and max(ew, eh, er) <= BAR[dtype]
    for r, seed in enumerate(seeds):
        assert same_bits(fit(name, dtype, seeds=[seed]), a, 0, r), (name, "solo", r)
    back, two, one = fit(name, dtype, seeds=seeds[::-1]), fit(name, dtype, _max_batch=2), fit(name, dtype, _max_batch=1)
    for r in range(len(seeds)):
        assert same_bits(back, a, len(seeds) - 1 - r, r), (name, "reversed", r)
        assert same_bits(two, a, r, r), (name, "batches of two", r)
        assert same_bits(one, a, r, r), (name, "batches of one", r)
    assert same_bits(fit(name, dtype), a, 0, 0)  # the same call twice
    # the gate: a batch with stopped and live starts leaves the stopped ones alone (the equalities
    # above, k4's seed 1 stops at 61); and once all have stopped, three more launches change no bit
    plan = MultiStartPlan(torch.from_numpy(g["X"].astype(dtype)).to("cuda:0"), k, len(seeds))
    for r in range(len(seeds)):
        plan.set_start(r, g["W0" + SUFFIX[dtype]][r], g["H0" + SUFFIX[dtype]][r])
    run_multistart(plan, max_iter=3, tol=1.0)
    before = _snapshot(plan)
    for _ in range(3):
        for b in range(len(plan.batches)):
            plan.step(b)
    for x, y in zip(before, _snapshot(plan)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name, dtype_name, teams, min_batch", [
    ("k4", "f32", 2, 4), ("k4", "f64", 2, 2), ("k8", "f32", 1, 4), ("k8", "f64", 2, 2), ("f17", "f32", 4, 5)])
def test_batched_form_on_the_diagnostic_library(name, dtype_name, teams, min_batch):
    _in_diag(f"m.case_batched({name!r}, {dtype_name!r}, {min_batch})", teams)
