"""solver='hals' over row shards on the GPU (cnmf_hals_shard_step, an all-reduce, cnmf_hals_basis).

* one process: the split form of the iteration gives the bits of the one launch (W, H64, Ht, HHt,
  the control block, the ticket), also across a stop inside a stretch;
* worlds 2 and 3, the ranks processes sharing cuda:0 over gloo (RCCL needs distinct devices; the
  kernels and the host orchestration are the same), through factorise_sharded(solver='hals'): the
  bars of tests/test_gpu_hals.py — float64 X: sklearn's n_iter, W and H within 1e-9 relative
  Frobenius of sklearn's own answer (tests/golden/hals_*.npz); float32 X: the same n_iter and 1e-5
  against tests/hals_ref.py run in fp64 from the rounded inputs — with H bit-identical on every rank;
* a rank without rows; the same fit twice.
One spawn per world runs all of that world's fits."""
import datetime
import functools
import json
import os
import socket
import warnings

import numpy as np
import pytest

import hals_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "MANIFEST_hals.json")) as f:
    MANIFEST = json.load(f)
BAR = {np.float64: 1e-9, np.float32: 1e-5}
DTYPES = [np.float64, np.float32]
SHARDED_CASES = ["k4", "k16", "reg", "dead", "f17", "transform"]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@functools.lru_cache(maxsize=None)
def load(name):
    g = np.load(os.path.join(GOLDEN, f"hals_{name}.npz"))
    return {k: g[k] for k in g.files}


def regs(name):
    """(l1_W, l1_H, l2_W, l2_H) from the case's GLOBAL shape."""
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


# ---- one process: the split form against the one launch -------------------------------------------

def _state(plan):
    import torch
    torch.cuda.synchronize()
    return [t.clone() for t in (plan.W, plan.H64, plan.Ht, plan.HHt, plan.ctl, plan.ticket)]


def _pair(X, W0, H0, max_iter, tol, reg=(0.0, 0.0, 0.0, 0.0), update_H=True):
    """The same fit by the one launch and by the split form: [(plan, n_iter)] * 2."""
    import torch
    from cnmf_amd.solver import HALSPlan, run_hals
    dev = torch.device("cuda:0")
    out = []
    for split in (False, True):
        plan = HALSPlan(torch.from_numpy(X).to(dev), H0.shape[0], reg[0], reg[2], reg[1], reg[3], split=split)
        assert plan.split is split and plan.world == 1 and (plan.acc is not None) is split
        if W0 is None:
            plan.W.zero_()
        else:
            plan.set_W(torch.from_numpy(W0))
        plan.set_H(torch.from_numpy(H0))
        out.append((plan, run_hals(plan, max_iter=max_iter, tol=tol, update_H=update_H)))
    return out


def _assert_same_bits(one, split):
    import torch
    for name, a, b in zip(("W", "H64", "Ht", "HHt", "ctl", "ticket"), _state(one), _state(split)):
        assert torch.equal(a, b), name
    assert int(split.ticket.item()) == 0  # the ticket word is left zero


@pytest.mark.parametrize("name, dtype", [("k4", np.float32), ("k4", np.float64), ("k16", np.float64),
                                         ("transform", np.float32), ("transform", np.float64)],
                         ids=["k4-f32", "k4-f64", "k16-f64", "transform-f32", "transform-f64"])
def test_split_form_gives_the_bits_of_the_one_launch(name, dtype):
    from cnmf_amd.solver import HALS_ITERS_DONE, HALS_STOPPED
    g, c = load(name), MANIFEST["cases"][name]
    W0 = g["W0"].astype(dtype) if c["update_H"] else None
    (one, n1), (split, n2) = _pair(g["X"].astype(dtype), W0, g["H0"].astype(dtype), c["kwargs"]["max_iter"],
                                   c["kwargs"]["tol"], regs(name), c["update_H"])
    assert n1 == n2 == c["n_iter"] and n1 % 16 != 0  # a tol stop inside a stretch: gated launches followed it
    _assert_same_bits(one, split)
    before = _state(split)
    assert before[4][HALS_STOPPED] == 1.0 and before[4][HALS_ITERS_DONE] == c["n_iter"]
    acc = split.acc.clone()
    for _ in range(3):  # after a stop both launches write nothing
        split.step(c["update_H"])
    import torch
    for a, b in zip(before, _state(split)):
        assert torch.equal(a, b)
    assert torch.equal(acc, split.acc)
    assert "hals_shard_step_kernel" in split.describe() and "hals_step_kernel" in one.describe()


def test_split_form_with_every_workgroup_looping_and_a_ragged_last_tile():
    from cnmf_amd import _lib
    from cnmf_amd.synthetic import iop_spectra, random_init
    n = 64 * 2 * 256 + 37
    assert _lib.load().cnmf_hals_rows(n) == 171
    X = iop_spectra(n, 81, seed=31)
    W0, H0 = random_init(X, 4, 31)
    (one, n1), (split, n2) = _pair(X, W0, H0, 10, 0.0)
    assert n1 == n2 == 10 and one.read_ctl()[0] == 0.0
    _assert_same_bits(one, split)
    # the summed row the ranks would all-reduce: its violation entry is the W-sweep's share
    acc = split.acc.cpu().numpy()
    assert acc.shape == (342,) and 0.0 < acc[4 * 81 + 16] < split.read_ctl()[3] and acc[-1] == 0.0
    assert abs(one.frobenius_error() - split.frobenius_error()) == 0.0


# ---- worlds 2 and 3: processes sharing cuda:0 over gloo ---------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, jobs, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    # a rank that fails leaves its peers in a collective: they give up instead of waiting for ever
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        torch.cuda.set_device(0)
        from cnmf_amd.distributed import factorise_sharded, shard_bounds
        out = {}
        for key, j in jobs.items():
            lo, hi = shard_bounds(j["X"].shape[0], world, rank)
            W0 = None if j["W0"] is None else j["W0"][lo:hi]
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                W, H, n = factorise_sharded(torch.from_numpy(j["X"][lo:hi]), W0, j["H0"], max_iter=j["max_iter"],
                                            tol=j["tol"], l1_reg_W=j["reg"][0], l1_reg_H=j["reg"][1],
                                            l2_reg_W=j["reg"][2], l2_reg_H=j["reg"][3], update_H=j["update_H"],
                                            solver="hals", exchange=j["exchange"])
            said = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
            out[key] = (lo, hi, W.cpu().numpy(), H.cpu().numpy(), n, said)
        q.put((rank, out, None))
    except Exception as ex:  # reported to the parent, and a non-zero exit code
        q.put((rank, None, f"{type(ex).__name__}: {ex}"))
        raise
    finally:
        dist.destroy_process_group()


def _job(name, dtype, exchange="auto"):
    g, c = load(name), MANIFEST["cases"][name]
    return dict(X=g["X"].astype(dtype), W0=g["W0"].astype(dtype) if c["update_H"] else None, H0=g["H0"].astype(dtype),
                max_iter=c["kwargs"]["max_iter"], tol=c["kwargs"]["tol"], reg=regs(name), update_H=c["update_H"],
                exchange=exchange)


def _jobs(world):
    jobs = {(name, dt.__name__): _job(name, dt) for name in SHARDED_CASES for dt in DTYPES}
    if world == 2:
        jobs[("k4-again", "float32")] = _job("k4", np.float32)
        jobs[("k1-exchange", "float32")] = _job("k1", np.float32, exchange=True)
    if world == 3:  # 2 rows over 3 ranks: rank 2 owns none
        for dt in DTYPES:
            j = _job("k1", dt)
            j.update(X=j["X"][:2].copy(), W0=j["W0"][:2].copy(), max_iter=10, tol=0.0)
            jobs[("empty", dt.__name__)] = j
    return jobs


@functools.lru_cache(maxsize=None)
def world_results(world):
    """Every fit of this world, run once: {key: [per rank (lo, hi, W, H, n_iter, warnings)]}."""
    import torch.multiprocessing as mp
    jobs = _jobs(world)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, jobs, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in procs), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    errs = [r[2] for r in res if r[2]]
    assert not errs, errs
    assert [p.exitcode for p in procs] == [0] * world  # every process exits 0
    return {key: [r[1][key] for r in res] for key in jobs}


def _check_fit(ranks, We, He, ne, dtype, label, silent=True):
    W = np.concatenate([r[2] for r in ranks])
    H = ranks[0][3]
    ew, eh = rel(W, We), rel(H, He)
    print(f"{label}: n_iter {[r[4] for r in ranks]} ({ne}) shards {[r[1] - r[0] for r in ranks]} relW {ew:.2e} relH {eh:.2e}")
    assert all(r[4] == ne for r in ranks)                     # n_iter: equal on all ranks, and the expected
    assert all(np.array_equal(r[3], H) for r in ranks[1:])    # H: bit-identical on all ranks
    assert not silent or all(r[5] == [] for r in ranks)       # exchange='auto' takes the all-reduce path silently
    assert W.dtype == dtype and H.dtype == dtype and W.shape == We.shape
    assert ew <= BAR[dtype] and eh <= BAR[dtype]
    return W, H


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", SHARDED_CASES)
@pytest.mark.parametrize("world", [2, 3])
def test_factorise_sharded_matches_sklearn(world, name, dtype):
    ranks = world_results(world)[(name, dtype.__name__)]
    We, He, ne = expected(name, dtype)
    assert ne == MANIFEST["cases"][name]["n_iter"]
    W, H = _check_fit(ranks, We, He, ne, dtype, f"world {world} {name} {dtype.__name__}")
    if name == "f17":  # no shard a multiple of the 64-row tile
        assert [r[1] - r[0] for r in ranks] == ([75, 75] if world == 2 else [50, 50, 50])
    if name == "dead":  # both hess == 0 branches: the component stays exactly as it is
        assert not W[:, 2].any() and not H[2].any() and not W[::9].any()
    if name == "transform":  # W_shard=None, update_H=False: H comes back as it went in
        assert np.array_equal(H, load(name)["H0"].astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_rank_without_rows(dtype):
    ranks = world_results(3)[("empty", dtype.__name__)]
    assert [(r[0], r[1]) for r in ranks] == [(0, 1), (1, 2), (2, 2)] and ranks[2][2].shape == (0, 1)
    g = load("k1")
    r = ref.fit(g["X"][:2].astype(dtype).astype(np.float64), g["W0"][:2].astype(dtype).astype(np.float64),
                g["H0"].astype(dtype).astype(np.float64), tol=0.0, max_iter=10)
    _check_fit(ranks, r["W"], r["H"], 10, dtype, f"world 3 empty {dtype.__name__}")


def test_same_sharded_fit_twice_is_bit_identical():
    res = world_results(2)
    for a, b in zip(res[("k4", "float32")], res[("k4-again", "float32")]):
        assert a[2] is not b[2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4] == 61


def test_exchange_true_warns_and_takes_the_all_reduce_path():
    ranks = world_results(2)[("k1-exchange", "float32")]
    for r in ranks:
        assert len(r[5]) == 1 and "in-launch exchange not used" in r[5][0] and "solver='hals'" in r[5][0]
    We, He, ne = expected("k1", np.float32)
    _check_fit(ranks, We, He, ne, np.float32, "world 2 k1 exchange=True", silent=False)
