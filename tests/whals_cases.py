"""The weighted cases of solver='whals' that tests/test_gpu_whals.py runs on the GPU and whose
reference runs tests/test_whals_ref.py checks on the CPU (every case with tol > 0 stops at least
0.1 % away from tol, the goldens' own margin, so the GPU's last bits cannot move n_iter).  Inputs
are rounded once to the case's dtype (the 333 x 81 cases start from the X, W0 and H0 of
tests/golden/hals_k4.npz, whose unweighted fit stops after 61 iterations); the reference
(tests/whals_ref.py) runs in fp64 from the rounded inputs."""
import functools
import os

import numpy as np

import hals_ref
import whals_ref as ref

# name: shape, k, dtypes, tol, max_iter, share of zero weights, regularisation, update_H, seed
CASES = {
    "w30": dict(shape=(333, 81), k=4, dtypes=("f64", "f32"), tol=1e-4, max_iter=200, zeros=0.3, seed=51),
    "w30reg": dict(shape=(333, 81), k=4, dtypes=("f64", "f32"), tol=1e-4, max_iter=200, zeros=0.3, seed=51,
                   reg=dict(alpha_W=0.01, alpha_H=0.02, l1_ratio=0.5)),
    "transform": dict(shape=(333, 81), k=4, dtypes=("f64", "f32"), tol=1e-4, max_iter=200, zeros=0.3, seed=51,
                      update_H=False),
    "k5f83": dict(shape=(337, 83), k=5, dtypes=("f32",), tol=0.0, max_iter=10, zeros=0.3, seed=43),
    "k8f81": dict(shape=(337, 81), k=8, dtypes=("f64",), tol=0.0, max_iter=10, zeros=0.3, seed=44),
    "corner8": dict(shape=(64, 128), k=8, dtypes=("f64", "f32"), tol=0.0, max_iter=5, zeros=0.3, seed=45),
    "corner8wide": dict(shape=(48, 192), k=8, dtypes=("f64", "f32"), tol=0.0, max_iter=5, zeros=0.3, seed=46),
    "corner4": dict(shape=(40, 512), k=4, dtypes=("f64", "f32"), tol=0.0, max_iter=5, zeros=0.3, seed=47),
    # k <= 4 with 129 <= F <= 256: 128 feature lanes, two features per lane, two row groups
    "lanes128": dict(shape=(70, 200), k=4, dtypes=("f64", "f32"), tol=0.0, max_iter=5, zeros=0.3, seed=52),
    "many": dict(shape=(32805, 81), k=4, dtypes=("f32",), tol=0.0, max_iter=5, zeros=0.3, seed=48),
    "k1": dict(shape=(100, 7), k=1, dtypes=("f64", "f32"), tol=1e-4, max_iter=200, zeros=0.3, seed=49),
    # whole rows (i % 7 == 3) and columns (f % 5 == 1) at weight zero, unit weights elsewhere
    "masked": dict(shape=(333, 81), k=4, dtypes=("f64", "f32"), tol=1e-4, max_iter=200, zeros=None, seed=50),
}
DTYPE = {"f64": np.float64, "f32": np.float32}
PARAMS = [(name, dt) for name, c in CASES.items() for dt in c["dtypes"]]


def regs(name):
    """(l1_W, l1_H, l2_W, l2_H) of the case."""
    c = CASES[name]
    return hals_ref.regularization(*c["shape"], **c.get("reg", {}))


@functools.lru_cache(maxsize=None)
def inputs(name, dt):
    """X, M, W0 (None for update_H=False), H0 in the case's dtype."""
    from cnmf_amd.synthetic import iop_spectra, random_init
    c = CASES[name]
    n, F = c["shape"]
    dtype = DTYPE[dt]
    if (n, F, c["k"]) == (333, 81, 4):
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hals_k4.npz"))
        X, W0, H0 = (g[a].astype(np.float64) for a in ("X", "W0", "H0"))
    elif F <= 128:
        X = iop_spectra(n, F, seed=c["seed"], dtype=np.float64)
    else:
        X = np.abs(np.random.RandomState(c["seed"]).randn(n, F))
    if (n, F, c["k"]) != (333, 81, 4):
        W0, H0 = random_init(X, c["k"], c["seed"])
    if c["zeros"] is None:
        M = np.ones((n, F))
        M[np.arange(n) % 7 == 3] = 0.0
        M[:, np.arange(F) % 5 == 1] = 0.0
    else:
        M = ref.weights((n, F), c["seed"] + 1000, zeros=c["zeros"])
    return (X.astype(dtype), M.astype(dtype), W0.astype(dtype) if c.get("update_H", True) else None, H0.astype(dtype))


@functools.lru_cache(maxsize=None)
def expected(name, dt):
    """whals_ref's fit in fp64 from the inputs as rounded to the case's dtype."""
    c = CASES[name]
    X, M, W0, H0 = (None if a is None else a.astype(np.float64) for a in inputs(name, dt))
    l1_W, l1_H, l2_W, l2_H = regs(name)
    return ref.fit(X, M, W0, H0, tol=c["tol"], max_iter=c["max_iter"], l1_W=l1_W, l1_H=l1_H, l2_W=l2_W, l2_H=l2_H,
                   update_H=c.get("update_H", True))


def kept(name):
    """The rows and columns of the 'masked' case that carry weight."""
    n, F = CASES[name]["shape"]
    return np.arange(n) % 7 != 3, np.arange(F) % 5 != 1


@functools.lru_cache(maxsize=None)
def expected_submatrix(name, dt):
    """The unweighted hals_ref fit of the rows and columns of `name` that carry weight."""
    c = CASES[name]
    X, M, W0, H0 = (a.astype(np.float64) for a in inputs(name, dt))
    kr, kc = kept(name)
    return hals_ref.fit(X[kr][:, kc], W0[kr], H0[:, kc], tol=c["tol"], max_iter=c["max_iter"])
