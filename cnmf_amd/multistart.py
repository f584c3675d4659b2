"""factorise_multistart: R starts of solver='hals' on the same X, run together and the best kept
(csrc/multistart.hip).  The launch takes a batch of up to cnmf_ms_batch(F, k, dtype)
starts that share each staged tile of X; that form measured slower than one launch per start, so
the library's batch is 1 and an iteration is one launch per live start.

NMF is not convex: the fit depends on the start, and with init='random' the final error differs by
a factor of 2.5 between seeds on the project's synthetic spectra.  The usual answer — run several
starts and keep the best — is here one call: start r is exactly `factorise(X, solver='hals',
init='random', random_state=seeds[r])`, every start stops by sklearn's rule on the device, and the
start with the smallest ‖X − WH‖ is returned.
"""
from __future__ import annotations

import numbers
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib
from . import api as _api
from . import init as _init
from ._lib import check

__all__ = ["factorise_multistart", "MultiStartResult", "MultiStartPlan", "run_multistart", "MS_STRETCH"]

# control-block slots and flags (include/cnmf_hip.h: cnmf_ms_slots, cnmf_ms_flags)
(MS_STOPPED, MS_ITERS_DONE, MS_VIOL_INIT, MS_VIOL_LAST, MS_TOL) = range(5)
MS_STRIDE = 8
MS_UPDATE_H = 1
MS_STRETCH = 16  # iterations enqueued between two reads of the control blocks
MAX_STARTS = 64


@dataclass
class MultiStartResult:
    """What factorise_multistart returns.  W, H, n_iter: the start with the smallest error (the
    lowest index on a tie), `best` its index.  errors[r] = ‖X − W_r·H_r‖ (NMF.reconstruction_err_ of
    the single fit), n_iters[r] the iterations start r ran, seeds[r] its random_state (None for
    init='custom').  W_all (R, n, k) and H_all (R, k, F) with keep='all', else None."""
    W: object
    H: object
    n_iter: int
    best: int
    errors: np.ndarray
    n_iters: np.ndarray
    seeds: object
    W_all: object = None
    H_all: object = None


def _seeds(random_state, n_init):
    """The R seeds: an int s gives s .. s+R-1, a sequence of R ints itself, a RandomState R draws,
    None a base seed drawn from NumPy's global state."""
    top = 2 ** 32 - n_init
    if random_state is None:
        random_state = int(np.random.randint(0, min(top, 2 ** 31 - 1)))
    if isinstance(random_state, np.random.RandomState):
        return [int(s) for s in random_state.randint(0, 2 ** 31 - 1, size=n_init)]
    if isinstance(random_state, numbers.Integral) and not isinstance(random_state, bool):
        if not 0 <= random_state <= top:
            raise ValueError(f"random_state={random_state!r}: an int seed must lie in [0, 2**32 - n_init].")
        return [int(random_state) + r for r in range(n_init)]
    try:
        seeds = list(random_state)
    except TypeError:
        raise TypeError(f"random_state must be None, an int, a sequence of n_init ints or a "
                        f"numpy RandomState. Got {random_state!r}.") from None
    if len(seeds) != n_init:
        raise ValueError(f"random_state holds {len(seeds)} seeds for n_init={n_init} starts.")
    for s in seeds:
        if not isinstance(s, numbers.Integral) or isinstance(s, bool) or not 0 <= s < 2 ** 32:
            raise ValueError(f"random_state: every seed must be an int in [0, 2**32). Got {s!r}.")
    return [int(s) for s in seeds]


def _validate(n_init, init, solver, keep):
    if solver != "hals":
        raise ValueError(f"solver={solver!r} is not available for factorise_multistart: the starts share "
                         "one launch of the HALS sweep ('hals').")
    if init not in ("random", "custom"):
        raise ValueError(f"init={init!r} is not available for factorise_multistart: it takes 'random' or "
                         "'custom'; the other inits are deterministic and give one start.")
    if (not isinstance(n_init, numbers.Integral) or isinstance(n_init, bool)
            or not 1 <= n_init <= MAX_STARTS):
        raise ValueError(f"The 'n_init' parameter must be an int in the range [1, {MAX_STARTS}]. "
                         f"Got {n_init!r} instead.")
    if keep not in ("best", "all"):
        raise ValueError(f"The 'keep' parameter must be a str among {{'all', 'best'}}. Got {keep!r} instead.")


class MultiStartPlan:
    """Device state of a multi-start HALS fit: start-major H64 (R, k, F), Ht (R, F, KP), HHt
    (R, KP, KP) and control blocks (R, MS_STRIDE), the starts grouped into ⌈R / RB⌉ batches of nearly
    equal size, RB = cnmf_ms_batch(F, k, dtype) (or the private max_batch, for tests).  W is one
    start-major array (starts of the batch, n, k) per batch, so that every batch's W starts 16-byte
    aligned whatever n·k is; `W_of(r)` is start r's plain (n, k) matrix, `W` all of them (R, n, k).
    A batch's launches use views of these arrays."""

    def __init__(self, X, n_components: int, n_starts: int, l1_W=0.0, l2_W=0.0, l1_H=0.0, l2_H=0.0,
                 max_batch: int | None = None):
        import torch
        if X.dtype == torch.bfloat16:
            raise TypeError("bfloat16 X is not available for factorise_multistart: pass float32 or float64")
        if X.device.type != "cuda":
            raise ValueError("MultiStartPlan needs X on a HIP device")
        if X.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"unsupported X dtype {X.dtype}")
        if X.dim() != 2:
            raise ValueError("X must be 2-D")
        self.lib = _lib.load()
        self.X = X.contiguous()
        self.device = X.device
        self.n_rows, self.F = (int(s) for s in self.X.shape)
        self.k, self.R = int(n_components), int(n_starts)
        self.tc = X.dtype
        self.xdt = _lib.F32 if X.dtype == torch.float32 else _lib.F64
        self.l1_W, self.l2_W, self.l1_H, self.l2_H = map(float, (l1_W, l2_W, l1_H, l2_H))
        rb = int(check(self.lib.cnmf_ms_batch(self.F, self.k, self.xdt), "cnmf_ms_batch"))
        if max_batch is not None:
            rb = max(1, min(rb, int(max_batch)))
        self.RB = rb
        nb = -(-self.R // rb)
        base, extra = divmod(self.R, nb)
        self.batches, lo = [], 0  # (first start, starts)
        for b in range(nb):
            n = base + (1 if b < extra else 0)
            self.batches.append((lo, n))
            lo += n
        self.KP = int(check(self.lib.cnmf_padded_k(self.k), "cnmf_padded_k"))
        self.rows = int(check(self.lib.cnmf_ms_rows(self.n_rows), "cnmf_ms_rows"))
        widest = max(n for _, n in self.batches)
        row = int(check(self.lib.cnmf_ms_row_doubles(self.F, self.k, widest), "cnmf_ms_row_doubles"))
        dev, f64 = self.device, torch.float64
        R, k, F, KP = self.R, self.k, self.F, self.KP
        self._W = [torch.empty((cnt, self.n_rows, k), dtype=self.tc, device=dev) for _, cnt in self.batches]
        self._batch_of = [(b, r - lo) for b, (lo, cnt) in enumerate(self.batches) for r in range(lo, lo + cnt)]
        self.H64 = torch.zeros((R, k, F), dtype=f64, device=dev)
        self.Ht = torch.zeros((R, F, KP), dtype=f64, device=dev)
        self.HHt = torch.zeros((R, KP, KP), dtype=f64, device=dev)
        self.partials = torch.empty(max(self.rows, 1) * row, dtype=f64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss_buf = torch.zeros(R, dtype=f64, device=dev)
        self.ctl = self.new_ctl()

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def W_of(self, r: int):
        """Start r's W (n, k): a view."""
        b, i = self._batch_of[r]
        return self._W[b][i]

    @property
    def W(self):
        """Every start's W (R, n, k): the batch's array itself when there is one batch, else a copy."""
        import torch
        return self._W[0] if len(self._W) == 1 else torch.cat(self._W)

    def new_ctl(self, tol: float = 0.0):
        """Zeroed control blocks (R, MS_STRIDE) with every start's TOL set."""
        import torch
        host = np.zeros((self.R, MS_STRIDE))
        assert host.size == int(check(self.lib.cnmf_ms_ctl_doubles(self.R), "cnmf_ms_ctl_doubles"))
        host[:, MS_TOL] = tol
        return torch.from_numpy(host).to(self.device)

    def set_start(self, r: int, W, H):
        """Load start r's factors; Ht / HHt derived as HALSPlan.set_H derives them."""
        import torch
        self.W_of(r).copy_(torch.as_tensor(W).to(device=self.device, dtype=self.tc))
        self.H64[r].copy_(torch.as_tensor(H).to(device=self.device, dtype=torch.float64))
        with torch.cuda.device(self.device):
            check(self.lib.cnmf_basis_update(None, self.H64[r].data_ptr(), self.Ht[r].data_ptr(),
                                             self.HHt[r].data_ptr(), self.F, self.k, 0.0, 0.0, 0, None,
                                             self._stream()), "cnmf_basis_update")

    def step(self, batch: int, update_H: bool = True):
        """One iteration of every live start of a batch (a no-op once all of them have stopped)."""
        import torch
        lo, n = self.batches[batch]
        with torch.cuda.device(self.device):
            check(self.lib.cnmf_ms_step(
                self.X.data_ptr(), self.xdt, self._W[batch].data_ptr(), self.H64[lo].data_ptr(),
                self.Ht[lo].data_ptr(), self.HHt[lo].data_ptr(), self.partials.data_ptr(), self.rows,
                self.ticket.data_ptr(), self.ctl[lo].data_ptr(), self.n_rows, self.F, self.k, n,
                self.l1_W, self.l2_W, self.l1_H, self.l2_H, MS_UPDATE_H if update_H else 0, self._stream()),
                "cnmf_ms_step")

    def read_ctl(self) -> np.ndarray:
        """The control blocks (R, MS_STRIDE) as a NumPy array (synchronises)."""
        return self.ctl.cpu().numpy()

    def errors(self) -> np.ndarray:
        """‖X − W_r·H_r‖ of every start: one cnmf_ms_loss launch per batch; synchronises."""
        import torch
        with torch.cuda.device(self.device):
            for b, (lo, n) in enumerate(self.batches):
                check(self.lib.cnmf_ms_loss(
                    self.X.data_ptr(), self.xdt, self._W[b].data_ptr(), self.H64[lo].data_ptr(),
                    self.partials.data_ptr(), self.rows, self.ticket.data_ptr(), self.loss_buf[lo:].data_ptr(),
                    self.n_rows, self.F, self.k, n, self._stream()), "cnmf_ms_loss")
        return np.sqrt(np.maximum(self.loss_buf.cpu().numpy(), 0.0))

    def H(self, r=None):
        """H of start r (all starts for None) in X's dtype."""
        return (self.H64 if r is None else self.H64[r]).to(self.tc)

    def describe(self) -> str:
        if self.RB == 1:
            return (f"cnmf_ms_step: {self.R} starts, one launch per live start and iteration (cnmf_hals_step's "
                    "iteration; X is read once per start)")
        sizes = ", ".join(str(n) for _, n in self.batches)
        return (f"ms_step_kernel: {len(self.batches)} launch(es) per iteration for {self.R} starts (batches of "
                f"{sizes}; at most {self.RB} starts share a launch at this shape), each tile of X staged once "
                "per batch")


def run_multistart(plan: MultiStartPlan, max_iter: int = 200, tol: float = 1e-4, verbose: int = 0,
                   stretch: int | None = None) -> np.ndarray:
    """The driver: per iteration one launch per batch that still has a live start, enqueued in
    stretches of `stretch` iterations with one read of the control blocks per stretch; the rule
    stops each start on the device, which turns its share of the later launches into no-ops.
    Returns n_iters (R,)."""
    from ._trace import trace_range
    stretch = MS_STRETCH if stretch is None else int(stretch)
    if stretch < 1:
        raise ValueError(f"stretch must be >= 1, got {stretch}")
    plan.ctl = plan.new_ctl(tol=float(tol))
    live = [True] * len(plan.batches)
    launched = 0
    host = np.zeros((plan.R, MS_STRIDE))
    while launched < max_iter and any(live):
        n = min(stretch, max_iter - launched)
        with trace_range(f"cnmf:multistart iterations {launched + 1}..{launched + n}"):
            for _ in range(n):
                for b, alive in enumerate(live):
                    if alive:
                        plan.step(b)
        launched += n
        host = plan.read_ctl()
        for b, (lo, cnt) in enumerate(plan.batches):
            live[b] = bool((host[lo:lo + cnt, MS_STOPPED] == 0).any())
        if verbose:
            print(f"multistart: {launched} iterations enqueued, "
                  f"{int((host[:, MS_STOPPED] == 0).sum())} of {plan.R} starts live")
    return host[:, MS_ITERS_DONE].astype(np.int64)


class _Default(int):
    """The default of n_init: 8, and recognisable as not given by the caller."""


_N_INIT = _Default(8)


def factorise_multistart(X, n_components, n_init=_N_INIT, *, W=None, H=None, init="random", solver="hals",
                         tol=1e-4, max_iter=200, alpha_W=0.0, alpha_H="same", l1_ratio=0.0,
                         random_state=None, keep="best", verbose=0, device=None, _max_batch=None):
    """R = n_init fits of `factorise(X, solver='hals')` from different starts, run together on one
    MI355X, and the best of them.

    Every start runs sklearn's coordinate-descent sweep (solver='hals', SK:376-523 with
    shuffle=False), per iteration one launch per batch of up to cnmf_ms_batch(F, k, dtype) starts
    (csrc/multistart.hip; 1 in this build), enqueued 16 iterations at a time with
    one read of all control blocks in between.  Each start stops on the device by sklearn's rule
    (violation <= tol x its first value, tested every iteration); a stopped start is not touched
    again.  A start's factors do not depend on the other starts: start r gives the bits it gives
    alone, and those of factorise(X, solver='hals').

    init='random' (default): start r is the start of `factorise(X, init='random',
    random_state=seeds[r])`, in X's dtype.  random_state: an int s gives seeds s .. s+R-1, a
    sequence of R ints those seeds, a numpy RandomState R seeds drawn from it, None a base seed
    drawn from NumPy's global state.  init='custom': W (R, n, k) and H (R, k, F) hold the starts,
    every slice validated as factorise validates one (X's sign is then not checked, as in factorise);
    n_init must equal R or be left out.
    tol, max_iter, alpha_W, alpha_H, l1_ratio: as factorise.  keep='all' also returns every start's
    factors.  float32 / float64 X on one device, n_components <= 16, at most 512 features, n_init
    in 1..64.

    Returns a MultiStartResult: W, H, n_iter of the start with the smallest ‖X − WH‖ (the lowest
    index on a tie), best, errors (R,), n_iters (R,), seeds, W_all / H_all (keep='all').  NumPy in,
    NumPy out; torch in, torch out on the device; X's dtype.  One ConvergenceWarning when tol > 0
    and any start ran to max_iter."""
    default_n_init = n_init is _N_INIT
    n_init = int(n_init) if default_n_init else n_init
    _validate(n_init, init, solver, keep)
    _api._validate_params(n_components, init, solver, "frobenius", tol, max_iter, alpha_W, alpha_H, l1_ratio)
    if n_components is None or n_components == "auto":
        if init != "custom":
            raise ValueError("factorise_multistart needs n_components as an int for init='random'.")
    X = _api._check_X(X)
    as_torch = _api._is_torch(X)
    torch = _api._torch()
    if as_torch and X.dtype == torch.bfloat16:
        raise TypeError("bfloat16 X is not available for factorise_multistart: pass float32 or float64")
    n_samples, n_features = (int(s) for s in X.shape)
    k = n_components
    if init == "custom":
        for A, whom in ((W, "W"), (H, "H")):
            if A is None:
                raise ValueError(f"NMF (input {whom}) must be provided when init='custom'")
            if (A.dim() if _api._is_torch(A) else np.asarray(A).ndim) != 3:
                raise ValueError(f"init='custom' takes {whom} with one slice per start: "
                                 f"{'(R, n_samples, k)' if whom == 'W' else '(R, k, n_features)'}.")
        W = W if _api._is_torch(W) else np.asarray(W)
        H = H if _api._is_torch(H) else np.asarray(H)
        R = int(H.shape[0])
        if int(W.shape[0]) != R:
            raise ValueError(f"W holds {int(W.shape[0])} starts and H holds {R}.")
        if not default_n_init and n_init != R:
            raise ValueError(f"n_init={n_init} but W and H hold {R} starts.")
        _validate(R, init, solver, keep)
        if k is None or k == "auto":
            k = int(H.shape[1])
        for r in range(R):
            _api._check_init(H[r], (k, n_features), "NMF (input H)")
            _api._check_init(W[r], (n_samples, k), "NMF (input W)")
        if H.dtype != X.dtype or W.dtype != X.dtype:
            raise TypeError("H and W should have the same dtype as X. Got H.dtype = {} and "
                            "W.dtype = {}.".format(_api._dtype_name(H), _api._dtype_name(W)))
        seeds = None
    else:
        if W is not None or H is not None:
            warnings.warn("When init!='custom', provided W or H are ignored. Set  init='custom' to "
                          "use them as initialization.", RuntimeWarning)
        R = int(n_init)
        seeds = _seeds(random_state, R)
        _api._check_non_negative(X, "NMF (input X)")
    k = int(k)
    if k > 16:
        raise ValueError(f"n_components={k} is not supported: the MI355X kernels handle 1..16.")
    if n_features > 512:
        raise ValueError(f"n_features={n_features} is not supported by factorise_multistart (1..512).")
    regs = _api._compute_regularization(n_samples, n_features, alpha_W, alpha_H, l1_ratio)

    # ---- device work from here
    dev = torch.device(device) if device is not None else (
        X.device if as_torch and X.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
    Xd = (X if as_torch else torch.from_numpy(np.ascontiguousarray(X))).to(dev).contiguous()
    plan = MultiStartPlan(Xd, k, R, regs[0], regs[2], regs[1], regs[3], max_batch=_max_batch)
    if init == "custom":
        for r in range(R):
            plan.set_start(r, W[r] if as_torch or _api._is_torch(W) else np.ascontiguousarray(W[r]),
                           H[r] if as_torch or _api._is_torch(H) else np.ascontiguousarray(H[r]))
    else:
        Xh = X if not as_torch else X.detach().to("cpu").numpy()
        for r, seed in enumerate(seeds):
            W0, H0 = _init.initialize_nmf(Xh, k, init="random", random_state=seed)
            plan.set_start(r, np.ascontiguousarray(W0), np.ascontiguousarray(H0))
    if verbose:
        print(plan.describe())
    n_iters = run_multistart(plan, max_iter=max_iter, tol=tol, verbose=verbose)
    errors = plan.errors()
    best = int(np.argmin(errors))  # the first minimum: ties go to the lowest index
    at_cap = int((n_iters == max_iter).sum())
    if tol > 0 and at_cap:
        warnings.warn("Maximum number of iterations %d reached by %d of %d starts. Increase it to improve "
                      "convergence." % (max_iter, at_cap, R), _api.ConvergenceWarning)
    out = lambda t: _api._out(t, as_torch, X)  # noqa: E731
    return MultiStartResult(
        W=out(plan.W_of(best).clone()), H=out(plan.H(best)), n_iter=int(n_iters[best]), best=best, errors=errors,
        n_iters=n_iters, seeds=None if seeds is None else list(seeds),
        W_all=out(plan.W) if keep == "all" else None, H_all=out(plan.H()) if keep == "all" else None)
