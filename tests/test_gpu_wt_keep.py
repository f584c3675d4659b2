"""X kept in the Infinity Cache across MU iterations (PersistArgs::x_keep16): the share
of X that mu_iter_wt_kernel loads with the default cache policy changes no bit of the result.

The share is chosen per launch by csrc/keep.hpp; the diagnostic library's CNMF_WT_KEEP16 overrides it,
so each case runs in a child process with CNMF_HIP_LIB = cnmf_amd/libcnmf_hip_diag.so (as
tests/test_gpu_mf8.py does) and CNMF_WT_MAXG=2 (two workgroups, 8 waves: many tile positions per wave,
so that the 16-position pattern wraps inside a wave and across the iteration boundary).  For the
shares 0 (every load `nt`, the kernel before the change), 5, 11 and 16 (every load default policy) W
and H must be bit-identical, in one launch and split in two, with the error word clean and the
counters at rest; the share-0 result is held against the fp64 oracle at 1e-5."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_io import rel_fro
from oracle import mu_ref

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIAG = os.path.join(_ROOT, "cnmf_amd", "libcnmf_hip_diag.so")
KEEPS = (0, 5, 11, 16)


def _in_diag(call: str, **env):
    """Run `call` (an expression over this module, imported as m) in a child on the diagnostic library."""
    code = (f"import sys; sys.path[:0] = [{_ROOT!r}, {os.path.join(_ROOT, 'tests')!r}]; "
            f"import test_gpu_wt_keep as m; {call}")
    r = subprocess.run([sys.executable, "-u", "-c", code], cwd=_ROOT, capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, CNMF_HIP_LIB=_DIAG, CNMF_WT_MAXG="2", **env))
    print(r.stdout[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])


def _plan(X, W0, H0):
    import torch
    from cnmf_amd.solver import MUPlan
    plan = MUPlan(torch.from_numpy(X).cuda(), W0.shape[1])
    plan.set_W(torch.from_numpy(W0))
    plan.set_H(torch.from_numpy(H0))
    return plan


def _done(plan):
    plan.check_sync_error()
    assert plan.counters_at_rest()
    return plan.W.clone(), plan.H64.clone()


def _oracle(X, W0, H0, iters):
    return mu_ref.mu_fit(X.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64),
                         max_iter=iters, tol=0.0)[:2]


def case_iterations(n, k, splits, streamed):
    """sum(splits) iterations in one launch and as the launches of `splits`, for every share."""
    import torch
    from cnmf_amd.synthetic import iop_spectra, random_init
    X = iop_spectra(n, 81, seed=n % 1009, dtype=np.float32)
    W0, H0 = random_init(X, k, 42)
    iters = sum(splits)
    Wr, Hr = _oracle(X, W0, H0, iters)
    ref = None
    for keep in KEEPS:
        os.environ["CNMF_WT_KEEP16"] = str(keep)  # read by the diagnostic library at every launch
        a = _plan(X, W0, H0)
        d = a.describe()
        assert a.persistent and "mu_iter_wt_kernel" in d and "(2 workgroups)" in d, d
        assert ("streamed" in d) == streamed and ("40 tiles per wave resident" in d) == streamed, d
        a.iterate(iters)
        Wa, Ha = _done(a)
        c = _plan(X, W0, H0)
        for m in splits:
            c.iterate(m)
        Wc, Hc = _done(c)
        assert torch.equal(Wa, Wc) and torch.equal(Ha, Hc), f"share {keep}: the split launches differ"
        if ref is None:
            ref = (Wa, Ha)
            ew, eh = rel_fro(Wa.cpu().numpy(), Wr), rel_fro(Ha.cpu().numpy(), Hr)
            print(f"k{k} {n} x 81, {iters} it, share 0: rel W {ew:.2e} H {eh:.2e}")
            assert ew <= 1e-5 and eh <= 1e-5, (ew, eh)
        assert torch.equal(Wa, ref[0]) and torch.equal(Ha, ref[1]), f"share {keep} differs from share 0"


def case_device_tol(n, iters):
    """cnmf_mu_fit_tol (the TOL instance) with a tolerance that never triggers, for every share."""
    import torch
    from cnmf_amd.synthetic import iop_spectra, random_init
    X = iop_spectra(n, 81, seed=n % 1009, dtype=np.float32)
    W0, H0 = random_init(X, 4, 42)
    Wr, Hr = _oracle(X, W0, H0, iters)
    ref = None
    for keep in KEEPS:
        os.environ["CNMF_WT_KEEP16"] = str(keep)
        a = _plan(X, W0, H0)
        out = a.fit_device_tol(iters, 1e-12)
        assert out is not None and out[0] == iters, out
        Wa, Ha = _done(a)
        if ref is None:
            ref = (Wa, Ha, out[1])
            ew, eh = rel_fro(Wa.cpu().numpy(), Wr), rel_fro(Ha.cpu().numpy(), Hr)
            print(f"k4 {n} x 81, device tolerance, {iters} it, share 0: rel W {ew:.2e} H {eh:.2e}")
            assert ew <= 1e-5 and eh <= 1e-5, (ew, eh)
        assert torch.equal(Wa, ref[0]) and torch.equal(Ha, ref[1]), f"share {keep} differs from share 0"
        assert out[1] == ref[2], f"share {keep}: the checked errors differ"


def test_k4_resident_w_bit_identical_for_every_share():
    """2,352 rows = 147 tiles over 8 waves: 18 per wave, 3 waves with one more."""
    _in_diag("m.case_iterations(2352, 4, (5, 7), False)")


def test_k8_streamed_w_bit_identical_for_every_share():
    """9,640 rows = 1,205 tiles of 8 samples over 8 waves (150 per wave, ragged), 40 of them W-resident."""
    _in_diag("m.case_iterations(9640, 8, (2, 4), True)", CNMF_WT_NRES="40")


def test_k4_device_tolerance_bit_identical_for_every_share():
    _in_diag("m.case_device_tol(2352, 20)")
