"""cnmf_amd — constrained NMF on AMD MI355X (gfx950).

The caller-facing API mirrors scikit-learn's Frobenius multiplicative-update NMF (the algorithm the
reference AI-for-Ocean-Science/cnmf declares; its own package is empty):

    W, H, n_iter = cnmf_amd.factorise(X, n_components=4, init="random", random_state=42, tol=0)
    model = cnmf_amd.NMF(n_components=4).fit(X)
    model = cnmf_amd.MiniBatchNMF(n_components=4, batch_size=65536).fit(X)   # online MU, fewer passes
    res = cnmf_amd.factorise_multistart(X, 4, n_init=8, random_state=0)       # 8 HALS starts, the best

The hot loop runs in libcnmf_hip.so (hand-written HIP for gfx950, C ABI in include/cnmf_hip.h);
there is no CPU fallback.  See DESIGN.md.
"""
from ._lib import HipLibraryError
from ._trace import tracing
from .api import NMF, ConvergenceWarning, factorise, fit, non_negative_factorization
from .minibatch import MiniBatchNMF
from .multistart import MultiStartResult, factorise_multistart
from .spa import spa, spa_init

__version__ = "0.1.0"
__all__ = ["factorise", "fit", "non_negative_factorization", "NMF", "MiniBatchNMF", "spa", "spa_init",
           "factorise_multistart", "MultiStartResult",
           "ConvergenceWarning", "HipLibraryError", "tracing", "__version__"]
