"""CPU: the dispatch of cnmf_mu_sample_pass, read through cnmf_pass_describe (host only), against the
case table tests/pass_cases.py runs on the GPU.

Completeness: every kernel the dispatch can choose for any dtype, F <= 1024, k <= 16 and either flag
set (the updating / accumulating pass, the loss pass) is run by at least one row of the table, in the
same role (over every tile, over the full tiles, on a ragged tail).  A kernel variant added later
fails here until it gets a row.  Limits: the widest F per dtype and padded k, pinned to the table's
WIDEST, and the refusals past them.
"""
import collections

import pytest

import pass_cases as pc
from cnmf_amd import _lib

UPDATE = _lib.PASS_UPDATE_W | _lib.PASS_ACCUMULATE
FLAG_SETS = (UPDATE, _lib.PASS_LOSS)

# Families whose single-pass parity another file owns; every mu_pass_kernel and mu_pass_mfma_kernel
# instantiation must have a row of its own:
#   mu_pass_bf16_mfma_kernel, mu_pass_bfw_kernel - the bf16 matrix-core pair:
#       test_gpu_parity.py::test_bf16_mfma_single_pass_matches_numpy
#   mu_pass_sl_kernel - the sample-lane kernel: test_gpu_persistent.py / test_gpu_cfg3.py
EXEMPT_FAMILIES = ("mu_pass_bf16_mfma_kernel", "mu_pass_bfw_kernel", "mu_pass_sl_kernel")


def _family(kernel):
    return kernel.split("<")[0]


def _covered(rows):
    got = collections.defaultdict(list)
    for row in rows:
        dt, F, k, N, _ = row
        n = None if N == pc.MULTI else N  # MULTI: full tiles and a ragged one
        for flags in FLAG_SETS:
            st, text = pc.describe(dt, F, k, flags)
            assert st == 0, (row, flags, _lib.load().cnmf_last_error())
            for role, kernel in pc.kernels(text, n):
                got[flags, role, kernel].append(row)
    return got


@pytest.fixture(scope="module")
def dispatch():
    """{(flags, role, kernel): first shape} over every dtype × F in 1..1024 × k in 1..16."""
    seen = {}
    for dt in pc.DTYPES:
        for k in range(1, 17):
            for F in range(1, 1025):
                for flags in FLAG_SETS:
                    st, text = pc.describe(dt, F, k, flags)
                    if st == 0:
                        for role, kernel in pc.kernels(text):
                            seen.setdefault((flags, role, kernel), (dt, F, k))
    return seen


def _missing(dispatch, rows):
    got = _covered(rows)
    return sorted((key, shape) for key, shape in dispatch.items()
                  if _family(key[2]) not in EXEMPT_FAMILIES and key not in got)


def test_every_dispatched_kernel_has_a_row(dispatch):
    families = {_family(key[2]) for key in dispatch}
    assert families == {"mu_pass_kernel", "mu_pass_mfma_kernel", *EXEMPT_FAMILIES}, families
    missing = _missing(dispatch, pc.ROWS)
    assert not missing, "kernels no row of tests/pass_cases.py runs (flags, role, kernel), first shape:\n" + \
        "\n".join(f"  {key} at {shape}" for key, shape in missing)
    got = _covered(pc.ROWS)
    for key in sorted(got):
        print(f"{len(got[key]):3d} rows: flags={key[0]} {key[1]:5s} {key[2]}")


def test_a_row_that_alone_covers_a_kernel_cannot_leave(dispatch):
    """Dropping the only row of an instantiation is noticed: the fp64 wide-row NPW = 2 kernel of
    KP = 8 has the rows past F + k = 256 only; the sample-lane shape's VALU tail needs a ragged N."""
    def without(pred):
        return [r for r in pc.ROWS if not pred(r)]
    m = _missing(dispatch, without(lambda r: r[0] == "float64" and r[1] + r[2] > 256 and 5 <= r[2] <= 8))
    assert [key[2] for key, _ in m] == ["mu_pass_kernel<TX=f64, KP=8, FT=0, NPW=2, SPLIT=0>"] * 2, m
    m = _missing(dispatch, without(lambda r: r[:3] == ("float32", 81, 4) and r[3] % 64 != 0))
    assert (UPDATE, "tail", "mu_pass_kernel<TX=f32, KP=4, FT=81, NPW=2, SPLIT=1>") in [key for key, _ in m], m


def test_rows_are_unique_and_accepted():
    ids = [pc.row_id(r) for r in pc.ROWS]
    assert len(set(ids)) == len(ids), [i for i, n in collections.Counter(ids).items() if n > 1]
    for dt, F, k, N, _ in pc.ROWS:
        assert dt in pc.DTYPES and F >= 1 and 1 <= k <= 16 and (N >= 1 or N == pc.MULTI)
    # bf16 rows meant for the VALU / F = 81 passes stay off the bf16 matrix-core pair
    for dt, F, k, N, _ in pc.ROWS:
        if dt == "bfloat16":
            assert "bf" not in _family(pc.describe(dt, F, k, UPDATE)[1]), (F, k)


def test_description_carries_the_launch_parameters():
    st, text = pc.describe("float32", 300, 9, UPDATE)
    assert st == 0 and text.startswith("mu_pass_kernel<TX=f32, KP=16, FT=0, NPW=2, SPLIT=0> lds=")
    # the LDS carve (cnmf_hip.hip pass_lds): X tile 64·F + 4 words, two W tiles, Ht, HHt, 16 zero bytes
    assert pc.lds_bytes(text) == [(64 * 300 + 4) * 4 + 2 * 64 * 16 * 4 + 300 * 16 * 4 + 16 * 16 * 8 + 16]
    st, text = pc.describe("float32", 81, 4, UPDATE)
    assert st == 0 and pc.kernels(text) == {("full", "mu_pass_sl_kernel"),
                                            ("tail", "mu_pass_kernel<TX=f32, KP=4, FT=81, NPW=2, SPLIT=1>")}
    # the loss pass never takes a matrix-core kernel
    for dt, F, k in (("float32", 81, 5), ("bfloat16", 81, 8), ("bfloat16", 320, 16), ("float32", 81, 4)):
        st, text = pc.describe(dt, F, k, _lib.PASS_LOSS)
        assert st == 0 and pc.kernels(text) == {("grid", text.split(" lds=")[0])} and text.startswith("mu_pass_kernel<"), text
    lib = _lib.load()
    assert lib.cnmf_pass_describe(81, 4, 0, 0, b"\0" * 64, 64) == -1 and b"flags" in lib.cnmf_last_error()
    assert lib.cnmf_pass_describe(81, 4, 0, _lib.PASS_ACCUMULATE, b"\0" * 64, 64) == -1
    assert lib.cnmf_pass_describe(81, 4, 9, UPDATE, b"\0" * 64, 64) == -1 and b"x_dtype" in lib.cnmf_last_error()
    assert lib.cnmf_pass_describe(81, 4, 0, UPDATE, None, 64) == -1


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("KP", [4, 8, 16])
def test_widest_F_and_the_refusals_past_it(dtype, KP):
    lib = _lib.load()
    k = KP

    def ok(F):
        return pc.describe(dtype, F, k, UPDATE)[0] == 0
    lo, hi = 1, 4096  # accepted, refused
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert lo == pc.WIDEST[dtype, KP], (dtype, KP, lo)
    # the bisection's premise: every F up to the widest is accepted, and by the loss pass as well
    for flags in FLAG_SETS:
        assert all(pc.describe(dtype, F, k, flags)[0] == 0 for F in range(1, lo + 1))
        st, _ = pc.describe(dtype, lo + 1, k, flags)
        assert st == -3 and lib.cnmf_last_error(), (st, lib.cnmf_last_error())
    # a smaller k of the same padding is no narrower
    assert all(pc.describe(dtype, lo, kk, UPDATE)[0] == 0 for kk in range(KP // 2 + 1, KP + 1))
    st, _ = pc.describe(dtype, 10, 17, UPDATE)
    assert st == -3 and b"k=17" in lib.cnmf_last_error()
    st, _ = pc.describe(dtype, 0, k, UPDATE)
    assert st == -2 and lib.cnmf_last_error()
    assert pc.describe(dtype, 10, 0, UPDATE)[0] == -2
