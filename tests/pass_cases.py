"""The case table of the MU pass dispatch (cnmf_mu_sample_pass): one row per shape the single-launch
parity tests run, shared by tests/test_pass_dispatch_cpu.py (every kernel the dispatch can choose has
a row) and tests/test_gpu_pass_matrix.py (every row against NumPy fp64).

A row is (dtype, F, k, N, note).  N = MULTI stands for 64·(2·cap) + 37 rows, cap being the grid cap
of the row's kernel on the device at hand (cnmf_pass_blocks of a very tall N): every workgroup then
loops over at least two tiles, the last one ragged.
"""
import ctypes
import zlib

import numpy as np

DTYPES = ("float32", "float64", "bfloat16")
MULTI = -1
RAGGED = 64 * 5 + 17  # N % 64 odd: with an odd F (and k) the tile's X / W bytes are no multiple of 16

# the widest n_features the pass accepts per (dtype, padded k) at k = KP; test_pass_dispatch_cpu.py
# pins them to what the library answers.  The LDS tile sets all but bf16 at KP = 4,
# where the 16 64-lane passes of the A phase do: F + k <= 1024.
WIDEST = {
    ("float32", 4): 586, ("float32", 8): 552, ("float32", 16): 479,
    ("float64", 4): 289, ("float64", 8): 268, ("float64", 16): 226,
    ("bfloat16", 4): 1020, ("bfloat16", 8): 994, ("bfloat16", 16): 799,
}


def _k_for(dtype, KP, V):
    """The k of a row with F + k = V: k = KP for an even V and a k the padding serves (1, 5, 9) for
    an odd one; bf16 at KP = 16 takes k = 13 / 14, whose F = V - k is no multiple of 4 for the V
    used here (a multiple of 4 goes to the bf16 matrix-core kernels instead)."""
    if dtype == "bfloat16" and KP == 16:
        return 14 if V % 2 else 13
    return {4: 1, 8: 5, 16: 9}[KP] if V % 2 else KP


def _rows():
    rows = []
    for dt in DTYPES:
        for KP in (4, 8, 16):
            wide = WIDEST[dt, KP]
            # the shape variants of mu_pass_kernel: F + k <= 64, 65..128 (SPLIT), then the wide rows
            # whose A phase deals 64-lane passes to the waves (NPW = 1, 2, 4), each boundary from
            # both sides
            for V in (24, 64, 65, 128, 129, 256, 257, 512, 513):
                k = _k_for(dt, KP, V)
                if V - k <= wide:
                    rows.append((dt, V - k, k, RAGGED, f"F + k = {V}"))
            kw = 13 if (dt == "bfloat16" and KP == 16) else KP
            rows.append((dt, wide, kw, RAGGED, "the widest F of this dtype and padded k"))
    # the F = 81 instantiations: fp64 always on mu_pass_kernel<FT = 81>; fp32 / bf16 on the F = 81
    # matrix-core pass (their loss pass on mu_pass_kernel<FT = 81>); fp32 k = 4 is the sample-lane
    # shape, its ragged tail on the VALU kernel
    for k in (3, 4, 7, 8, 9, 16):
        rows.append(("float64", 81, k, RAGGED, "FT = 81"))
    for k in (1, 3, 4, 5, 8, 9, 16):
        rows.append(("float32", 81, k, RAGGED, "F = 81 matrix-core pass" if k != 4 else "sample-lane + VALU tail"))
    for k in (1, 4, 7, 8, 12, 16):
        rows.append(("bfloat16", 81, k, RAGGED, "F = 81 matrix-core pass"))
    # F < 4 and F no multiple of 4: feat_per_wave rounds up, quarters read past the row
    for dt in ("float32", "float64"):
        for F in (1, 2, 3, 5, 6, 7):
            for k in (1, 4, 5):
                rows.append((dt, F, k, RAGGED, "narrow row"))
    # k below the padding at KP = 16, and bf16 with k >= 9 kept on the VALU pass by F % 4 != 0
    rows += [("float32", 37, 13, RAGGED, "k < KP"), ("float64", 37, 13, RAGGED, "k < KP"),
             ("bfloat16", 37, 9, RAGGED, "k >= 9, F % 4 != 0"), ("bfloat16", 30, 16, RAGGED, "k >= 9, F % 4 != 0"),
             ("bfloat16", 17, 5, RAGGED, "bf16 on the VALU pass"), ("bfloat16", 300, 3, RAGGED, "bf16 wide row")]
    # N = 1, 63, 64, 65: no full tile, one ragged tile, exactly one tile, one sample past it
    for dt, F, k in (("float32", 17, 4), ("float64", 37, 5), ("bfloat16", 17, 8),      # SPLIT
                     ("float32", 200, 9), ("float64", 150, 4), ("bfloat16", 301, 16),  # wide rows
                     ("float32", 81, 5), ("bfloat16", 81, 8), ("float32", 81, 4)):     # F = 81 families
        for N in (1, 63, 64, 65):
            rows.append((dt, F, k, N, "edge N"))
    # several tiles per workgroup: the prefetch of the next tile during this one's compute, and
    # stage_tile's loop past the register depth on every tile
    rows += [("float32", 17, 4, MULTI, "narrow"), ("float64", 17, 5, MULTI, "narrow"),
             ("bfloat16", 17, 8, MULTI, "narrow"),
             ("float32", 125, 4, MULTI, "NPW = 1"), ("float32", 249, 8, MULTI, "NPW = 2"),
             ("float32", 509, 4, MULTI, "NPW = 4"), ("float64", 200, 4, MULTI, "fp64 NPW = 1"),
             ("float32", 81, 5, MULTI, "F = 81 matrix-core pass"),
             ("bfloat16", 81, 8, MULTI, "F = 81 matrix-core pass")]
    return rows


ROWS = _rows()


def row_id(row):
    dt, F, k, N, _ = row
    return f"{dt}-F{F}-k{k}-N{'multi' if N == MULTI else N}"


def xdt(dtype):
    from cnmf_amd import _lib
    return {"float32": _lib.F32, "float64": _lib.F64, "bfloat16": _lib.BF16}[dtype]


def describe(dtype, F, k, flags):
    """(status, text) of cnmf_pass_describe; text is "" for a refused shape."""
    from cnmf_amd import _lib
    buf = ctypes.create_string_buffer(320)
    st = _lib.load().cnmf_pass_describe(F, k, xdt(dtype), flags, buf, 320)
    return st, (buf.value.decode() if st == 0 else "")


def kernels(text, n_rows=None):
    """The kernels a description names, as (role, kernel without its LDS bytes): role "grid" for a
    kernel over every tile, "full" / "tail" for the two families that split the full 64-sample
    tiles from a ragged tail.  With n_rows, only the kernels a launch of that many rows runs."""
    def strip(s):
        return s.split(" lds=")[0].strip()
    if "; ragged tail: " not in text:
        return {("grid", strip(text))}
    full, tail = text.split("; ragged tail: ")
    out = set()
    if n_rows is None or n_rows >= 64:
        out.add(("full", strip(full)))
    if n_rows is None or n_rows % 64:
        out.add(("tail", strip(tail)))
    return out


def lds_bytes(text):
    return [int(p.split()[0]) for p in text.split(" lds=")[1:]]


def inputs(row, n_rows=None):
    """X (N × F), W0 (N × k), H0 (k × F) in fp64, uniform in [0, 1), every value exactly
    representable in fp32 (bf16 for a bf16 X), seeded from the row."""
    dt, F, k, N, _ = row
    N = N if n_rows is None else n_rows
    rng = np.random.default_rng(zlib.crc32(row_id(row).encode()))
    X = rng.random((N, F), dtype=np.float32)
    if dt == "bfloat16":  # truncate to bf16's 8 significant bits
        X = (X.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    W0 = rng.random((N, k), dtype=np.float32)
    H0 = rng.random((k, F), dtype=np.float32)
    return X.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64)
