"""Cases of the device-wide primitives (csrc/prims.hip), shared by the CPU twin (host-emulation loops of tests/host_emu/emu_parts.cpp, which
check this file's own logic) and the GPU run (wave-64 shuffles, LDS, atomics) of tests/test_gpu_prims.py.  Every case compares with a plain
high-precision reference: numpy.cumsum in int64, math.fsum, numpy max, and float64 numpy for the re-neighbouring criterion."""
import math

import numpy as np

# ---- exclusive scan: one wave (64), one block of the tile-sum scan (256 tiles), one tile (2048 items), the carry loop of k_scan_tiles (256 x 2048) ----
SCAN_N = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 524287, 524288, 524289, 1300001]
SCAN_KINDS = ["random", "zeros", "ones", "last"]
REGROW = (5, 2_300_000)              # the scratch of a first scan holds 2 x tiles + 1024 = 1026 tiles = 2 101 248 items: the second scan re-allocates it


def scan_input(kind, n, seed=0):
    if kind == "random":
        return np.random.default_rng(1000 + n + seed).integers(0, 201, size=n).astype(np.int32)
    if kind == "zeros":
        return np.zeros(n, dtype=np.int32)
    if kind == "ones":
        return np.ones(n, dtype=np.int32)
    v = np.zeros(n, dtype=np.int32)
    if n:
        v[-1] = 12345
    return v


def check_scan(lib, v, warm_n=0):
    ref = np.concatenate([[0], np.cumsum(v.astype(np.int64))])
    assert ref[-1] <= 2 ** 31 - 1
    out = lib.debug_scan_i32(v, warm_n)
    bad = np.flatnonzero(out.astype(np.int64) != ref)
    assert bad.size == 0, f"n = {len(v)}: first wrong prefix at {bad[0]}: {out[bad[0]]} != {ref[bad[0]]} ({bad.size} wrong)"


def scan_int32_max_input():
    """524 289 items (the carry loop) whose total is exactly 2^31 - 1"""
    n = 524289
    q, r = divmod(2 ** 31 - 1, n)
    v = np.full(n, q, dtype=np.int32)
    v[np.random.default_rng(5).permutation(n)[:r]] += 1
    assert int(v.astype(np.int64).sum()) == 2 ** 31 - 1
    return v


# ---- column sums: one block (256 rows), the 512-block cap of stage 1 (131 072 rows), the grid-stride loop behind it ----
COLSUM_NROW = [0, 1, 255, 256, 257, 131071, 131072, 131073, 300000]
COLSUM_NCOL = [1, 7, 8]
_colsum = {}


def colsum_case(nrow, ncol):
    """(input, math.fsum per column, bar per column): entries of magnitude [0.5, 1.5] with random sign, so that one dropped or doubled row moves a sum
    by at least 0.5.  Bar: nrow additions in any order, each rounding its partial sum (at most sum|x|) to 2^-53 relative."""
    if (nrow, ncol) not in _colsum:
        rng = np.random.default_rng(77 * nrow + ncol)
        a = rng.uniform(0.5, 1.5, size=(nrow, ncol)) * rng.choice([-1.0, 1.0], size=(nrow, ncol))
        ref = np.array([math.fsum(a[:, c].tolist()) for c in range(ncol)])
        bar = nrow * 2.0 ** -53 * np.abs(a).sum(axis=0)
        _colsum[(nrow, ncol)] = (a, ref, bar)
    return _colsum[(nrow, ncol)]


def check_colsum(lib, nrow, ncol):
    a, ref, bar = colsum_case(nrow, ncol)
    out = lib.debug_sum_columns_f64(a.reshape(-1), ncol)
    if nrow == 0:
        assert np.all(out == 0.0), out
    err = np.abs(out - ref)
    assert np.all(err <= bar), (nrow, ncol, err, bar)


# ---- max: one wave, two blocks, the 1024-block grid-stride cap (262 144 items) ----
MAX_N = [0, 1, 64, 257, 262144, 262145, 400000]


def check_max(lib, n):
    rng = np.random.default_rng(31 + n)
    base = rng.integers(-1000, 1001, size=n).astype(np.int32)
    if n == 0:
        assert lib.debug_max_i32(base) == 0
        return
    for at in sorted({0, n - 1, int(rng.integers(0, n))}):
        v = base.copy()
        v[at] = 5000 + at % 7
        assert lib.debug_max_i32(v) == int(v.max()) == 5000 + at % 7, (n, at)
    assert lib.debug_max_i32(-1 - np.abs(base)) == 0, "the result is max(0, max(in))"


# ---- re-neighbouring flag ----
FLAG_N = [0, 1, 256, 257, 262145]           # 262 145: index 262 144 is the first item of the grid-stride loop behind the 1024-block cap
FLAG_DT = 0.002


def flag_case(n):
    """(x, xhold, v, reach): the largest displacement and the largest speed on different atoms, one of them the last atom; float64 reference
    reach = max|x - xhold| + 2 dt max|v|"""
    rng = np.random.default_rng(900 + n)
    x = rng.uniform(0.0, 30.0, size=(n, 3))
    xh = x - rng.uniform(-0.02, 0.02, size=(n, 3))
    v = rng.uniform(-1.0, 1.0, size=(n, 3))
    if n:
        last = n - 1
        other = int(rng.integers(0, max(n - 1, 1)))
        big_d, big_v = (last, other) if n % 2 else (other, last)      # n = 1: both on the only atom
        xh[big_d] = x[big_d] - np.array([0.21, -0.17, 0.13])
        v[big_v] = np.array([-3.1, 6.7, 2.9])
    d = np.sqrt(((x - xh) ** 2).sum(axis=1)).max() if n else 0.0
    s = np.sqrt((v ** 2).sum(axis=1)).max() if n else 0.0
    return x, xh, v, float(d + 2.0 * FLAG_DT * s)


FLAG_THRESHOLDS = [1.0 - 1e-3, 1.0 + 1e-3, 1.0 - 1e-9, 1.0 + 1e-9]


def check_flag_value(flag, reach, half_skin, what):
    """never a miss; a false alarm only inside the kernel's rounding band (squared lengths x 1.000001f: at most 5e-7 on a length, plus float32 rounding)"""
    assert flag in (0, 1), flag
    if reach > half_skin:
        assert flag == 1, f"{what}: missed: reach {reach!r} > half_skin {half_skin!r}"
    if not reach * (1.0 + 1e-6) > half_skin:
        assert flag == 0, f"{what}: flagged outside the rounding band: reach {reach!r}, half_skin {half_skin!r}"
