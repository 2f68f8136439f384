"""CPU checks of sdbv_select_topk, the host twin of the device select of the
all-distances route: the same digit walk (one shared per-pass step) on host
histograms. The reference is numpy: the f64 bits mapped to the total-order
key, restricted to the allowed rows, rows[np.lexsort((rows, keys))][:k].
Every comparison is exact equality. No device call."""
import numpy as np
import pytest

import surrealdb_amd


def total_key(d):
    """f64 -> u64, monotone in the total order (-NaN, -inf, ..., -0, +0,
    ..., +inf, +NaN): negative values flip every bit, the rest set the top
    bit."""
    bits = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(1 << 63))


def reference(d, k, allow=None):
    rows = np.arange(d.size, dtype=np.uint32)
    if allow is not None:
        rows = rows[allow[:d.size]]
    keys = total_key(d)[rows]
    return rows[np.lexsort((rows, keys))][:k]


def pack(allow, nwords=None):
    n = allow.size
    words = np.zeros((n + 63) // 64 if nwords is None else nwords,
                     dtype=np.uint64)
    for r in np.flatnonzero(allow):
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


def check(d, k, allow=None, allow_arg=None):
    want = reference(d, k, allow)
    arg = allow if allow_arg is None else allow_arg
    got = surrealdb_amd.select_topk(d, k, arg)
    assert got.dtype == np.uint32
    assert got.size == want.size, (got.size, want.size)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 70001])
def test_random(n):
    d = np.random.default_rng(n).standard_normal(n) * 1e3
    for k in sorted({1, n - 1, n, n + 5, 64, 65, 1000}):
        if k >= 1:
            check(d, k)


@pytest.mark.parametrize("n", [257, 1000, 70001])
@pytest.mark.parametrize("p", [0.5, 0.02])
def test_random_under_a_bitmap(n, p):
    rng = np.random.default_rng(7 * n + int(p * 100))
    d = rng.standard_normal(n)
    allow = rng.random(n) < p
    for k in (1, 10, 65, 1000, n):
        check(d, k, allow)
        check(d, k, allow, allow_arg=pack(allow))


@pytest.mark.parametrize("k", [300, 65536])
def test_all_equal_rows_decide(k):
    """70001 equal distances: the key digits choose nothing, the row digits
    above bit 16 decide."""
    n = 70001
    d = np.full(n, 3.0)
    got = check(d, k)
    assert np.array_equal(got, np.arange(k, dtype=np.uint32))


@pytest.mark.parametrize("k", [300, 65536])
def test_all_equal_first_66000_disallowed(k):
    n = 70001
    d = np.full(n, 3.0)
    allow = np.ones(n, bool)
    allow[:66000] = False
    got = check(d, k, allow)
    m = min(k, n - 66000)
    assert np.array_equal(got, np.arange(66000, 66000 + m, dtype=np.uint32))


def test_lowest_byte_only():
    """Values that differ in the last key digit alone, with duplicates."""
    rng = np.random.default_rng(3)
    base = np.float64(1.5).view(np.uint64)
    bits = (base & ~np.uint64(255)) | rng.integers(0, 256, 5000).astype(
        np.uint64)
    d = bits.view(np.float64)
    for k in (1, 17, 64, 65, 1000, 4999, 5000):
        check(d, k)
    check(-d, 100)  # the other branch of the key


def test_special_values():
    nan = np.uint64(0x7FF8000000000001).view(np.float64)
    neg_nan = np.uint64(0xFFF8000000000001).view(np.float64)
    nan2 = np.uint64(0x7FF0000000000001).view(np.float64)
    sub = np.float64(5e-324)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, nan, neg_nan, nan2, sub,
                     -sub, 1e-310, -1e-310, -1.0, 1.0, -1e300, 1e300, 2.5,
                     -2.5], dtype=np.float64)
    rng = np.random.default_rng(4)
    d = vals[rng.integers(0, vals.size, 3000)]
    for k in (1, 5, 64, 65, 500, 2999, 3000, 3100):
        check(d, k)
    got = check(vals, vals.size)
    # the documented sequence: -NaN, -inf, ..., -0, +0, ..., +inf, +NaNs
    assert got[0] == 5 and got[1] == 3
    assert list(got[-3:]) == [2, 6, 4]
    z = list(got)
    assert z.index(1) + 1 == z.index(0)  # -0 directly before +0


def test_empty_bitmap():
    d = np.random.default_rng(5).standard_normal(1000)
    got = surrealdb_amd.select_topk(d, 10, np.zeros(1000, bool))
    assert got.size == 0
    got = surrealdb_amd.select_topk(d, 10, np.zeros(16, np.uint64))
    assert got.size == 0


def test_tail_bits_ignored():
    n = 999
    rng = np.random.default_rng(6)
    d = rng.standard_normal(n)
    allow = rng.random(n) < 0.3
    words = pack(allow)
    words[-1] |= ~((np.uint64(1) << np.uint64(n & 63)) - np.uint64(1))
    for k in (1, 10, 400, 999, 1100):
        check(d, k, allow, allow_arg=words)
    full = np.full(16, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    got = check(d, 2000, np.ones(n, bool), allow_arg=full)
    assert got.size == n and int(got.max()) == n - 1


def test_fewer_allowed_rows_than_k():
    n = 3000
    d = np.random.default_rng(8).standard_normal(n)
    allow = np.zeros(n, bool)
    allow[[3, 1500, 2999]] = True
    got = check(d, 10, allow)
    assert got.size == 3


def test_bad_arguments():
    import ctypes
    L = surrealdb_amd.lib()
    d = np.zeros(4)
    out = np.zeros(4, np.uint32)
    out_n = ctypes.c_uint32(7)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    BAD_ARG = -3
    assert L.sdbv_select_topk(dp, 4, None, 2, op, None) == BAD_ARG
    assert L.sdbv_select_topk(None, 4, None, 2, op,
                              ctypes.byref(out_n)) == BAD_ARG
    assert L.sdbv_select_topk(dp, 1 << 32, None, 2, op,
                              ctypes.byref(out_n)) == BAD_ARG
    assert L.sdbv_select_topk(dp, 4, None, 2, None,
                              ctypes.byref(out_n)) == BAD_ARG
    assert L.sdbv_select_topk(dp, 4, None, 0, op, ctypes.byref(out_n)) == 0
    assert out_n.value == 0
    assert L.sdbv_select_topk(dp, 0, None, 3, op, ctypes.byref(out_n)) == 0
    assert out_n.value == 0
