"""CPU checks of the filtered scan's host-side bitmap walk (sdbv_filter_rows,
the routine sdbv_knn_bruteforce_filtered counts rows and builds its row list
with) against numpy. No device call."""
import numpy as np
import pytest

import surrealdb_amd

NS = [1, 63, 64, 65, 999, 4096]
DENSITIES = [0.0, 0.01, 0.5, 1.0]


def make_allow(n, p, seed=0):
    rng = np.random.default_rng(1000 * n + int(p * 100) + seed)
    if p <= 0.0:
        return np.zeros(n, dtype=bool)
    if p >= 1.0:
        return np.ones(n, dtype=bool)
    return rng.random(n) < p


def pack(allow):
    """Reference packing: row r -> bit r & 63 of word r >> 6."""
    n = allow.size
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    for r in np.flatnonzero(allow):
        words[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return words


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", DENSITIES)
def test_filter_rows_matches_numpy(n, p):
    allow = make_allow(n, p)
    want = np.flatnonzero(allow).astype(np.uint32)
    count, rows = surrealdb_amd.filter_rows(allow, n)
    assert count == want.size
    assert rows.dtype == np.uint32
    assert np.array_equal(rows, want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", DENSITIES)
def test_bool_and_word_input_agree(n, p):
    allow = make_allow(n, p, seed=1)
    words = pack(allow)
    cb, rb = surrealdb_amd.filter_rows(allow, n)
    cw, rw = surrealdb_amd.filter_rows(words, n)
    assert cb == cw == int(allow.sum())
    assert np.array_equal(rb, rw)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", DENSITIES)
def test_tail_bits_ignored(n, p):
    """Every bit at or past n set in the last word: neither the count nor
    the rows may see them."""
    allow = make_allow(n, p, seed=2)
    words = pack(allow)
    if n & 63:
        words[-1] |= ~((np.uint64(1) << np.uint64(n & 63)) - np.uint64(1))
    want = np.flatnonzero(allow).astype(np.uint32)
    count, rows = surrealdb_amd.filter_rows(words, n)
    assert count == want.size
    assert np.array_equal(rows, want)
    assert rows.size == 0 or int(rows.max()) < n


def test_last_word_all_ones():
    n = 999
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    count, rows = surrealdb_amd.filter_rows(words, n)
    assert count == n - 960
    assert np.array_equal(rows, np.arange(960, n, dtype=np.uint32))


@pytest.mark.parametrize("n", [65, 999, 4096])
@pytest.mark.parametrize("p", [0.5, 1.0])
def test_cap_below_count(n, p):
    allow = make_allow(n, p, seed=3)
    want = np.flatnonzero(allow).astype(np.uint32)
    for cap in (0, 1, 7, want.size - 1):
        count, rows = surrealdb_amd.filter_rows(allow, n, cap=cap)
        assert count == want.size  # the full count, whatever the cap
        assert np.array_equal(rows, want[:cap])


def test_cap_is_a_hard_limit_on_writes():
    """Only the first cap entries of the output buffer are written."""
    import ctypes
    n = 4096
    words = pack(np.ones(n, dtype=bool))
    out = np.full(64, 0xDEADBEEF, dtype=np.uint32)
    cap = 10
    count = surrealdb_amd.lib().sdbv_filter_rows(
        words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), words.size, n,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap)
    assert count == n
    assert np.array_equal(out[:cap], np.arange(cap, dtype=np.uint32))
    assert np.all(out[cap:] == 0xDEADBEEF)


def test_wrong_length_rejected():
    with pytest.raises(surrealdb_amd.SdbvError):
        surrealdb_amd.filter_rows(np.ones(10, dtype=bool), 11)
    with pytest.raises(surrealdb_amd.SdbvError):
        surrealdb_amd.filter_rows(np.zeros(3, dtype=np.uint64), 64)
