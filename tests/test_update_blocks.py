"""sdbv_update_blocks (host-only): the distinct 256-row blocks that hold a
strictly increasing list of row positions, the block list sdbv_update_rows
uploads for the shadow builders. Held against np.unique(row_idx // 256)."""
import ctypes

import numpy as np
import pytest

U32P = ctypes.POINTER(ctypes.c_uint32)


def raw(row_idx, cap):
    """(return value, the first min(count, cap) blocks written)."""
    import surrealdb_amd
    row_idx = np.ascontiguousarray(row_idx, dtype=np.uint32)
    out = np.full(cap, 0xDEADBEEF, dtype=np.uint32)
    count = surrealdb_amd.lib().sdbv_update_blocks(
        row_idx.ctypes.data_as(U32P), row_idx.size,
        out.ctypes.data_as(U32P) if cap else None, cap)
    return int(count), out


CASES = {
    "one_row": [77],
    "row_0": [0],
    "rows_255_256": [255, 256],
    "rows_256_257": [256, 257],
    "whole_block": list(range(512, 768)),
    "whole_block_and_neighbours": list(range(511, 769)),
    "shared_and_distinct": [5, 300, 301, 1000],
    "all_of_1003": list(range(1003)),
    "near_2_32": [2 ** 32 - 513, 2 ** 32 - 257, 2 ** 32 - 256, 2 ** 32 - 2,
                  2 ** 32 - 1],
    "scattered": sorted(np.random.default_rng(3).choice(
        10_000_000, 4096, replace=False).tolist()),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_blocks_equal_unique(name):
    from surrealdb_amd import update_blocks
    row_idx = np.array(CASES[name], dtype=np.uint32)
    want = np.unique(row_idx // 256).astype(np.uint32)
    got = update_blocks(row_idx)
    assert got.dtype == np.uint32
    assert np.array_equal(got, want)
    count, out = raw(row_idx, want.size)
    assert count == want.size
    assert np.array_equal(out, want)


def test_empty_list():
    from surrealdb_amd import update_blocks
    assert update_blocks(np.empty(0, np.uint32)).size == 0
    assert raw(np.empty(0, np.uint32), 0)[0] == 0
    count, out = raw(np.empty(0, np.uint32), 4)
    assert count == 0 and np.all(out == 0xDEADBEEF)


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_cap_below_the_count_still_returns_the_count(cap):
    row_idx = np.array([5, 300, 301, 1000, 5000, 2 ** 32 - 1], np.uint32)
    want = np.unique(row_idx // 256).astype(np.uint32)
    assert want.size == 5
    count, out = raw(row_idx, cap)
    assert count == want.size
    assert np.array_equal(out, want[:cap])
    # and nothing is written past cap
    big = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    import surrealdb_amd
    surrealdb_amd.lib().sdbv_update_blocks(
        row_idx.ctypes.data_as(U32P), row_idx.size, big.ctypes.data_as(U32P),
        cap)
    assert np.all(big[cap:] == 0xDEADBEEF)


def test_stats_fields_follow_the_append_fields():
    """The three new fields sit at the end of sdbv_stats, behind the layout
    every earlier caller compiled against."""
    import surrealdb_amd
    full, old = surrealdb_amd._StatsUpdate, surrealdb_amd._Stats
    assert [f for f, _ in full._fields_] == [
        "last_update_ms", "last_update_kernel_ms", "last_update_blocks"]
    assert issubclass(full, old)
    assert full.last_update_ms.offset == ctypes.sizeof(old)
    assert full.last_update_kernel_ms.offset == ctypes.sizeof(old) + 8
    assert full.last_update_blocks.offset == ctypes.sizeof(old) + 16
    assert ctypes.sizeof(full) == ctypes.sizeof(old) + 24
    assert callable(surrealdb_amd.Context.update_rows)
