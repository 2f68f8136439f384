"""Capacity rule of sdbv_append_rows (host-only, no GPU): the capacity a
table of capacity n_pad gets when an append needs `need` rows."""
import surrealdb_amd
from surrealdb_amd import append_capacity

ALIGN = 4096  # lcm of the scan tile (1024) and the shadow tiles (2048, 4096)


def test_fits_keeps_the_capacity():
    for n_pad in (0, 1024, 3072, 4096, 10_000_384):
        for need in {0, min(1, n_pad), n_pad // 2, n_pad}:
            assert append_capacity(n_pad, need) == n_pad


def test_growth_is_aligned_sufficient_and_geometric():
    for n_pad in (0, 1024, 3072, 4096, 12288, 1_000_448, 10_000_384):
        for extra in (1, 63, 64, 65, 4095, 4096, 4097, n_pad, 3 * n_pad + 5):
            need = n_pad + extra
            cap = append_capacity(n_pad, need)
            assert cap % ALIGN == 0
            assert cap >= need
            assert cap >= n_pad + n_pad // 2
            # and no more than the rule asks for
            assert cap < max(need, n_pad + n_pad // 2) + ALIGN


def test_the_issue_examples():
    assert append_capacity(1024, 1025) == 4096
    assert append_capacity(3072, 10000) == 12288
    assert append_capacity(4096, 4097) == 8192
    assert append_capacity(8192, 8193) == 12288


def test_one_row_at_a_time_regrows_log_n_times():
    """From 1024 to a million rows one row at a time: each growth multiplies
    the capacity by at least 1.5, so there are at most
    log(1e6 / 4096) / log(1.5) + 2 < 16 of them."""
    cap, grows = 1024, 0
    for n in range(1025, 1_000_001):
        new = append_capacity(cap, n)
        if new != cap:
            assert new >= n and new >= cap + cap // 2
            cap = new
            grows += 1
    assert cap >= 1_000_000
    assert grows <= 16
    print(f"{grows} regrowths, final capacity {cap}")


def test_python_surface_exists():
    for name in ("append_rows", "table_reserve", "table_capacity"):
        assert callable(getattr(surrealdb_amd.Context, name))
    fields = [f for f, _ in surrealdb_amd._Stats._fields_]
    assert fields[-3:] == ["last_append_ms", "last_append_kernel_ms",
                           "last_append_realloc"]
