"""Single-query prefilter, two-stage int6 path (plane H streamed alone, the
threshold from exact distances, survivors refined with plane L, then the
exact rescore) — GPU parity.

Every case runs knn_bruteforce on a table staged with the int6 shadow and its
H-only side data and compares ids and distance BITS with the same context's
exact scan (the same rows staged without a shadow, SDBV_SCAN_PREFILTER=0, as
table + 100) and with the CPU oracle, and asserts which path
ran (stats last_scan_path: 15 two-stage, 5 plain int6, 0 exact scan, 13 int6
under a filter). The four MIN_ROWS variables at 1 bring the path down to
tables of a few rows. Shapes: the stream gives one row to each lane per sweep
(256 rows), collects 8 sweeps (2048 rows) per select and gives a block a
span of whole sweeps; the first list is collected per block, 4096 rows a
round (256 lanes x 4 quads of scores), at most 512 blocks, and reserved in
the global list when more than 4096 rows wait or the block is done; the
refine kernel shares a row among 32 lanes, so d = 4 and 36 leave most of
them idle and d = 768 gives each lane one of its 24 groups."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_CAND_CAP = 16384
MIN_ROWS = ("SDBV_SCAN_PREFILTER_MIN_ROWS", "SDBV_SCAN_PREFILTER_I8_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_I6_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_H4_MIN_ROWS")
H4, LIST_MAX = "SDBV_SCAN_PREFILTER_H4", "SDBV_SCAN_PREFILTER_H4_LIST_MAX"


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    for name in MIN_ROWS:
        monkeypatch.setenv(name, "1")
    monkeypatch.delenv(H4, raising=False)
    monkeypatch.delenv(LIST_MAX, raising=False)


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run(ctx, table, q, k):
    """(ids, dists, path, candidates, stage1) of one call."""
    ids, dists = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    return (ids.copy(), dists.copy(), st["last_scan_path"],
            st["last_prefilter_candidates"], st["last_prefilter_stage1"])


def stage(ctx, table, corpus, ids=None):
    """Stage corpus as table under the forced policy (int6 shadow with the
    side data) and as table + 100 with no shadow."""
    ctx.stage_corpus(table, corpus, ids=ids, metric="cosine")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SDBV_SCAN_PREFILTER", "0")
        ctx.stage_corpus(table + 100, corpus, ids=ids, metric="cosine")


def drop(ctx, table):
    ctx.drop_table(table)
    ctx.drop_table(table + 100)


def run_exact(ctx, table, q, k):
    """The same call over the shadowless copy of the table."""
    off = run(ctx, table + 100, q, k)
    assert off[2] == 0 and off[3] == 0 and off[4] == 0
    return off


def assert_same(on, off):
    assert np.array_equal(on[0], off[0]), "ids differ from the exact scan"
    assert np.array_equal(bits(on[1]), bits(off[1])), \
        "distance bits differ from the exact scan"


def assert_oracle(on, corpus, q, k):
    oids, odists = oracle.topk_f32("cosine", corpus, q, k)
    assert np.array_equal(on[0], oids), "ids differ from the oracle"
    assert np.array_equal(bits(on[1]), bits(odists)), \
        "distance bits differ from the oracle"


def assert_two_stage(on, n, k):
    assert on[2] == 15
    assert min(k, n) <= on[3] <= on[4] <= n


@pytest.mark.parametrize("d", [4, 36, 768])
@pytest.mark.parametrize("n", [1, 9, 2047, 2048, 2049, 4100, 8999])
def test_h4_matches_exact_and_oracle(ctx, n, d):
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    stage(ctx, 81, corpus)
    for k in (1, 10, 64):           # n < k: the threshold is +inf
        on = run(ctx, 81, q, k)
        print(f"n={n} d={d} k={k}: stage 1 {on[4]}, candidates {on[3]}")
        assert_two_stage(on, n, k)
        assert_oracle(on, corpus, q, k)
        assert_same(on, run_exact(ctx, 81, q, k))
    drop(ctx, 81)


def test_h4_explicit_ids(ctx):
    n, d, k = 3000, 32, 5
    corpus = oracle.gen_f32(0x88, 0, n, d)
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    q = oracle.gen_f32(0x99, 0, 1, d)[0]
    stage(ctx, 82, corpus, ids=ids)
    on = run(ctx, 82, q, k)
    assert_two_stage(on, n, k)
    assert_same(on, run_exact(ctx, 82, q, k))
    oids, odists = oracle.topk_f32("cosine", corpus, q, k)
    assert np.array_equal(on[0], ids[oids.astype(np.int64)])
    assert np.array_equal(bits(on[1]), bits(odists))
    drop(ctx, 82)


@pytest.mark.parametrize("k", [1, 6, 9, 12])
def test_h4_duplicates_tie_order(ctx, k):
    """Nine copies of the best row at sweep and tile edges: with k = 6 the
    ties straddle the Kth place, and every copy must survive both tests so
    that the six smallest ids come out, ascending, as in the exact scan."""
    n, d = 4100, 64
    corpus = oracle.gen_f32(0x77, 0, n, d)
    dup_rows = [7, 8, 63, 64, 255, 256, 2047, 2048, n - 1]
    for r in dup_rows:
        corpus[r] = corpus[7]
    q = corpus[7].copy()
    stage(ctx, 83, corpus)
    on = run(ctx, 83, q, k)
    assert_two_stage(on, n, k)
    assert on[3] >= len(dup_rows)   # the threshold is one of the copies'
    assert_same(on, run_exact(ctx, 83, q, k))
    assert_oracle(on, corpus, q, k)
    m = min(k, len(dup_rows))
    assert list(on[0][:m]) == dup_rows[:m]
    assert np.all(bits(on[1][:m]) == bits(on[1][:1]))
    drop(ctx, 83)


def unsafe_corpus(n, d):
    corpus = oracle.gen_f32(0x61, 0, n, d)
    corpus[3] = 0.0                      # zero norm
    corpus[9, 2] = np.nan
    corpus[10, 0] = np.inf
    corpus[11, 5] = -np.inf
    corpus[12, 1] = 3e38                 # finite, the norm overflows
    corpus[13] = 1e-40                   # all subnormal: the norm underflows
    corpus[16] = 2.5                     # constant row
    corpus[17] = 1e-3                    # one dominant element
    corpus[17, 6] = -50.0
    corpus[n - 1, d - 1] = np.nan
    return corpus


@pytest.mark.parametrize("n,k", [(3000, 10), (40, 64)])
def test_h4_uncovered_rows(ctx, n, k):
    """Rows the bound cannot cover pass both tests and reach the exact
    stage: with k = 64 > n every one of them is in the result, NaN and
    infinite distances included; with k = 10 of 3000 they are dropped by the
    final select alone. Queries: a plain one, and rows of the table itself,
    so that the best row is the query."""
    d = 32
    corpus = unsafe_corpus(n, d)
    stage(ctx, 84, corpus)
    for q in (oracle.gen_f32(0x62, 0, 1, d)[0], corpus[16].copy(),
              corpus[17].copy(), corpus[20].copy()):
        on = run(ctx, 84, q, k)
        assert on[2] == 15
        assert on[3] >= 7               # the seven uncovered rows at least
        assert on[3] <= on[4] <= n
        assert_same(on, run_exact(ctx, 84, q, k))
    assert 20 in on[0]                  # the row that is the query
    drop(ctx, 84)


def test_h4_first_list_overflow_falls_back_to_int6(ctx, monkeypatch):
    n, d, k = 4100, 36, 10
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    stage(ctx, 85, corpus)
    fits = run(ctx, 85, q, k)
    assert_two_stage(fits, n, k)
    monkeypatch.setenv(LIST_MAX, "4")
    on = run(ctx, 85, q, k)
    assert on[2] == 5                   # served by the plain int6 path
    assert on[4] == fits[4] > 4         # the raw count, past the capacity
    assert_same(on, fits)
    assert_oracle(on, corpus, q, k)
    monkeypatch.setenv(LIST_MAX, str(fits[4]))  # exactly full: no overflow
    on = run(ctx, 85, q, k)
    assert on[2] == 15 and on[3:] == fits[3:]
    assert_same(on, fits)
    drop(ctx, 85)


def test_h4_first_list_overflow_past_one_round_per_block(ctx):
    """More rows than 512 blocks take in two rounds (4 194 304), nearly all
    of them zero rows, which carry no bound and always pass: a block holds
    up to two rounds (8192 rows), so the blocks with a third round reserve
    list space in mid-loop, and every block far past the list's 262144
    entries, where nothing may be written. The call goes to the plain int6
    path, whose own list overflows too (path 6), and to the exact scan."""
    n, d, k = 4_300_000, 4, 10
    corpus = np.zeros((n, d), dtype=np.float32)
    keep = np.arange(0, n, 1000)
    corpus[keep] = oracle.gen_f32(0x5DB1, 0, keep.size, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    stage(ctx, 90, corpus)
    on = run(ctx, 90, q, k)
    assert on[2] == 6
    assert n - keep.size <= on[4] <= n and on[3] >= n - keep.size
    # zero rows have NaN distances, whose sign the CPU oracle and the device
    # give differently: the exact scan is the reference here, as for every
    # table with uncovered rows
    assert_same(on, run_exact(ctx, 90, q, k))
    drop(ctx, 90)


@pytest.mark.parametrize("kind", ["zero", "nan", "huge", "tiny"])
def test_h4_unsafe_query_takes_exact_scan(ctx, kind):
    n, d, k = 3000, 32, 10
    corpus = oracle.gen_f32(0x61, 0, n, d)
    q = oracle.gen_f32(0x63, 0, 1, d)[0]
    if kind == "zero":
        q[:] = 0.0
    elif kind == "nan":
        q[7] = np.nan
    elif kind == "huge":
        q[0] = 3e38
    else:
        q[:] = 1e-30
    stage(ctx, 86, corpus)
    on = run(ctx, 86, q, k)
    assert on[2] == 0 and on[3] == 0 and on[4] == 0
    assert_same(on, run_exact(ctx, 86, q, k))
    drop(ctx, 86)


def test_h4_toggles_per_call_on_one_staged_table(ctx, monkeypatch):
    n, d, k = 8999, 36, 10
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 2, 1, d)[0]
    stage(ctx, 87, corpus)
    first = run(ctx, 87, q, k)
    assert_two_stage(first, n, k)
    monkeypatch.setenv(H4, "0")
    plain = run(ctx, 87, q, k)
    assert plain[2] == 5 and plain[4] == 0
    monkeypatch.delenv(H4)
    again = run(ctx, 87, q, k)
    assert again[2:] == first[2:]
    assert_same(plain, first)
    assert_same(again, first)
    assert_oracle(first, corpus, q, k)
    print(f"candidates: two-stage {first[3]} of {first[4]}, plain {plain[3]}")
    # the row threshold is read at each call too
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_H4_MIN_ROWS", str(n + 1))
    assert run(ctx, 87, q, k)[2] == 5
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_H4_MIN_ROWS", str(n))
    assert run(ctx, 87, q, k)[2] == 15
    drop(ctx, 87)


def test_h4_filtered_call_keeps_its_path(ctx, monkeypatch):
    n, d, k = 4100, 36, 10
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 3, 1, d)[0]
    stage(ctx, 88, corpus)
    assert run(ctx, 88, q, k)[2] == 15
    monkeypatch.setenv("SDBV_FILTER_ROWLIST_MAX", "0")
    monkeypatch.setenv("SDBV_FILTER_PREFILTER_MIN_ROWS", "0")
    allow = np.ones(n, dtype=bool)
    allow[::3] = False
    ids, dists = ctx.knn_bruteforce_filtered(88, q, k, allow)
    st = ctx.stats()
    assert st["last_scan_path"] == 13 and st["last_prefilter_stage1"] == 0
    rows = np.flatnonzero(allow)
    oids, odists = oracle.topk_f32("cosine", corpus[rows], q, k)
    assert np.array_equal(ids, rows[oids.astype(np.int64)].astype(np.uint64))
    assert np.array_equal(bits(dists), bits(odists))
    assert run(ctx, 88, q, k)[2] == 15
    drop(ctx, 88)


def test_h4_side_data_is_staged_by_policy(ctx, monkeypatch):
    """The two side arrays (8 B per row) come with an int6 shadow that
    staging builds while the policy holds; the explicit entry builds the
    plain shadow, which serves the plain path."""
    n, d = 5000, 36
    sn_pad, d_pad = -(-n // 2048) * 2048, -(-d // 32) * 32
    plain = sn_pad * (d_pad * 3 // 4 + 12)
    corpus = oracle.gen_f32(0x71, 0, n, d)
    ctx.stage_corpus(89, corpus, metric="cosine")
    with_side = ctx.stats()["bytes_staged"]
    assert run(ctx, 89, corpus[0], 5)[2] == 15
    ctx.table_set_prefilter_kind(89, 0)
    base = ctx.stats()["bytes_staged"]
    assert with_side - base == plain + 8 * sn_pad
    ctx.table_set_prefilter_i6(89)
    assert ctx.stats()["bytes_staged"] - base == plain
    assert run(ctx, 89, corpus[0], 5)[2] == 5   # no side data: plain int6
    for name, value in ((H4, "0"),
                        ("SDBV_SCAN_PREFILTER_H4_MIN_ROWS", str(n + 1))):
        monkeypatch.setenv(name, value)
        ctx.stage_corpus(89, corpus, metric="cosine")
        assert ctx.stats()["bytes_staged"] - base == plain
        monkeypatch.setenv(name, "1")
        assert run(ctx, 89, corpus[0], 5)[2] == 5
    ctx.stage_corpus(89, corpus, metric="cosine")
    assert ctx.stats()["bytes_staged"] == with_side
    assert run(ctx, 89, corpus[0], 5)[2] == 15
    ctx.drop_table(89)
