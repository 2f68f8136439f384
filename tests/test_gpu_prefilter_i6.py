"""Single-query prefilter, int6 tier (6-bit shadow, integer dot products
against a 12-bit query, per-row bound + exact rescore) — GPU parity.

Every case runs knn_bruteforce with the table's int6 shadow ON and compares
ids and distance BITS with the same call with no shadow
(sdbv_table_set_prefilter_i6 / sdbv_table_set_prefilter_kind) and with the
CPU oracle, and asserts which
path ran (stats last_scan_path: 0 exact scan, 5 int6 prefilter, 6 int6
prefilter overflowed then exact scan). Shapes are the smallest at which each
mechanism can fail: the int6 prefilter gives one row to each lane per sweep
(256 rows), collects 8 sweeps (T = 2048 rows, the block tile) for one block
select, and a block takes one tile unless the table has more tiles than the
device holds blocks."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_TILE = 2048
PF8_TILE = 4096
PF6_TILE = 2048
PF_CAND_CAP = 16384


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def set_kind(ctx, table, kind):
    """Shadow kind 0 none, 1 bf16, 2 int8 through table_set_prefilter_kind;
    3 = int6 has an entry of its own."""
    if kind == 3:
        ctx.table_set_prefilter_i6(table)
    else:
        ctx.table_set_prefilter_kind(table, kind)


def run_on_off(ctx, table, q, k):
    """(ids, dists, path, candidates) with the int6 shadow, then (ids,
    dists) with no shadow."""
    set_kind(ctx, table, 3)
    on = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    on = (on[0].copy(), on[1].copy(), st["last_scan_path"],
          st["last_prefilter_candidates"])
    ctx.table_set_prefilter_kind(table, 0)
    off = ctx.knn_bruteforce(table, q, k)
    assert ctx.stats()["last_scan_path"] == 0
    return on, off


def assert_same(on, off):
    assert np.array_equal(on[0], off[0]), "ids differ from the shadow-off path"
    assert np.array_equal(bits(on[1]), bits(off[1])), \
        "distance bits differ from the shadow-off path"


def assert_oracle(on, corpus, q, k, ids=None):
    oids, odists = oracle.topk_f32("cosine", corpus, q, k)
    if ids is not None:
        oids = ids[oids.astype(np.int64)]
    assert np.array_equal(on[0], oids), "ids differ from the oracle"
    assert np.array_equal(bits(on[1]), bits(odists)), \
        "distance bits differ from the oracle"


@pytest.mark.parametrize("n,d,k", [
    (5, 16, 10),              # n < k: threshold +inf; d < 32
    (999, 128, 10),           # partial tile: a partial sweep, then none
    (PF6_TILE + 1, 20, 64),   # one row past the tile; features padded 20->32
    (PF6_TILE + 1, 36, 10),   # two groups, the second one 4 of 32 features
    (50_000, 768, 10),        # many blocks; both merge levels; 24 groups
])
def test_i6_matches_exact_and_oracle(ctx, n, d, k):
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    ctx.stage_corpus(61, corpus, metric="cosine")
    on, off = run_on_off(ctx, 61, q, k)
    print(f"n={n} d={d} k={k}: candidates {on[3]}")
    assert on[2] == 5
    assert min(k, n) <= on[3] <= PF_CAND_CAP
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(61)


def test_i6_explicit_ids(ctx):
    n, d, k = 3000, 32, 5
    corpus = oracle.gen_f32(0x88, 0, n, d)
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    q = oracle.gen_f32(0x99, 0, 1, d)[0]
    ctx.stage_corpus(62, corpus, ids=ids, metric="cosine")
    on, off = run_on_off(ctx, 62, q, k)
    assert on[2] == 5
    assert_same(on, off)
    assert_oracle(on, corpus, q, k, ids=ids)
    ctx.drop_table(62)


def test_i6_duplicates_tie_order(ctx):
    """Exact duplicates of the best row in neighbouring lanes, across a
    wave boundary (64 rows), a sweep boundary (256 rows), the select-feed
    boundary, which is the block boundary at this size (2048 rows), and in
    further blocks: ties come out in ascending id order."""
    n, d, k = 9000, 64, 12
    corpus = oracle.gen_f32(0x77, 0, n, d)
    dup_rows = [7, 8, 63, 64, 255, 256, 2047, 2048, 4100, 8999]
    for r in dup_rows:
        corpus[r] = corpus[7]
    q = corpus[7].copy()
    ctx.stage_corpus(63, corpus, metric="cosine")
    on, off = run_on_off(ctx, 63, q, k)
    assert on[2] == 5
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    assert list(on[0][:10]) == dup_rows
    assert np.all(bits(on[1][:10]) == bits(on[1][:1]))
    ctx.drop_table(63)


def test_i6_two_tiles_per_block_tie_order(ctx):
    """More tiles than the device holds blocks (at most 8 per CU, 256 CUs),
    so a block sweeps two tiles and carries its Kth upper bound from one
    select feed to the next: duplicates on both sides of a feed boundary
    inside a block (2047 | 2048) and of the block boundary (4095 | 4096),
    and in the last, partial tile."""
    n, d, k = 2048 * PF6_TILE + 1500, 8, 8
    corpus = oracle.gen_f32(0x78, 0, n, d)
    dup_rows = [2047, 2048, 4095, 4096, n - 1]
    for r in dup_rows:
        corpus[r] = corpus[2047]
    q = corpus[2047].copy()
    ctx.stage_corpus(64, corpus, metric="cosine")
    on, off = run_on_off(ctx, 64, q, k)
    print(f"two tiles per block: candidates {on[3]}")
    assert on[2] == 5
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    assert list(on[0][:5]) == dup_rows
    ctx.drop_table(64)


def unsafe_corpus(n, d):
    corpus = oracle.gen_f32(0x61, 0, n, d)
    corpus[3] = 0.0                      # zero norm
    corpus[9, 2] = np.nan
    corpus[10, 0] = np.inf
    corpus[11, 5] = -np.inf
    corpus[12, 1] = 3e38                 # finite, the norm overflows
    corpus[13] = 1e-40                   # all subnormal: the norm underflows
    corpus[14, 4] = 1e-40                # one subnormal element: a safe row
    corpus[15] = -corpus[15]
    corpus[16] = 2.5                     # constant row: every code is 31
    corpus[17] = 1e-3                    # one dominant element: the other
    corpus[17, 6] = -50.0                # codes are 0
    corpus[n - 1, d - 1] = np.nan
    return corpus


@pytest.mark.parametrize("n,k", [(3000, 10), (40, 64)])
def test_i6_unsafe_rows(ctx, n, k):
    """Rows the bound cannot cover always reach the exact stage: results,
    NaN and infinite distances included, equal the shadow-off path's."""
    d = 32
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x62, 0, 1, d)[0]
    ctx.stage_corpus(65, corpus, metric="cosine")
    on, off = run_on_off(ctx, 65, q, k)
    assert on[2] == 5
    assert_same(on, off)
    # the constant and the dominant-element row as the best rows (and as
    # queries: one with a single 12-bit code, one with a large residual)
    for r in (16, 17):
        on, off = run_on_off(ctx, 65, corpus[r].copy(), k)
        assert on[2] == 5
        assert_same(on, off)
    ctx.drop_table(65)


@pytest.mark.parametrize("kind", ["zero", "nan", "huge", "tiny"])
def test_i6_unsafe_query_takes_exact_scan(ctx, kind):
    n, d, k = 3000, 32, 10
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x63, 0, 1, d)[0]
    if kind == "zero":
        q[:] = 0.0
    elif kind == "nan":
        q[7] = np.nan
    elif kind == "huge":
        q[0] = 3e38
    else:
        q[:] = 1e-30
    ctx.stage_corpus(66, corpus, metric="cosine")
    on, off = run_on_off(ctx, 66, q, k)
    assert on[2] == 0
    assert on[3] == 0
    assert_same(on, off)
    ctx.drop_table(66)


def test_i6_candidate_overflow_falls_back(ctx):
    """The int8 test's construction: rows equal to one vector times
    (1 + 1e-4 u), u in [-1, 1), far below the 6-bit step. Checked first on
    the CPU with the numpy restatement of the bounds: more than 16384 rows
    have a lower bound at or under the Kth smallest upper bound."""
    from test_prefilter_i6_bound import bounds
    n, d, k = PF_CAND_CAP + 3616, 16, 10
    base = oracle.gen_f32(0x51, 0, 1, d)[0]
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, size=(n, d))
    corpus = (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)
    q = oracle.gen_f32(0x53, 0, 1, d)[0]
    _, lo, up, _, _, _ = bounds(q, corpus, check_quantisers=False)
    passing = int(np.sum(lo <= np.sort(up)[k - 1]))
    print(f"overflow construction: {passing} of {n} rows pass on the CPU")
    assert passing > PF_CAND_CAP
    ctx.stage_corpus(67, corpus, metric="cosine")
    on, off = run_on_off(ctx, 67, q, k)
    assert on[2] == 6
    assert on[3] == passing  # the counter keeps counting past the capacity
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(67)


def base_bytes(n, d):
    n_pad = -(-n // 1024) * 1024
    return d * n_pad * 4 + n_pad * (8 + 8 + 4)  # cm, norms, ids, aux


def bf16_bytes(n, d):
    sn_pad = -(-n // PF_TILE) * PF_TILE
    return d * sn_pad * 2 + sn_pad * 4


def i8_bytes(n, d):
    sn_pad = -(-n // PF8_TILE) * PF8_TILE
    return d * sn_pad + 8 * sn_pad


def i6_bytes(n, d):
    sn_pad = -(-n // PF6_TILE) * PF6_TILE
    d_pad = -(-d // 32) * 32
    return sn_pad * (d_pad * 3 // 4 + 12)  # H, L; pscale, peps, xsum


def test_i6_switching_kinds_accounts_bytes(ctx):
    n, d = 5000, 36
    corpus = oracle.gen_f32(0x71, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    ctx.stage_corpus(68, corpus, metric="cosine")
    want = {0: 0, 1: bf16_bytes(n, d), 2: i8_bytes(n, d), 3: i6_bytes(n, d)}
    path = {0: 0, 1: 1, 2: 3, 3: 5}

    def check(kind):
        assert ctx.stats()["bytes_staged"] - before == \
            base_bytes(n, d) + want[kind]
        ctx.knn_bruteforce(68, corpus[0], 5)
        assert ctx.stats()["last_scan_path"] == path[kind]

    check(0)
    for kind in (3, 3, 2, 3, 1, 3, 0, 3, 2, 1, 0):  # every ordered pair
        set_kind(ctx, 68, kind)
        check(kind)
    set_kind(ctx, 68, 3)
    ctx.table_set_prefilter(68, True)    # the bf16 switch replaces int6
    check(1)
    set_kind(ctx, 68, 3)
    ctx.table_set_prefilter(68, False)   # off frees whichever shadow
    check(0)
    import surrealdb_amd
    set_kind(ctx, 68, 3)
    for bad in (3, 4, -1):  # the kind entry keeps its three kinds
        with pytest.raises(surrealdb_amd.SdbvError):
            ctx.table_set_prefilter_kind(68, bad)
        check(3)            # and a rejected call changes nothing
    ctx.stage_corpus(68, corpus, metric="euclidean")  # cosine only
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.table_set_prefilter_i6(68)
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.table_set_prefilter_i6(6868)  # no such table
    ctx.drop_table(68)


def test_i6_policy_env(ctx, monkeypatch):
    n, d = 3000, 32
    corpus = oracle.gen_f32(0x72, 0, n, d)
    before = ctx.stats()["bytes_staged"]

    def staged():
        return ctx.stats()["bytes_staged"] - before

    def path():
        ctx.knn_bruteforce(69, corpus[0], 5)
        return ctx.stats()["last_scan_path"]

    # the int6 threshold alone builds nothing: no shadow below the first one
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I6_MIN_ROWS", "1000")
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) and path() == 0
    monkeypatch.delenv("SDBV_SCAN_PREFILTER_I6_MIN_ROWS")
    # 3000 rows with the first two thresholds lowered still get int8 ...
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_MIN_ROWS", "1000")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8_MIN_ROWS", "1000")
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    # ... until the int6 threshold is lowered too
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I6_MIN_ROWS", "3000")
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + i6_bytes(n, d) and path() == 5
    ctx.stage_synthetic(69, n, d, metric="cosine")
    assert staged() == base_bytes(n, d) + i6_bytes(n, d)
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I6_MIN_ROWS", "3001")
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I6_MIN_ROWS", "1000")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I6", "0")  # opt out: int8
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    monkeypatch.delenv("SDBV_SCAN_PREFILTER_I6")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8", "0")  # int8 off: bf16
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + bf16_bytes(n, d) and path() == 1
    monkeypatch.delenv("SDBV_SCAN_PREFILTER_I8")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER", "0")  # no shadow of any kind
    ctx.stage_corpus(69, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) and path() == 0
    ctx.drop_table(69)
