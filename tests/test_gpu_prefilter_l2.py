"""Single-query prefilter, euclidean (l2) tier: int8 shadow + triangle-
inequality interval + exact rescore — GPU parity.

Every case runs knn_bruteforce with the table's l2 shadow ON and compares ids
and distance BITS with the same call with no shadow
(table_set_prefilter_l2) and with the CPU oracle, and asserts which path ran
(stats last_scan_path: 0 exact scan, 17 l2 prefilter, 18 l2 prefilter
overflowed then exact scan). Shapes are the smallest at which each mechanism
can fail: the stream sweeps 4096-row tiles, 16 rows per lane, fed to the
block select in two 2048-row halves, one tile per block at these sizes."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF8_TILE = 4096
PF_CAND_CAP = 16384
PATH_L2, PATH_L2_OVERFLOW = 17, 18


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run_on_off(ctx, table, q, k):
    """(ids, dists, path, candidates) with the l2 shadow, then (ids, dists)
    with no shadow."""
    ctx.table_set_prefilter_l2(table, True)
    on = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    on = (on[0].copy(), on[1].copy(), st["last_scan_path"],
          st["last_prefilter_candidates"])
    ctx.table_set_prefilter_l2(table, False)
    off = ctx.knn_bruteforce(table, q, k)
    assert ctx.stats()["last_scan_path"] == 0
    return on, off


def assert_same(on, off):
    assert np.array_equal(on[0], off[0]), "ids differ from the shadow-off path"
    assert np.array_equal(bits(on[1]), bits(off[1])), \
        "distance bits differ from the shadow-off path"


def assert_oracle(on, corpus, q, k, ids=None):
    oids, odists = oracle.topk_f32("euclidean", corpus, q, k)
    if ids is not None:
        oids = ids[oids.astype(np.int64)]
    assert np.array_equal(on[0], oids), "ids differ from the oracle"
    assert np.array_equal(bits(on[1]), bits(odists)), \
        "distance bits differ from the oracle"


@pytest.mark.parametrize("n,d,k", [
    (5, 16, 10),              # n < k: threshold +inf
    (999, 128, 10),           # partial tile, first select half only
    (PF8_TILE + 1, 20, 64),   # one row past the tile; d % 8 != 0: tail
    (50_000, 768, 10),        # many blocks; both merge levels
])
def test_l2_matches_exact_and_oracle(ctx, n, d, k):
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    ctx.stage_corpus(71, corpus, metric="euclidean")
    on, off = run_on_off(ctx, 71, q, k)
    print(f"n={n} d={d} k={k}: candidates {on[3]}")
    assert on[2] == PATH_L2
    assert min(k, n) <= on[3] <= PF_CAND_CAP
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(71)


def test_l2_explicit_ids(ctx):
    n, d, k = 3000, 32, 5
    corpus = oracle.gen_f32(0x88, 0, n, d)
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    q = oracle.gen_f32(0x99, 0, 1, d)[0]
    ctx.stage_corpus(72, corpus, ids=ids, metric="euclidean")
    on, off = run_on_off(ctx, 72, q, k)
    assert on[2] == PATH_L2
    assert_same(on, off)
    assert_oracle(on, corpus, q, k, ids=ids)
    ctx.drop_table(72)


def test_l2_duplicates_tie_order(ctx):
    """Exact duplicates of the best row in the same lane group, in other
    lane groups (16 rows), in the other select half (2048 rows) and in
    other blocks (4096 rows): ties come out in ascending id order."""
    n, d, k = 9000, 64, 8
    corpus = oracle.gen_f32(0x77, 0, n, d)
    dup_rows = [7, 8, 15, 16, 2100, 4100, 8999]
    for r in dup_rows:
        corpus[r] = corpus[7]
    q = corpus[7].copy()
    ctx.stage_corpus(73, corpus, metric="euclidean")
    on, off = run_on_off(ctx, 73, q, k)
    assert on[2] == PATH_L2
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    assert list(on[0][:7]) == dup_rows
    assert np.all(on[1][:7] == 0.0)
    ctx.drop_table(73)


def unsafe_corpus(n, d):
    """The unsafe-row corpus of test_gpu_prefilter_i8.py."""
    corpus = oracle.gen_f32(0x61, 0, n, d)
    corpus[3] = 0.0                      # zero row: covered on this tier
    corpus[9, 2] = np.nan
    corpus[10, 0] = np.inf
    corpus[11, 5] = -np.inf
    corpus[12, 1] = 3e38                 # finite, the norm leaves the window
    corpus[13] = 1e-40                   # all subnormal: squares underflow
    corpus[14, 4] = 1e-40                # one subnormal element
    corpus[15] = -corpus[15]
    corpus[16] = 2.5                     # constant row: every code is 127
    corpus[17] = 1e-3                    # one dominant element: the other
    corpus[17, 6] = -50.0                # codes are 0
    corpus[n - 1, d - 1] = np.nan
    return corpus


@pytest.mark.parametrize("n,k", [(3000, 10), (40, 64)])
def test_l2_unsafe_rows(ctx, n, k):
    """Rows the bound cannot cover always reach the exact stage: results,
    NaN and infinite distances included, equal the shadow-off path's."""
    d = 32
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x62, 0, 1, d)[0]
    ctx.stage_corpus(74, corpus, metric="euclidean")
    with np.errstate(all="ignore"):
        on, off = run_on_off(ctx, 74, q, k)
        assert on[2] == PATH_L2
        assert_same(on, off)
        if k > n:  # every row comes back, the uncovered ones included
            assert on[0].size == n and not np.isfinite(on[1]).all()
        # the zero, the subnormal, the constant and the dominant-element row
        # as the best rows, and the zero query (inside this tier's window)
        for qq in (corpus[3], corpus[13], corpus[16], corpus[17]):
            on, off = run_on_off(ctx, 74, qq.copy(), k)
            assert on[2] == PATH_L2
            assert_same(on, off)
    ctx.drop_table(74)


@pytest.mark.parametrize("kind", ["nan", "huge"])
def test_l2_unsafe_query_takes_exact_scan(ctx, kind):
    n, d, k = 3000, 32, 10
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x63, 0, 1, d)[0]
    if kind == "nan":
        q[7] = np.nan
    else:
        q[0] = 3e38
    ctx.stage_corpus(75, corpus, metric="euclidean")
    on, off = run_on_off(ctx, 75, q, k)
    assert on[2] == 0
    assert on[3] == 0
    assert_same(on, off)
    ctx.drop_table(75)


def test_l2_candidate_overflow_falls_back(ctx):
    """Rows equal to one vector times (1 + 1e-4 u), u in [-1, 1): far below
    the int8 step, so every row's interval holds every other row's distance
    and all rows are candidates."""
    n, d, k = 20000, 16, 10
    base = oracle.gen_f32(0x51, 0, 1, d)[0]
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, size=(n, d))
    corpus = (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)
    q = oracle.gen_f32(0x53, 0, 1, d)[0]
    ctx.stage_corpus(76, corpus, metric="euclidean")
    on, off = run_on_off(ctx, 76, q, k)
    assert on[2] == PATH_L2_OVERFLOW
    assert on[3] == n  # the counter keeps counting past the capacity
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(76)


def base_bytes(n, d):
    n_pad = -(-n // 1024) * 1024
    return d * n_pad * 4 + n_pad * (8 + 4)  # cm, ids, aux (no norms)


def l2_bytes(n, d):
    sn_pad = -(-n // PF8_TILE) * PF8_TILE
    return d * sn_pad + 12 * sn_pad


def test_l2_switching_accounts_bytes_and_entries_refuse(ctx):
    import surrealdb_amd
    n, d = 5000, 32
    corpus = oracle.gen_f32(0x71, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    ctx.stage_corpus(77, corpus, metric="euclidean")

    def staged():
        return ctx.stats()["bytes_staged"] - before

    def path():
        ctx.knn_bruteforce(77, corpus[0], 5)
        return ctx.stats()["last_scan_path"]

    assert staged() == base_bytes(n, d) and path() == 0
    ctx.table_set_prefilter_l2(77, True)
    assert staged() == base_bytes(n, d) + l2_bytes(n, d) and path() == PATH_L2
    ctx.table_set_prefilter_l2(77, True)   # already there: nothing changes
    assert staged() == base_bytes(n, d) + l2_bytes(n, d)
    # the three older entries keep refusing a euclidean table, shadow or not
    for call in (lambda: ctx.table_set_prefilter(77, True),
                 lambda: ctx.table_set_prefilter_kind(77, 2),
                 lambda: ctx.table_set_prefilter_i6(77)):
        with pytest.raises(surrealdb_amd.SdbvError):
            call()
    assert staged() == base_bytes(n, d) + l2_bytes(n, d) and path() == PATH_L2
    ctx.table_set_prefilter_l2(77, False)
    assert staged() == base_bytes(n, d) and path() == 0
    # the new entry refuses a cosine table, on and off
    ctx.stage_corpus(77, corpus, metric="cosine")
    for on in (True, False):
        with pytest.raises(surrealdb_amd.SdbvError):
            ctx.table_set_prefilter_l2(77, on)
    ctx.drop_table(77)


def test_l2_policy_env(ctx, monkeypatch):
    n, d = 3000, 32
    corpus = oracle.gen_f32(0x72, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    for name in ("SDBV_SCAN_PREFILTER_L2", "SDBV_SCAN_PREFILTER_L2_MIN_ROWS"):
        monkeypatch.delenv(name, raising=False)

    def staged():
        return ctx.stats()["bytes_staged"] - before

    def path():
        ctx.knn_bruteforce(78, corpus[0], 5)
        return ctx.stats()["last_scan_path"]

    ctx.stage_corpus(78, corpus, metric="euclidean")     # default: 500000 rows
    assert staged() == base_bytes(n, d) and path() == 0
    # the cosine tiers' variables give a euclidean table nothing
    for name in ("SDBV_SCAN_PREFILTER", "SDBV_SCAN_PREFILTER_MIN_ROWS",
                 "SDBV_SCAN_PREFILTER_I8", "SDBV_SCAN_PREFILTER_I8_MIN_ROWS",
                 "SDBV_SCAN_PREFILTER_I6", "SDBV_SCAN_PREFILTER_I6_MIN_ROWS"):
        monkeypatch.setenv(name, "1")
    ctx.stage_corpus(78, corpus, metric="euclidean")
    assert staged() == base_bytes(n, d) and path() == 0
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_L2_MIN_ROWS", str(n + 1))
    ctx.stage_corpus(78, corpus, metric="euclidean")
    assert staged() == base_bytes(n, d) and path() == 0
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_L2_MIN_ROWS", str(n))
    ctx.stage_corpus(78, corpus, metric="euclidean")
    assert staged() == base_bytes(n, d) + l2_bytes(n, d) and path() == PATH_L2
    ctx.stage_synthetic(78, n, d, metric="euclidean")
    assert staged() == base_bytes(n, d) + l2_bytes(n, d)
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_L2", "0")
    ctx.stage_corpus(78, corpus, metric="euclidean")
    assert staged() == base_bytes(n, d) and path() == 0
    ctx.drop_table(78)


def test_l2_policy_hnsw_finalize_has_no_shadow(ctx, monkeypatch):
    """A table staged for graph search never pays for the shadow, whatever
    the scan policy says."""
    n, d = 300, 16
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_L2_MIN_ROWS", "1")
    pts = oracle.gen_f32(0x73, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    h = ctx.hnsw_create(d, metric="euclidean")
    for p in pts:
        h.insert(p)
    h.finalize(79)
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    h.destroy()
    ctx.drop_table(79)
