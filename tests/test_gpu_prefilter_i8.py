"""Single-query prefilter, int8 tier (int8 shadow + per-row bound + exact
rescore) — GPU parity.

Every case runs knn_bruteforce with the table's int8 shadow ON and compares
ids and distance BITS with the same call with no shadow
(sdbv_table_set_prefilter_kind) and with the CPU oracle, and asserts which
path ran (stats last_scan_path: 0 exact scan, 3 int8 prefilter, 4 int8
prefilter overflowed then exact scan). Shapes are the smallest at which each
mechanism can fail: the int8 prefilter sweeps 4096-row tiles, 16 rows per
lane, fed to the block select in two 2048-row halves, one tile per block at
these sizes."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_TILE = 2048
PF8_TILE = 4096
PF_CAND_CAP = 16384


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run_on_off(ctx, table, q, k):
    """(ids, dists, path, candidates) with the int8 shadow, then (ids,
    dists) with no shadow."""
    ctx.table_set_prefilter_kind(table, 2)
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
    (5, 16, 10),              # n < k: threshold +inf
    (999, 128, 10),           # partial tile, first select half only
    (PF8_TILE + 1, 20, 64),   # one row past the tile; d % 8 != 0: tail
    (50_000, 768, 10),        # many blocks; both merge levels
])
def test_i8_matches_exact_and_oracle(ctx, n, d, k):
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    ctx.stage_corpus(51, corpus, metric="cosine")
    on, off = run_on_off(ctx, 51, q, k)
    print(f"n={n} d={d} k={k}: candidates {on[3]}")
    assert on[2] == 3
    assert min(k, n) <= on[3] <= PF_CAND_CAP
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(51)


def test_i8_explicit_ids(ctx):
    n, d, k = 3000, 32, 5
    corpus = oracle.gen_f32(0x88, 0, n, d)
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    q = oracle.gen_f32(0x99, 0, 1, d)[0]
    ctx.stage_corpus(52, corpus, ids=ids, metric="cosine")
    on, off = run_on_off(ctx, 52, q, k)
    assert on[2] == 3
    assert_same(on, off)
    assert_oracle(on, corpus, q, k, ids=ids)
    ctx.drop_table(52)


def test_i8_duplicates_tie_order(ctx):
    """Exact duplicates of the best row in the same lane group, in other
    lane groups (16 rows), in the other select half (2048 rows) and in
    other blocks (4096 rows): ties come out in ascending id order."""
    n, d, k = 9000, 64, 8
    corpus = oracle.gen_f32(0x77, 0, n, d)
    dup_rows = [7, 8, 15, 16, 2100, 4100, 8999]
    for r in dup_rows:
        corpus[r] = corpus[7]
    q = corpus[7].copy()
    ctx.stage_corpus(53, corpus, metric="cosine")
    on, off = run_on_off(ctx, 53, q, k)
    assert on[2] == 3
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    assert list(on[0][:7]) == dup_rows
    assert np.all(bits(on[1][:7]) == bits(on[1][:1]))
    ctx.drop_table(53)


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
    corpus[16] = 2.5                     # constant row: every code is 127
    corpus[17] = 1e-3                    # one dominant element: the other
    corpus[17, 6] = -50.0                # codes are 0
    corpus[n - 1, d - 1] = np.nan
    return corpus


@pytest.mark.parametrize("n,k", [(3000, 10), (40, 64)])
def test_i8_unsafe_rows(ctx, n, k):
    """Rows the bound cannot cover always reach the exact stage: results,
    NaN and infinite distances included, equal the shadow-off path's."""
    d = 32
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x62, 0, 1, d)[0]
    ctx.stage_corpus(54, corpus, metric="cosine")
    on, off = run_on_off(ctx, 54, q, k)
    assert on[2] == 3
    assert_same(on, off)
    # the constant and the dominant-element row as the best rows
    for r in (16, 17):
        on, off = run_on_off(ctx, 54, corpus[r].copy(), k)
        assert on[2] == 3
        assert_same(on, off)
    ctx.drop_table(54)


@pytest.mark.parametrize("kind", ["zero", "nan", "huge", "tiny"])
def test_i8_unsafe_query_takes_exact_scan(ctx, kind):
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
    ctx.stage_corpus(55, corpus, metric="cosine")
    on, off = run_on_off(ctx, 55, q, k)
    assert on[2] == 0
    assert on[3] == 0
    assert_same(on, off)
    ctx.drop_table(55)


def test_i8_candidate_overflow_falls_back(ctx):
    """Rows equal to one vector times (1 + 1e-4 u), u in [-1, 1): far below
    the int8 step (>= 1/254 of the largest element), so every row's interval
    [l, u] holds every other row's distance and all rows are candidates."""
    n, d, k = PF_CAND_CAP + 3616, 16, 10
    base = oracle.gen_f32(0x51, 0, 1, d)[0]
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, size=(n, d))
    corpus = (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)
    q = oracle.gen_f32(0x53, 0, 1, d)[0]
    ctx.stage_corpus(56, corpus, metric="cosine")
    on, off = run_on_off(ctx, 56, q, k)
    assert on[2] == 4
    assert on[3] == n  # the counter keeps counting past the capacity
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(56)


def base_bytes(n, d):
    n_pad = -(-n // 1024) * 1024
    return d * n_pad * 4 + n_pad * (8 + 8 + 4)  # cm, norms, ids, aux


def bf16_bytes(n, d):
    sn_pad = -(-n // PF_TILE) * PF_TILE
    return d * sn_pad * 2 + sn_pad * 4


def i8_bytes(n, d):
    sn_pad = -(-n // PF8_TILE) * PF8_TILE
    return d * sn_pad + 8 * sn_pad


def test_i8_switching_kinds_accounts_bytes(ctx):
    n, d = 5000, 32
    corpus = oracle.gen_f32(0x71, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    ctx.stage_corpus(57, corpus, metric="cosine")

    def staged():
        return ctx.stats()["bytes_staged"] - before

    def path():
        ctx.knn_bruteforce(57, corpus[0], 5)
        return ctx.stats()["last_scan_path"]

    assert staged() == base_bytes(n, d) and path() == 0
    ctx.table_set_prefilter_kind(57, 2)
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    ctx.table_set_prefilter_kind(57, 2)  # already there: nothing changes
    assert staged() == base_bytes(n, d) + i8_bytes(n, d)
    ctx.table_set_prefilter_kind(57, 1)
    assert staged() == base_bytes(n, d) + bf16_bytes(n, d) and path() == 1
    ctx.table_set_prefilter_kind(57, 2)
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    ctx.table_set_prefilter(57, True)    # the bf16 switch replaces int8
    assert staged() == base_bytes(n, d) + bf16_bytes(n, d) and path() == 1
    ctx.table_set_prefilter_kind(57, 0)
    assert staged() == base_bytes(n, d) and path() == 0
    ctx.table_set_prefilter_kind(57, 2)
    ctx.table_set_prefilter(57, False)   # off frees whichever shadow
    assert staged() == base_bytes(n, d) and path() == 0
    import surrealdb_amd
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.table_set_prefilter_kind(57, 3)
    ctx.stage_corpus(57, corpus, metric="euclidean")  # cosine only
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.table_set_prefilter_kind(57, 2)
    ctx.drop_table(57)


def test_i8_policy_env(ctx, monkeypatch):
    n, d = 3000, 32
    corpus = oracle.gen_f32(0x72, 0, n, d)
    before = ctx.stats()["bytes_staged"]

    def staged():
        return ctx.stats()["bytes_staged"] - before

    def path():
        ctx.knn_bruteforce(58, corpus[0], 5)
        return ctx.stats()["last_scan_path"]

    # the int8 threshold alone builds nothing: no shadow below the first one
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8_MIN_ROWS", "1000")
    ctx.stage_corpus(58, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) and path() == 0
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_MIN_ROWS", "1000")
    ctx.stage_corpus(58, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + i8_bytes(n, d) and path() == 3
    ctx.stage_synthetic(58, n, d, metric="cosine")
    assert staged() == base_bytes(n, d) + i8_bytes(n, d)
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8_MIN_ROWS", "3001")
    ctx.stage_corpus(58, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + bf16_bytes(n, d) and path() == 1
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8_MIN_ROWS", "1000")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_I8", "0")
    ctx.stage_corpus(58, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) + bf16_bytes(n, d) and path() == 1
    monkeypatch.delenv("SDBV_SCAN_PREFILTER_I8")
    monkeypatch.setenv("SDBV_SCAN_PREFILTER", "0")  # no shadow of any kind
    ctx.stage_corpus(58, corpus, metric="cosine")
    assert staged() == base_bytes(n, d) and path() == 0
    ctx.drop_table(58)
