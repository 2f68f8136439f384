"""Single-query prefilter (bf16 shadow + exact rescore) — GPU parity.

Every case runs knn_bruteforce with the table's shadow ON and compares ids
and distance BITS with the same call with the shadow OFF
(sdbv_table_set_prefilter) and with the CPU oracle, and asserts which path
ran (stats last_scan_path: 0 exact scan, 1 prefilter, 2 prefilter overflowed
then exact scan). Shapes are the smallest at which each mechanism can fail:
the prefilter sweeps 2048-row tiles, 8 rows per lane, one tile per block at
these sizes."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_TILE = 2048
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
    """(ids, dists, path, candidates) with the shadow on, then (ids, dists)
    with it off."""
    ctx.table_set_prefilter(table, True)
    on = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    on = (on[0].copy(), on[1].copy(), st["last_scan_path"],
          st["last_prefilter_candidates"])
    ctx.table_set_prefilter(table, False)
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
    (5, 16, 10),         # n < k: threshold +inf
    (999, 128, 10),      # partial tile
    (2049, 20, 64),      # crosses the 2048-row lane tile; d % 8 != 0: tail
    (50_000, 768, 10),   # many blocks; both merge levels
])
def test_prefilter_matches_exact_and_oracle(ctx, n, d, k):
    corpus = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    ctx.stage_corpus(31, corpus, metric="cosine")
    on, off = run_on_off(ctx, 31, q, k)
    assert on[2] == 1
    assert min(k, n) <= on[3] <= PF_CAND_CAP
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(31)


def test_prefilter_explicit_ids(ctx):
    n, d, k = 3000, 32, 5
    corpus = oracle.gen_f32(0x88, 0, n, d)
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    q = oracle.gen_f32(0x99, 0, 1, d)[0]
    ctx.stage_corpus(32, corpus, ids=ids, metric="cosine")
    on, off = run_on_off(ctx, 32, q, k)
    assert on[2] == 1
    assert_same(on, off)
    assert_oracle(on, corpus, q, k, ids=ids)
    ctx.drop_table(32)


def test_prefilter_duplicates_tie_order(ctx):
    """Exact duplicates of the best row in other lane tiles (8 rows) and
    other blocks (2048 rows): ties come out in ascending id order."""
    n, d, k = 6000, 64, 8
    corpus = oracle.gen_f32(0x77, 0, n, d)
    dup_rows = [7, 8, 2100, 5000, 5999]
    for r in dup_rows:
        corpus[r] = corpus[7]
    q = corpus[7].copy()
    ctx.stage_corpus(33, corpus, metric="cosine")
    on, off = run_on_off(ctx, 33, q, k)
    assert on[2] == 1
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    assert list(on[0][:5]) == dup_rows
    assert np.all(bits(on[1][:5]) == bits(on[1][:1]))
    ctx.drop_table(33)


def sub_resolution_corpus(n, d):
    """n rows equal to one bf16-exact vector times (1 + 1e-4 u), u in
    [-1, 1): far below the bf16 half-spacing (>= 2^-9), so every shadow row
    is the same vector and the approximate scores tell nothing."""
    import surrealdb_amd
    base = oracle.gen_f32(0x51, 0, 1, d)[0]
    base = np.array([surrealdb_amd.bf16_rne(v) for v in base],
                    dtype=np.float32)
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, size=(n, d))
    return (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)


def test_prefilter_sub_resolution_differences(ctx):
    n, d, k = 5000, 64, 10
    corpus = sub_resolution_corpus(n, d)
    q = oracle.gen_f32(0x52, 0, 1, d)[0]
    ctx.stage_corpus(34, corpus, metric="cosine")
    on, off = run_on_off(ctx, 34, q, k)
    assert on[2] == 1
    assert on[3] == n  # every row is a candidate: the true order is rescored
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(34)


def test_prefilter_candidate_overflow_falls_back(ctx):
    n, d, k = PF_CAND_CAP + 3616, 16, 10
    corpus = sub_resolution_corpus(n, d)
    q = oracle.gen_f32(0x53, 0, 1, d)[0]
    ctx.stage_corpus(35, corpus, metric="cosine")
    on, off = run_on_off(ctx, 35, q, k)
    assert on[2] == 2
    assert on[3] == n  # the counter keeps counting past the capacity
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    ctx.drop_table(35)


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
    corpus[n - 1, d - 1] = np.nan
    return corpus


@pytest.mark.parametrize("n,k", [(3000, 10), (40, 64)])
def test_prefilter_unsafe_rows(ctx, n, k):
    """Rows the bound cannot cover always reach the exact stage: results,
    NaN and infinite distances included, equal the shadow-off path's."""
    d = 32
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x62, 0, 1, d)[0]
    ctx.stage_corpus(36, corpus, metric="cosine")
    on, off = run_on_off(ctx, 36, q, k)
    assert on[2] == 1
    assert_same(on, off)
    ctx.drop_table(36)


@pytest.mark.parametrize("kind", ["zero", "nan", "huge", "tiny"])
def test_prefilter_unsafe_query_takes_exact_scan(ctx, kind):
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
    ctx.stage_corpus(37, corpus, metric="cosine")
    on, off = run_on_off(ctx, 37, q, k)
    assert on[2] == 0
    assert on[3] == 0
    assert_same(on, off)
    ctx.drop_table(37)


def base_bytes(n, d):
    n_pad = -(-n // 1024) * 1024
    return d * n_pad * 4 + n_pad * (8 + 8 + 4)  # cm, norms, ids, aux


def shadow_bytes(n, d):
    sn_pad = -(-n // PF_TILE) * PF_TILE
    return d * sn_pad * 2 + sn_pad * 4


def test_policy_small_table_has_no_shadow(ctx):
    n, d = 3000, 32
    corpus = oracle.gen_f32(0x71, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    ctx.stage_corpus(38, corpus, metric="cosine")
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    ctx.knn_bruteforce(38, corpus[0], 5)
    assert ctx.stats()["last_scan_path"] == 0
    ctx.table_set_prefilter(38, True)
    assert ctx.stats()["bytes_staged"] - before == \
        base_bytes(n, d) + shadow_bytes(n, d)
    ctx.table_set_prefilter(38, False)
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    ctx.drop_table(38)


def test_policy_env_opt_out_and_min_rows(ctx, monkeypatch):
    n, d = 3000, 32
    corpus = oracle.gen_f32(0x72, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_MIN_ROWS", "1000")
    ctx.stage_corpus(39, corpus, metric="cosine")  # policy builds the shadow
    assert ctx.stats()["bytes_staged"] - before == \
        base_bytes(n, d) + shadow_bytes(n, d)
    ctx.knn_bruteforce(39, corpus[0], 5)
    assert ctx.stats()["last_scan_path"] == 1
    monkeypatch.setenv("SDBV_SCAN_PREFILTER", "0")
    ctx.stage_corpus(39, corpus, metric="cosine")  # restage: opted out
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    ctx.stage_synthetic(39, n, d, metric="cosine")
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    monkeypatch.delenv("SDBV_SCAN_PREFILTER")
    ctx.stage_synthetic(39, n, d, metric="cosine")
    assert ctx.stats()["bytes_staged"] - before == \
        base_bytes(n, d) + shadow_bytes(n, d)
    ctx.stage_corpus(39, corpus, metric="euclidean")  # cosine only
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d) - 8 * 3072
    import surrealdb_amd
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.table_set_prefilter(39, True)
    ctx.drop_table(39)


def test_policy_hnsw_finalize_has_no_shadow(ctx, monkeypatch):
    """A table staged for graph search never pays for the shadow, whatever
    the scan policy says."""
    n, d = 300, 16
    monkeypatch.setenv("SDBV_SCAN_PREFILTER_MIN_ROWS", "1")
    pts = oracle.gen_f32(0x73, 0, n, d)
    before = ctx.stats()["bytes_staged"]
    h = ctx.hnsw_create(d, metric="cosine")
    for p in pts:
        h.insert(p)
    h.finalize(40)
    assert ctx.stats()["bytes_staged"] - before == base_bytes(n, d)
    h.destroy()
    ctx.drop_table(40)
