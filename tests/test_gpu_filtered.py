"""Filtered brute-force KNN (sdbv_knn_bruteforce_filtered) against the CPU
oracle on the allowed subset: oracle.topk_f32(metric, corpus[rows], q, k)
with rows = np.flatnonzero(allow); expected ids are ids[rows[oids]]. Every
comparison is exact equality of ids and of distance bits.

Each case runs on both device paths: SDBV_FILTER_ROWLIST_MAX=0 forces the
masked scan (last_scan_path 7), the default takes the row-list path
(last_scan_path 8) for the at most 16384 allowed rows these shapes have."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ENV = "SDBV_FILTER_ROWLIST_MAX"
PATH_MASKED, PATH_LIST = 7, 8


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


@contextlib.contextmanager
def rowlist_max(value):
    """Set (or, with None, unset) SDBV_FILTER_ROWLIST_MAX, then restore."""
    old = os.environ.get(ENV)
    if value is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


@functools.lru_cache(maxsize=None)
def corpus_of(seed, n, d):
    c = oracle.gen_f32(seed, 0, n, d)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def query_of(seed, d):
    q = oracle.gen_f32(seed, 0, 1, d)[0]
    q.setflags(write=False)
    return q


def expected(metric, corpus, q, k, allow, ids=None):
    rows = np.flatnonzero(allow)
    if rows.size == 0:
        return np.empty(0, np.uint64), np.empty(0, np.float64), 0
    oids, odists = oracle.topk_f32(metric, np.ascontiguousarray(corpus[rows]),
                                   q, k)
    pos = rows[oids.astype(np.int64)]
    eids = pos.astype(np.uint64) if ids is None else ids[pos]
    return eids, odists, rows.size


def check_both_paths(ctx, table, metric, corpus, q, k, allow, ids=None,
                     allow_arg=None):
    """Run the filtered call on the masked scan and on the row list; both
    must equal the oracle on the subset exactly."""
    eids, edists, count = expected(metric, corpus, q, k, allow, ids)
    arg = allow if allow_arg is None else allow_arg
    out = {}
    for value, path in ((0, PATH_MASKED), (None, PATH_LIST)):
        with rowlist_max(value):
            gids, gdists = ctx.knn_bruteforce_filtered(table, q, k, arg)
        st = ctx.stats()
        assert st["last_filter_rows"] == count
        assert st["last_rows_scanned"] == count
        if count:
            assert st["last_scan_path"] == path
        assert gids.size == min(k, count)
        assert np.array_equal(gids, eids), (
            f"path {path}: ids {gids} != {eids}")
        assert np.array_equal(gdists.view(np.uint64), edists.view(np.uint64)), (
            f"path {path}: distance bits differ")
        out[path] = (gids, gdists)
    return out


# ---- random masks ---------------------------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,d,k", [(999, 20, 10), (5000, 128, 10),
                                   (3000, 768, 64)])
@pytest.mark.parametrize("p", [0.5, 0.02])
def test_random_masks(ctx, metric, n, d, k, p):
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(n + int(p * 100)).random(n) < p
    ctx.stage_corpus(40, corpus, metric=metric)
    check_both_paths(ctx, 40, metric, corpus, q, k, allow)
    ctx.drop_table(40)


# ---- edge masks at n = 3000, d = 32 ---------------------------------------

EDGE_N, EDGE_D, EDGE_K = 3000, 32, 10


def edge_masks():
    n = EDGE_N
    m = {}
    a = np.zeros(n, bool)
    a[0] = True
    m["only_row_0"] = a
    a = np.zeros(n, bool)
    a[n - 1] = True
    m["only_last_row"] = a
    a = np.ones(n, bool)
    a[1024:2048] = False
    m["tile_1024_2047_clear"] = a
    a = np.random.default_rng(5).random(n) < 0.5
    a[256:512] = False
    a[512:768] = True
    m["wave_clear_then_wave_full"] = a
    a = np.zeros(n, bool)
    rng = np.random.default_rng(6)
    for s in range(0, n, 256):
        a[s + int(rng.integers(0, min(256, n - s)))] = True
    m["one_row_per_256"] = a
    a = np.zeros(n, bool)
    a[[3, 1500, 2999]] = True
    m["fewer_than_k"] = a
    return m


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("name", sorted(edge_masks()))
def test_edge_masks(ctx, metric, name):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    allow = edge_masks()[name]
    ctx.stage_corpus(41, corpus, metric=metric)
    got = check_both_paths(ctx, 41, metric, corpus, q, EDGE_K, allow)
    if name == "fewer_than_k":
        for gids, gdists in got.values():
            assert gids.size == 3
            assert np.all(np.diff(gdists) >= 0)
    ctx.drop_table(41)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_all_ones_equals_unfiltered(ctx, metric):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    ctx.stage_corpus(41, corpus, metric=metric)
    uids, udists = ctx.knn_bruteforce(41, q, EDGE_K)
    got = check_both_paths(ctx, 41, metric, corpus, q, EDGE_K,
                           np.ones(EDGE_N, bool))
    for gids, gdists in got.values():
        assert np.array_equal(gids, uids)
        assert np.array_equal(gdists.view(np.uint64), udists.view(np.uint64))
    ctx.drop_table(41)


def test_all_zeros(ctx):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    ctx.stage_corpus(41, corpus, metric="cosine")
    got = check_both_paths(ctx, 41, "cosine", corpus, q, EDGE_K,
                           np.zeros(EDGE_N, bool))
    for gids, gdists in got.values():
        assert gids.size == 0 and gdists.size == 0
    ctx.drop_table(41)


# ---- tail bits -------------------------------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_tail_bits_ignored(ctx, metric):
    """n = 999 with the last word all ones: bits 39..63 of word 15 name rows
    999..1023, which do not exist. The result equals the clean mask's."""
    n, d, k = 999, 20, 10
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    clean = np.random.default_rng(9).random(n) < 0.3
    clean[960:] = True
    import surrealdb_amd
    words = surrealdb_amd._allow_words(clean, n).copy()
    words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    ctx.stage_corpus(42, corpus, metric=metric)
    check_both_paths(ctx, 42, metric, corpus, q, k, clean, allow_arg=words)
    ctx.drop_table(42)


# ---- ties -------------------------------------------------------------------

def test_ties_follow_the_mask(ctx):
    base = oracle.gen_f32(0x77, 0, 500, 64)
    corpus = np.concatenate([base, base[:20]])  # exact duplicates
    q = base[7].copy()
    ctx.stage_corpus(43, corpus, metric="euclidean")
    allow = np.ones(520, bool)
    allow[7] = False
    for gids, gdists in check_both_paths(ctx, 43, "euclidean", corpus, q, 8,
                                         allow).values():
        assert gids[0] == 507 and gdists[0] == 0.0
    allow = np.ones(520, bool)
    allow[507] = False
    for gids, gdists in check_both_paths(ctx, 43, "euclidean", corpus, q, 8,
                                         allow).values():
        assert gids[0] == 7 and gdists[0] == 0.0
    ctx.drop_table(43)


# ---- explicit ids ------------------------------------------------------------

def test_explicit_ids(ctx):
    corpus = corpus_of(0x88, 1000, 32)
    ids = np.arange(1000, dtype=np.uint64) * 7 + 100
    q = query_of(0x99, 32)
    allow = np.random.default_rng(11).random(1000) < 0.5
    ctx.stage_corpus(44, corpus, ids=ids, metric="cosine")
    check_both_paths(ctx, 44, "cosine", corpus, q, 5, allow, ids=ids)
    ctx.drop_table(44)


# ---- the all-distances routes ------------------------------------------------

@pytest.mark.parametrize("metric,n,d,k", [("cosine", 2000, 32, 65),
                                          ("manhattan", 1000, 16, 5)])
def test_other_routes(ctx, metric, n, d, k):
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(12).random(n) < 0.5
    eids, edists, count = expected(metric, corpus, q, k, allow)
    ctx.stage_corpus(45, corpus, metric=metric)
    gids, gdists = ctx.knn_bruteforce_filtered(45, q, k, allow)
    st = ctx.stats()
    assert st["last_scan_path"] == 0
    assert st["last_filter_rows"] == count
    assert np.array_equal(gids, eids)
    assert np.array_equal(gdists.view(np.uint64), edists.view(np.uint64))
    ctx.drop_table(45)


# ---- a table with a prefilter shadow -----------------------------------------

def test_shadowed_table(ctx):
    """A filtered call on a shadowed table is exact and takes path 7 or 8;
    an unfiltered call afterwards still takes the tier's own path and is
    still exact (no scratch shared by accident)."""
    n, d, k = 4096, 64, 10
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(13).random(n) < 0.5
    oids, odists = oracle.topk_f32("cosine", corpus, q, k)
    ctx.stage_corpus(46, corpus, metric="cosine")
    for set_tier, tier_path in (
            (lambda: ctx.table_set_prefilter_kind(46, 2), 3),
            (lambda: ctx.table_set_prefilter_i6(46), 5)):
        set_tier()
        check_both_paths(ctx, 46, "cosine", corpus, q, k, allow)
        uids, udists = ctx.knn_bruteforce(46, q, k)
        assert ctx.stats()["last_scan_path"] == tier_path
        assert np.array_equal(uids, oids)
        assert np.array_equal(udists.view(np.uint64), odists.view(np.uint64))
    ctx.drop_table(46)


# ---- the rule itself picks the masked scan -------------------------------------

def test_dense_mask_takes_masked_scan_by_rule(ctx):
    n, d, k = 40000, 32, 10
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(14).random(n) < 0.5
    eids, edists, count = expected("cosine", corpus, q, k, allow)
    assert count > 16384
    ctx.stage_corpus(47, corpus, metric="cosine")
    with rowlist_max(None):
        gids, gdists = ctx.knn_bruteforce_filtered(47, q, k, allow)
    st = ctx.stats()
    assert st["last_scan_path"] == PATH_MASKED
    assert st["last_filter_rows"] == count
    assert np.array_equal(gids, eids)
    assert np.array_equal(gdists.view(np.uint64), edists.view(np.uint64))
    ctx.drop_table(47)


# ---- a graph-staged table -----------------------------------------------------

def test_hnsw_finalized_table(ctx):
    n, d, k = 300, 16, 5
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    h = ctx.hnsw_create(d, metric="euclidean")
    for i in range(n):
        h.insert(corpus[i])
    h.finalize(48)
    allow = np.random.default_rng(15).random(n) < 0.5
    check_both_paths(ctx, 48, "euclidean", corpus, q, k, allow)
    h.destroy()
    ctx.drop_table(48)


# ---- the operator mirror -------------------------------------------------------

def test_knn_topk_row_filter(ctx):
    from surrealdb_amd.host import KnnTopK
    n, d, k = 999, 20, 10
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(16).random(n) < 0.5
    eids, edists, _ = expected("cosine", corpus, q, k, allow)
    ctx.stage_corpus(49, corpus, metric="cosine")
    gids, gdists = KnnTopK(ctx, 49, q, k, "cosine", row_filter=allow).execute()
    assert np.array_equal(gids, eids)
    assert np.array_equal(gdists.view(np.uint64), edists.view(np.uint64))
    uids, _ = KnnTopK(ctx, 49, q, k, "cosine").execute()
    assert np.array_equal(uids, oracle.topk_f32("cosine", corpus, q, k)[0])
    ctx.drop_table(49)


# ---- bad arguments --------------------------------------------------------------

def raw_call(ctx, table, q, d, k, words, nwords):
    import surrealdb_amd
    ids = np.empty(k, dtype=np.uint64)
    dists = np.empty(k, dtype=np.float64)
    out_n = ctypes.c_uint32(0)
    wp = (None if words is None
          else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return surrealdb_amd.lib().sdbv_knn_bruteforce_filtered(
        ctx._ptr, table, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), d,
        k, wp, nwords, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        dists.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        ctypes.byref(out_n))


def test_bad_arguments(ctx):
    import surrealdb_amd
    n, d, k = 999, 20, 10
    corpus = corpus_of(0x5DB1, n, d)
    q = np.ascontiguousarray(query_of(0xBEEF, d))
    ctx.stage_corpus(50, corpus, metric="cosine")
    words = np.full(17, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    OK, NO_TABLE, BAD_ARG = 0, -2, -3
    assert raw_call(ctx, 50, q, d, k, words, 16) == OK
    assert raw_call(ctx, 50, q, d, k, words, 15) == BAD_ARG
    assert raw_call(ctx, 50, q, d, k, words, 17) == BAD_ARG
    assert raw_call(ctx, 50, q, d, k, None, 16) == BAD_ARG
    assert raw_call(ctx, 50, q, d + 4, k, words, 16) == BAD_ARG  # d mismatch
    assert raw_call(ctx, 50, q, d, 0, words, 16) == BAD_ARG
    assert raw_call(ctx, 51, q, d, k, words, 16) == NO_TABLE
    # through the wrapper: an allow array of the wrong length never reaches
    # the library
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.knn_bruteforce_filtered(50, q, k, np.ones(n + 1, bool))
    with pytest.raises(surrealdb_amd.SdbvError):
        ctx.knn_bruteforce_filtered(50, q, k, np.zeros(15, np.uint64))
    with pytest.raises(surrealdb_amd.SdbvError, match="bad argument"):
        ctx.knn_bruteforce_filtered(50, q[:16], k, np.ones(n, bool))
    ctx.drop_table(50)
