"""The all-distances route with the top-K selected on the device
(last_scan_path 21, 22 under a bitmap).

Every case runs twice. SDBV_SELECT_DEVICE_MIN_ROWS=0 admits these small
tables to the device select, and the path assertion says it ran. Then
SDBV_SELECT_DEVICE=0 sends the same call through the host selection (path
0): both read the same kernel's distance buffer, so ids and distance bits
must be equal for every metric and every input, NaN and inf included. On
finite inputs both also equal oracle.topk_f32 exactly (minkowski distances
at rtol 1e-12, as in test_gpu_parity.py)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ENV_ON = "SDBV_SELECT_DEVICE"
ENV_MIN = "SDBV_SELECT_DEVICE_MIN_ROWS"
PATH_HOST, PATH_DEVICE, PATH_DEVICE_MASKED = 0, 21, 22


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


@contextlib.contextmanager
def select_env(on=None, min_rows=None):
    """Set (or, with None, unset) the two policy variables, then restore."""
    old = {e: os.environ.get(e) for e in (ENV_ON, ENV_MIN)}
    for e, v in ((ENV_ON, on), (ENV_MIN, min_rows)):
        if v is None:
            os.environ.pop(e, None)
        else:
            os.environ[e] = str(v)
    try:
        yield
    finally:
        for e, v in old.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v


@functools.lru_cache(maxsize=None)
def corpus_of(seed, n, d):
    c = oracle.gen_f32(seed, 0, n, d)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def quantized(seed, n, d):
    """The coarse corpus of test_gpu_parity.py: element collisions, so
    hamming / jaccard distances fall into large tie groups."""
    c = np.round(oracle.gen_f32(seed, 0, n, d) * 0.25).astype(np.float32)
    c.setflags(write=False)
    return c


def call(ctx, table, q, k, allow):
    if allow is None:
        return ctx.knn_bruteforce(table, q, k)
    return ctx.knn_bruteforce_filtered(table, q, k, allow)


def both_routes(ctx, table, q, k, allow=None, count=None):
    """Device select, then host selection; paths asserted, results equal in
    every bit. Returns the device run's (ids, dists)."""
    if allow is None:
        want_path = PATH_DEVICE
    else:
        # no allowed row: the filtered call returns before any launch
        want_path = PATH_DEVICE_MASKED if count else PATH_HOST
    with select_env(min_rows=0):
        gids, gdists = call(ctx, table, q, k, allow)
        st = ctx.stats()
    assert st["last_scan_path"] == want_path, st["last_scan_path"]
    if want_path != PATH_HOST:
        assert st["last_scan_kernel_ms"] > 0
        assert st["last_merge_kernel_ms"] > 0
    if allow is not None:
        assert st["last_filter_rows"] == count
        assert st["last_rows_scanned"] == count
    with select_env(on=0, min_rows=0):
        hids, hdists = call(ctx, table, q, k, allow)
        assert ctx.stats()["last_scan_path"] == PATH_HOST
    assert np.array_equal(gids, hids), (gids, hids)
    assert np.array_equal(gdists.view(np.uint64), hdists.view(np.uint64))
    return gids, gdists


def expected(metric, corpus, q, k, allow=None, ids=None, order=0.0):
    rows = (np.arange(corpus.shape[0]) if allow is None
            else np.flatnonzero(allow))
    if rows.size == 0:
        return np.empty(0, np.uint64), np.empty(0, np.float64)
    oids, odists = oracle.topk_f32(metric, np.ascontiguousarray(corpus[rows]),
                                   q, k, order=order)
    pos = rows[oids.astype(np.int64)]
    return (pos.astype(np.uint64) if ids is None else ids[pos]), odists


def check_oracle(metric, got, want):
    gids, gdists = got
    eids, edists = want
    assert np.array_equal(gids, eids), (gids, eids)
    if metric == "minkowski":
        assert np.allclose(gdists, edists, rtol=1e-12, atol=0)
    else:
        assert np.array_equal(gdists.view(np.uint64), edists.view(np.uint64))


# ---- each of the 8 metrics -------------------------------------------------

METRIC_KS = [(m, k) for m in ("manhattan", "chebyshev", "hamming", "jaccard",
                              "minkowski", "pearson") for k in (1, 10, 100)]
METRIC_KS += [(m, k) for m in ("cosine", "euclidean") for k in (65, 100)]


@pytest.mark.parametrize("metric,k", METRIC_KS)
def test_each_metric(ctx, metric, k):
    n, d = 999, 20
    coarse = metric in ("hamming", "jaccard")
    corpus = quantized(0x5DB1, n, d) if coarse else corpus_of(0x5DB1, n, d)
    q = (quantized(0xBEEF, 1, d) if coarse else corpus_of(0xBEEF, 1, d))[0]
    order = 3.0 if metric == "minkowski" else 0.0
    ctx.stage_corpus(60, corpus, metric=metric, order=order or None)
    got = both_routes(ctx, 60, q, k)
    assert got[0].size == k
    check_oracle(metric, got, expected(metric, corpus, q, k, order=order))
    ctx.drop_table(60)


# ---- boundaries -------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 70, 256, 257])
def test_boundaries(ctx, n):
    d = 4
    corpus = corpus_of(0x5DB1, n, d)
    q = corpus_of(0xBEEF, 1, d)[0]
    ctx.stage_corpus(61, corpus, metric="manhattan")
    for k in (n - 1, n, n + 30):
        if k < 1:
            continue
        got = both_routes(ctx, 61, q, k)
        assert got[0].size == min(k, n)
        check_oracle("manhattan", got, expected("manhattan", corpus, q, k))
    ctx.drop_table(61)


# ---- all rows identical: the row digits decide ------------------------------

@pytest.fixture(scope="module")
def identical(ctx):
    n, d = 70001, 4
    corpus = np.tile(np.array([1, 2, 3, 4], np.float32), (n, 1))
    ids = np.arange(n, dtype=np.uint64) * 7 + 100
    ctx.stage_corpus(62, corpus, ids=ids, metric="hamming")
    yield corpus, ids, np.array([1, 0, 3, 0], np.float32)
    ctx.drop_table(62)


@pytest.mark.parametrize("k", [300, 65536])
def test_identical_rows(ctx, identical, k):
    corpus, ids, q = identical
    gids, gdists = both_routes(ctx, 62, q, k)
    assert np.array_equal(gids, ids[:k])
    check_oracle("hamming", (gids, gdists),
                 expected("hamming", corpus, q, k, ids=ids))


@pytest.mark.parametrize("k", [300, 65536])
def test_identical_rows_under_a_bitmap(ctx, identical, k):
    corpus, ids, q = identical
    n = corpus.shape[0]
    allow = np.ones(n, bool)
    allow[:66000] = False
    gids, gdists = both_routes(ctx, 62, q, k, allow, n - 66000)
    m = min(k, n - 66000)
    assert np.array_equal(gids, ids[66000:66000 + m])
    check_oracle("hamming", (gids, gdists),
                 expected("hamming", corpus, q, k, allow, ids=ids))


# ---- near-ties on cosine ----------------------------------------------------

@pytest.mark.parametrize("k", [65, 500])
def test_cosine_near_ties(ctx, k):
    """Rows s_i * x against the query x: distances within a few ulps of 0 on
    both sides, exact duplicates among them."""
    n, d = 3000, 32
    x = corpus_of(0x77, 1, d)[0]
    rng = np.random.default_rng(21)
    scales = rng.uniform(0.25, 4.0, n).astype(np.float32)
    scales[1000:2000] = scales[:1000]  # exact duplicate rows
    corpus = (scales[:, None] * x[None, :]).astype(np.float32)
    ctx.stage_corpus(63, corpus, metric="cosine")
    got = both_routes(ctx, 63, x, k)
    assert np.abs(got[1]).max() < 1e-6
    check_oracle("cosine", got, expected("cosine", corpus, x, k))
    ctx.drop_table(63)


# ---- non-finite distances ---------------------------------------------------

@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_non_finite(ctx, metric):
    n, d = 2000, 16
    corpus = corpus_of(0x5DB1, n, d).copy()
    corpus[0] = 0.0
    corpus[255, 3] = np.inf
    corpus[256, 5] = np.nan
    corpus[n - 1] = 1e30
    q = corpus_of(0xBEEF, 1, d)[0]
    ctx.stage_corpus(64, corpus, metric=metric)
    for k in (65, n):
        gids, gdists = both_routes(ctx, 64, q, k)
        assert gids.size == k
    assert np.isnan(gdists).any()  # k = n holds the NaN rows
    ctx.drop_table(64)


# ---- filtered ---------------------------------------------------------------

FLT_N, FLT_D = 5000, 16


@pytest.mark.parametrize("metric,k", [("manhattan", 10), ("cosine", 100)])
@pytest.mark.parametrize("p", [0.5, 0.02])
def test_filtered_random(ctx, metric, k, p):
    corpus = corpus_of(0x5DB1, FLT_N, FLT_D)
    q = corpus_of(0xBEEF, 1, FLT_D)[0]
    allow = np.random.default_rng(FLT_N + int(p * 100)).random(FLT_N) < p
    ctx.stage_corpus(65, corpus, metric=metric)
    got = both_routes(ctx, 65, q, k, allow, int(allow.sum()))
    check_oracle(metric, got, expected(metric, corpus, q, k, allow))
    ctx.drop_table(65)


def test_filtered_edges(ctx):
    import surrealdb_amd
    metric, k = "manhattan", 10
    corpus = corpus_of(0x5DB1, FLT_N, FLT_D)
    q = corpus_of(0xBEEF, 1, FLT_D)[0]
    ctx.stage_corpus(65, corpus, metric=metric)
    # no allowed row
    none = np.zeros(FLT_N, bool)
    gids, _ = both_routes(ctx, 65, q, k, none, 0)
    assert gids.size == 0
    # fewer allowed rows than k
    few = np.zeros(FLT_N, bool)
    few[[3, 2500, FLT_N - 1]] = True
    got = both_routes(ctx, 65, q, k, few, 3)
    assert got[0].size == 3
    check_oracle(metric, got, expected(metric, corpus, q, k, few))
    # the unfiltered nearest rows disallowed
    near, _ = expected(metric, corpus, q, 50)
    hole = np.ones(FLT_N, bool)
    hole[near.astype(np.int64)] = False
    got = both_routes(ctx, 65, q, k, hole, FLT_N - 50)
    assert not np.intersect1d(got[0], near).size
    check_oracle(metric, got, expected(metric, corpus, q, k, hole))
    # tail bits set past n
    clean = np.random.default_rng(9).random(FLT_N) < 0.3
    clean[FLT_N - 40:] = True
    words = surrealdb_amd._allow_words(clean, FLT_N).copy()
    words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for kk in (k, FLT_N):
        got = both_routes(ctx, 65, q, kk, words, int(clean.sum()))
        check_oracle(metric, got, expected(metric, corpus, q, kk, clean))
    ctx.drop_table(65)


# ---- the cap and the default policy -----------------------------------------

def test_k_above_the_cap_keeps_the_host_route(ctx):
    n, d, k = 70001, 4, 65537
    corpus = corpus_of(0x5DB1, n, d)
    q = corpus_of(0xBEEF, 1, d)[0]
    ctx.stage_corpus(66, corpus, metric="manhattan")
    with select_env(min_rows=0):
        got = ctx.knn_bruteforce(66, q, k)
        assert ctx.stats()["last_scan_path"] == PATH_HOST
    check_oracle("manhattan", got, expected("manhattan", corpus, q, k))
    ctx.drop_table(66)


def test_default_policy(ctx):
    n, d, k = 1000, 16, 5
    corpus = corpus_of(0x5DB1, n, d)
    q = corpus_of(0xBEEF, 1, d)[0]
    want = expected("manhattan", corpus, q, k)
    ctx.stage_corpus(67, corpus, metric="manhattan")
    with select_env():  # both unset: the default minimum is at least 16384
        got = ctx.knn_bruteforce(67, q, k)
        assert ctx.stats()["last_scan_path"] == PATH_HOST
    check_oracle("manhattan", got, want)
    with select_env(min_rows=1000):
        got = ctx.knn_bruteforce(67, q, k)
        assert ctx.stats()["last_scan_path"] == PATH_DEVICE
    check_oracle("manhattan", got, want)
    with select_env(min_rows=1001):
        ctx.knn_bruteforce(67, q, k)
        assert ctx.stats()["last_scan_path"] == PATH_HOST
    ctx.drop_table(67)


# ---- batch ------------------------------------------------------------------

def test_batch_inherits_the_route(ctx):
    n, d, b, k = 8000, 16, 3, 10
    corpus = corpus_of(0x5DB1, n, d)
    Q = corpus_of(0xBEEF, b, d)
    ctx.stage_corpus(68, corpus, metric="manhattan")
    with select_env(min_rows=0):
        bids, bdists = ctx.knn_batch(68, Q, k)
        assert ctx.stats()["last_scan_path"] == PATH_DEVICE
        for j in range(b):
            sids, sdists = ctx.knn_bruteforce(68, Q[j], k)
            assert np.array_equal(bids[j], sids)
            assert np.array_equal(bdists[j].view(np.uint64),
                                  sdists.view(np.uint64))
            check_oracle("manhattan", (sids, sdists),
                         expected("manhattan", corpus, Q[j], k))
    ctx.drop_table(68)


# ---- scratch reuse ----------------------------------------------------------

def test_scratch_reuse(ctx):
    """A k = 65536 call grows the scratch; a k = 1 call on another table and
    an ordinary cosine scan after it are not disturbed."""
    big = corpus_of(0x5DB1, 70001, 4)
    small = corpus_of(0x88, 999, 20)
    cos = corpus_of(0x99, 3000, 32)
    qb, qs, qc = (corpus_of(0xBEEF, 1, dd)[0] for dd in (4, 20, 32))
    ctx.stage_corpus(69, big, metric="manhattan")
    ctx.stage_corpus(70, small, metric="chebyshev")
    ctx.stage_corpus(71, cos, metric="cosine")
    with select_env(min_rows=0):
        got = ctx.knn_bruteforce(69, qb, 65536)
        assert ctx.stats()["last_scan_path"] == PATH_DEVICE
        check_oracle("manhattan", got,
                     expected("manhattan", big, qb, 65536))
        got = ctx.knn_bruteforce(70, qs, 1)
        assert ctx.stats()["last_scan_path"] == PATH_DEVICE
        check_oracle("chebyshev", got, expected("chebyshev", small, qs, 1))
        got = ctx.knn_bruteforce(71, qc, 10)
        assert ctx.stats()["last_scan_path"] not in (PATH_DEVICE,
                                                     PATH_DEVICE_MASKED)
        check_oracle("cosine", got, expected("cosine", cos, qc, 10))
    for t in (69, 70, 71):
        ctx.drop_table(t)
