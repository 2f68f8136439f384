"""Filtered brute-force KNN on a euclidean table with the l2 shadow: the
shadow streamed under the allowed-row bitmap.

The expected value is the CPU oracle on the allowed subset; every comparison
is exact equality of ids and of distance bits, and every case asserts which
path ran (stats last_scan_path: 19 the l2 shadow under a filter, 20 the same
after a candidate overflow and the masked scan, 17 the unfiltered call).
SDBV_FILTER_ROWLIST_MAX=0 and SDBV_FILTER_PREFILTER_MIN_ROWS=0 bring the path
down to a table of 9000 rows: three 4096-row tiles, a wave covers 1024 rows
of the bitmap."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, D, K = 9000, 64, 8
PF_CAND_CAP = 16384
PATH_UNFILTERED, PATH_FILTERED, PATH_FILTERED_OVERFLOW = 17, 19, 20
TABLE = 81


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def corpus():
    c = oracle.gen_f32(0x5DB1, 0, N, D)
    c.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def query():
    q = oracle.gen_f32(0xBEEF, 0, 1, D)[0]
    q.setflags(write=False)
    return q


@pytest.fixture(scope="module")
def ctx(corpus):
    import surrealdb_amd
    c = surrealdb_amd.Context()
    c.stage_corpus(TABLE, corpus, metric="euclidean")
    c.table_set_prefilter_l2(TABLE, True)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def filter_env(monkeypatch):
    monkeypatch.setenv("SDBV_FILTER_ROWLIST_MAX", "0")
    monkeypatch.setenv("SDBV_FILTER_PREFILTER_MIN_ROWS", "0")
    monkeypatch.delenv("SDBV_FILTER_PREFILTER", raising=False)


def masks():
    m = {"all_ones": np.ones(N, bool),
         "random_half": np.random.default_rng(7).random(N) < 0.5}
    a = np.zeros(N, bool)
    rng = np.random.default_rng(8)
    for s in range(0, N, 1024):
        a[s + int(rng.integers(0, min(1024, N - s)))] = True
    m["one_row_per_1024"] = a
    a = np.random.default_rng(9).random(N) < 0.5
    a[5120:6144] = False                 # the second wave of the second tile
    m["wave_span_clear"] = a
    a = np.zeros(N, bool)
    a[[3, 4097, 8999]] = True
    m["fewer_than_k"] = a
    return m


def oracle_subset(corpus, q, k, allow):
    rows = np.flatnonzero(allow)
    oids, odists = oracle.topk_f32(
        "euclidean", np.ascontiguousarray(corpus[rows]), q, k)
    return rows[oids.astype(np.int64)].astype(np.uint64), odists, rows.size


def unfiltered(ctx, corpus, q):
    ids, dists = ctx.knn_bruteforce(TABLE, q, K)
    assert ctx.stats()["last_scan_path"] == PATH_UNFILTERED
    oids, odists = oracle.topk_f32("euclidean", corpus, q, K)
    assert np.array_equal(ids, oids)
    assert np.array_equal(bits(dists), bits(odists))


@pytest.mark.parametrize("name", sorted(masks()))
def test_masks(ctx, corpus, query, name):
    allow = masks()[name]
    eids, edists, count = oracle_subset(corpus, query, K, allow)
    if name == "fewer_than_k":
        assert count < K
    unfiltered(ctx, corpus, query)
    gids, gdists = ctx.knn_bruteforce_filtered(TABLE, query, K, allow)
    st = ctx.stats()
    print(f"{name}: allowed {count}, candidates "
          f"{st['last_prefilter_candidates']}, path {st['last_scan_path']}")
    assert st["last_scan_path"] == PATH_FILTERED
    assert st["last_filter_rows"] == count
    assert st["last_rows_scanned"] == count
    assert min(K, count) <= st["last_prefilter_candidates"] <= count
    assert np.array_equal(gids, eids)
    assert np.array_equal(bits(gdists), bits(edists))
    unfiltered(ctx, corpus, query)      # the shadow is only read


def test_policy_off_takes_the_masked_scan(ctx, corpus, query, monkeypatch):
    allow = masks()["random_half"]
    eids, edists, _ = oracle_subset(corpus, query, K, allow)
    monkeypatch.setenv("SDBV_FILTER_PREFILTER", "0")
    gids, gdists = ctx.knn_bruteforce_filtered(TABLE, query, K, allow)
    assert ctx.stats()["last_scan_path"] == 7
    assert np.array_equal(gids, eids)
    assert np.array_equal(bits(gdists), bits(edists))


def test_candidate_overflow_reruns_the_masked_scan(ctx, query):
    """The overflow corpus of test_gpu_prefilter_l2.py under an all-ones
    mask: every row is a candidate, the masked scan answers."""
    n, d, k = 20000, 16, 10
    base = oracle.gen_f32(0x51, 0, 1, d)[0]
    u = np.random.default_rng(5).uniform(-1.0, 1.0, size=(n, d))
    rows = (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)
    q = oracle.gen_f32(0x53, 0, 1, d)[0]
    ctx.stage_corpus(TABLE + 1, rows, metric="euclidean")
    ctx.table_set_prefilter_l2(TABLE + 1, True)
    gids, gdists = ctx.knn_bruteforce_filtered(TABLE + 1, q, k,
                                               np.ones(n, bool))
    st = ctx.stats()
    assert st["last_scan_path"] == PATH_FILTERED_OVERFLOW
    assert st["last_prefilter_candidates"] == n
    oids, odists = oracle.topk_f32("euclidean", rows, q, k)
    assert np.array_equal(gids, oids)
    assert np.array_equal(bits(gdists), bits(odists))
    ctx.drop_table(TABLE + 1)
