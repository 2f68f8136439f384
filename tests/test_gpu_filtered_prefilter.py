"""Filtered brute-force KNN on a shadowed cosine table: the prefilter shadow
streamed under the allowed-row bitmap, on all three tiers.

The expected value is the CPU oracle on the allowed subset, as in
test_gpu_filtered.py; where rows have NaN or infinite distances it is the
same call with SDBV_FILTER_PREFILTER=0 (the masked exact scan, path 7). Every
comparison is exact equality of ids and of distance bits, and every case
asserts which path ran (stats last_scan_path: 9 / 11 / 13 the bf16 / int8 /
int6 shadow under a filter, 10 / 12 / 14 the same after a candidate overflow
and the masked scan).

SDBV_FILTER_ROWLIST_MAX=0 and SDBV_FILTER_PREFILTER_MIN_ROWS=0 bring the path
down to shapes of a few thousand rows: the tiers sweep 2048-row (bf16, int6)
and 4096-row (int8) tiles, a wave covers 512, 1024 and 64 rows of the
bitmap."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_CAND_CAP = 16384
PATH_MASKED, PATH_LIST = 7, 8
ROWLIST, PREFILTER, MIN_ROWS = ("SDBV_FILTER_ROWLIST_MAX",
                                "SDBV_FILTER_PREFILTER",
                                "SDBV_FILTER_PREFILTER_MIN_ROWS")

# tier -> (shadow kind, path under a filter, path of the unfiltered call)
TIERS = {"bf16": (1, 9, 1), "int8": (2, 11, 3), "int6": (3, 13, 5)}


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


@contextlib.contextmanager
def env(rowlist="0", prefilter=None, min_rows="0"):
    """Set the three variables of the filtered call (None = unset), then
    restore. The defaults reach the shadow path at any shape."""
    want = {ROWLIST: rowlist, PREFILTER: prefilter, MIN_ROWS: min_rows}
    old = {name: os.environ.get(name) for name in want}
    try:
        for name, value in want.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = str(value)
        yield
    finally:
        for name, value in old.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


def set_tier(ctx, table, tier):
    kind = TIERS[tier][0]
    if kind == 3:
        ctx.table_set_prefilter_i6(table)
    else:
        ctx.table_set_prefilter_kind(table, kind)


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


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


_expected = {}


def expected(key, corpus, q, k, allow):
    """Oracle top-k on the allowed subset, computed once per key and shared
    by the three tiers: (ids, dists, allowed-row count)."""
    if key not in _expected:
        rows = np.flatnonzero(allow)
        if rows.size == 0:
            _expected[key] = (np.empty(0, np.uint64), np.empty(0, np.float64),
                              0)
        else:
            oids, odists = oracle.topk_f32(
                "cosine", np.ascontiguousarray(corpus[rows]), q, k)
            _expected[key] = (rows[oids.astype(np.int64)].astype(np.uint64),
                              odists, rows.size)
    return _expected[key]


def run_filtered(ctx, table, q, k, allow):
    gids, gdists = ctx.knn_bruteforce_filtered(table, q, k, allow)
    return gids.copy(), gdists.copy(), ctx.stats()


def assert_equal(got, want_ids, want_dists, what):
    assert np.array_equal(got[0], want_ids), (
        f"{what}: ids {got[0]} != {want_ids}")
    assert np.array_equal(bits(got[1]), bits(want_dists)), (
        f"{what}: distance bits differ")


def check_shadow_path(ctx, table, tier, key, corpus, q, k, allow):
    """One filtered call on the shadow path: the tier's odd path, the
    counters, and the oracle's ids and bits."""
    eids, edists, count = expected(key, corpus, q, k, allow)
    with env():
        got = run_filtered(ctx, table, q, k, allow)
    st = got[2]
    print(f"{tier} {key}: allowed {count}, candidates "
          f"{st['last_prefilter_candidates']}, path {st['last_scan_path']}")
    assert st["last_scan_path"] == TIERS[tier][1]
    assert st["last_filter_rows"] == count
    assert st["last_rows_scanned"] == count
    assert min(k, count) <= st["last_prefilter_candidates"] <= count
    assert got[0].size == min(k, count)
    assert_equal(got, eids, edists, f"{tier} {key}")
    return got


# ---- random masks -----------------------------------------------------------

@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("n,d,k", [(999, 20, 10), (5000, 128, 10),
                                   (3000, 768, 64)])
@pytest.mark.parametrize("p", [0.5, 0.02])
def test_random_masks(ctx, tier, n, d, k, p):
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(n + int(p * 100)).random(n) < p
    if p == 0.02 and k == 64:
        assert allow.sum() < k  # fewer allowed rows than k: U_K = +inf
    ctx.stage_corpus(60, corpus, metric="cosine")
    set_tier(ctx, 60, tier)
    check_shadow_path(ctx, 60, tier, ("random", n, d, k, p), corpus, q, k,
                      allow)
    ctx.drop_table(60)


# ---- edge masks at n = 5000, d = 32 -------------------------------------------

EDGE_N, EDGE_D, EDGE_K = 5000, 32, 10


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
    a[2048:4096] = False
    m["rows_2048_4095_clear"] = a
    a = np.random.default_rng(5).random(n) < 0.5
    a[1024:1088] = False
    a[1088:1152] = True
    m["word_clear_then_word_full"] = a
    a = np.zeros(n, bool)
    rng = np.random.default_rng(6)
    for s in range(0, n, 64):
        a[s + int(rng.integers(0, min(64, n - s)))] = True
    m["one_row_per_64"] = a
    a = np.zeros(n, bool)
    a[[3, 2500, 4999]] = True
    m["fewer_than_k"] = a
    return m


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("name", sorted(edge_masks()))
def test_edge_masks(ctx, tier, name):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    allow = edge_masks()[name]
    ctx.stage_corpus(61, corpus, metric="cosine")
    set_tier(ctx, 61, tier)
    got = check_shadow_path(ctx, 61, tier, ("edge", name), corpus, q, EDGE_K,
                            allow)
    if name == "fewer_than_k":
        assert got[0].size == 3
        assert np.all(np.diff(got[1]) >= 0)
    ctx.drop_table(61)


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_all_ones_equals_unfiltered(ctx, tier):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    ctx.stage_corpus(61, corpus, metric="cosine")
    set_tier(ctx, 61, tier)
    uids, udists = ctx.knn_bruteforce(61, q, EDGE_K)
    assert ctx.stats()["last_scan_path"] == TIERS[tier][2]
    got = check_shadow_path(ctx, 61, tier, ("edge", "all_ones"), corpus, q,
                            EDGE_K, np.ones(EDGE_N, bool))
    assert_equal(got, uids, udists, "all ones against the unfiltered call")
    ctx.drop_table(61)


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_all_zeros(ctx, tier):
    corpus = corpus_of(0x5DB1, EDGE_N, EDGE_D)
    q = query_of(0xBEEF, EDGE_D)
    ctx.stage_corpus(61, corpus, metric="cosine")
    set_tier(ctx, 61, tier)
    with env():
        gids, gdists, st = run_filtered(ctx, 61, q, EDGE_K,
                                        np.zeros(EDGE_N, bool))
    assert gids.size == 0 and gdists.size == 0
    assert st["last_filter_rows"] == 0
    ctx.drop_table(61)


# ---- stale scores -------------------------------------------------------------

@pytest.mark.parametrize("tier", sorted(TIERS))
def test_stale_scores_make_no_candidates(ctx, tier):
    """Two calls on one table with complementary masks. The first allows the
    unfiltered top-100 rows (plus noise) and leaves their scores, the best
    of the table, in the score scratch; the second disallows them. Rows
    2048..4095 are all allowed in the first call and all disallowed in the
    second, so the second call's waves skip their loads there on every
    tier and still have to overwrite those scores."""
    n, d, k = EDGE_N, EDGE_D, EDGE_K
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    top = oracle.topk_f32("cosine", corpus, q, 100)[0].astype(np.int64)
    first = np.random.default_rng(21).random(n) < 0.3
    first[2048:4096] = True  # second call: whole waves without a live row
    first[top] = True
    second = ~first
    ctx.stage_corpus(62, corpus, metric="cosine")
    set_tier(ctx, 62, tier)
    check_shadow_path(ctx, 62, tier, ("stale", "first"), corpus, q, k, first)
    got = check_shadow_path(ctx, 62, tier, ("stale", "second"), corpus, q, k,
                            second)
    assert not np.intersect1d(got[0].astype(np.int64), top).size
    ctx.drop_table(62)


# ---- rows the bound cannot cover ------------------------------------------------

UNSAFE_ROWS = [3, 9, 10, 11, 12, 13]


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
    corpus[16] = 2.5                     # constant row
    corpus[17] = 1e-3                    # one dominant element
    corpus[17, 6] = -50.0
    corpus[n - 1, d - 1] = np.nan
    return corpus


def unsafe_masks(n):
    unsafe = UNSAFE_ROWS + [n - 1]
    m = {}
    a = np.random.default_rng(31).random(n) < 0.5
    a[unsafe] = True
    m["unsafe_allowed"] = a
    a = a.copy()
    a[unsafe] = False
    m["unsafe_disallowed"] = a
    a = np.zeros(n, bool)
    a[unsafe] = True
    a[[14, 1500, 2998]] = True
    m["unsafe_plus_three"] = a
    return m


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("name", sorted(unsafe_masks(3000)))
def test_uncovered_rows(ctx, tier, name):
    """Allowed rows without a bound (-inf scores) always reach the exact
    stage; disallowed ones (NaN scores) never do, whatever they hold. The
    reference is the masked exact scan on the same table."""
    n, d, k = 3000, 32, 10
    corpus = unsafe_corpus(n, d)
    q = oracle.gen_f32(0x62, 0, 1, d)[0]
    allow = unsafe_masks(n)[name]
    ctx.stage_corpus(63, corpus, metric="cosine")
    set_tier(ctx, 63, tier)
    with env(prefilter="0"):
        ref = run_filtered(ctx, 63, q, k, allow)
    assert ref[2]["last_scan_path"] == PATH_MASKED
    with env():
        got = run_filtered(ctx, 63, q, k, allow)
    st = got[2]
    assert st["last_scan_path"] == TIERS[tier][1]
    assert st["last_filter_rows"] == allow.sum()
    assert st["last_prefilter_candidates"] >= min(k, allow.sum())
    assert_equal(got, ref[0], ref[1], f"{tier} {name}")
    if name == "unsafe_disallowed":
        assert not np.intersect1d(got[0].astype(np.int64),
                                  UNSAFE_ROWS + [n - 1]).size
    ctx.drop_table(63)


# ---- overflow is counted on allowed rows ----------------------------------------

OVF_N, OVF_D, OVF_K = 20000, 16, 10


@functools.lru_cache(maxsize=None)
def near_duplicates():
    """Rows equal to one vector times (1 + 1e-4 u), u in [-1, 1): far below
    every tier's resolution, so every allowed row is a candidate."""
    base = oracle.gen_f32(0x51, 0, 1, OVF_D)[0]
    u = np.random.default_rng(5).uniform(-1.0, 1.0, size=(OVF_N, OVF_D))
    corpus = (base[None, :].astype(np.float64) * (1.0 + 1e-4 * u)).astype(
        np.float32)
    corpus.setflags(write=False)
    return corpus


@pytest.mark.parametrize("tier", sorted(TIERS))
@pytest.mark.parametrize("allowed", [19990, 10000])
def test_overflow_counts_allowed_rows(ctx, tier, allowed):
    corpus = near_duplicates()
    q = query_of(0x53, OVF_D)
    allow = np.zeros(OVF_N, bool)
    allow[np.random.default_rng(allowed).permutation(OVF_N)[:allowed]] = True
    eids, edists, count = expected(("overflow", allowed), corpus, q, OVF_K,
                                   allow)
    assert count == allowed
    ctx.stage_corpus(64, corpus, metric="cosine")
    set_tier(ctx, 64, tier)
    with env():
        got = run_filtered(ctx, 64, q, OVF_K, allow)
    st = got[2]
    overflowed = allowed > PF_CAND_CAP
    assert st["last_scan_path"] == TIERS[tier][1] + (1 if overflowed else 0)
    assert st["last_prefilter_candidates"] == allowed
    assert st["last_filter_rows"] == allowed
    assert st["last_rows_scanned"] == allowed
    assert_equal(got, eids, edists, f"{tier} {allowed} allowed")
    ctx.drop_table(64)


# ---- fall-throughs keep path 7 (or 8) -------------------------------------------

def test_fall_throughs(ctx):
    n, d, k = EDGE_N, EDGE_D, EDGE_K
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(41).random(n) < 0.5
    eids, edists, count = expected(("fall", "half"), corpus, q, k, allow)

    def check(path, query=q, want=None, **kw):
        with env(**kw):
            got = run_filtered(ctx, 65, query, k, allow)
        assert got[2]["last_scan_path"] == path
        assert got[2]["last_prefilter_candidates"] == 0
        assert got[2]["last_filter_rows"] == count
        w = (eids, edists) if want is None else want
        assert_equal(got, w[0], w[1], f"fall-through {kw}")
        return got

    zero = np.zeros(d, np.float32)
    nanq = np.array(q)
    nanq[7] = np.nan
    # a cosine table without a shadow: also the reference for the two
    # queries outside the norm window
    ctx.stage_corpus(65, corpus, metric="cosine")
    check(PATH_MASKED)
    with env():
        want_zero = run_filtered(ctx, 65, zero, k, allow)[:2]
        want_nan = run_filtered(ctx, 65, nanq, k, allow)[:2]
    for tier in sorted(TIERS):
        set_tier(ctx, 65, tier)
        check(PATH_MASKED, prefilter="0")
        check(PATH_MASKED, min_rows=None)  # default: 500000 rows
        check(PATH_MASKED, min_rows=str(n + 1))
        check(PATH_MASKED, query=zero, want=want_zero)
        check(PATH_MASKED, query=nanq, want=want_nan)
        # the row list keeps priority at its default cap
        check(PATH_LIST, rowlist=None)
        # and the shadow path is there when nothing holds it back
        with env():
            assert run_filtered(ctx, 65, q, k, allow)[2][
                "last_scan_path"] == TIERS[tier][1]
    ctx.drop_table(65)

    # a euclidean table has no shadow and never leaves path 7
    oids, odists = oracle.topk_f32(
        "euclidean", np.ascontiguousarray(corpus[np.flatnonzero(allow)]), q, k)
    ctx.stage_corpus(65, corpus, metric="euclidean")
    check(PATH_MASKED, want=(np.flatnonzero(allow)[oids.astype(np.int64)]
                             .astype(np.uint64), odists))
    ctx.drop_table(65)


# ---- no scratch shared by accident ------------------------------------------------

@pytest.mark.parametrize("tier", sorted(TIERS))
def test_unfiltered_call_before_and_after(ctx, tier):
    n, d, k = EDGE_N, EDGE_D, EDGE_K
    corpus = corpus_of(0x5DB1, n, d)
    q = query_of(0xBEEF, d)
    allow = np.random.default_rng(42).random(n) < 0.5
    oids, odists = oracle.topk_f32("cosine", corpus, q, k)
    ctx.stage_corpus(66, corpus, metric="cosine")
    set_tier(ctx, 66, tier)
    for _ in range(2):  # unfiltered, filtered, unfiltered, filtered
        uids, udists = ctx.knn_bruteforce(66, q, k)
        st = ctx.stats()
        assert st["last_scan_path"] == TIERS[tier][2]
        assert st["last_rows_scanned"] == n
        assert_equal((uids, udists), oids, odists, "unfiltered")
        check_shadow_path(ctx, 66, tier, ("order", "half"), corpus, q, k,
                          allow)
    uids, udists = ctx.knn_bruteforce(66, q, k)
    assert ctx.stats()["last_scan_path"] == TIERS[tier][2]
    assert_equal((uids, udists), oids, odists, "unfiltered, last")
    ctx.drop_table(66)
