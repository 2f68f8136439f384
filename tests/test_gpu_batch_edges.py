"""Where the batched-query path could be wrong without test_gpu_batch.py
noticing: near-duplicate rows that tie in the f32 selection key, rows and
queries without a usable key, the candidate-overflow refold, the fused MFMA
kernel's tile edges and the legacy pass's.

Finite inputs are held to the oracle (ids equal, distance bits equal).
Non-finite ones are held to the single-query scan of the same staged table,
as in the prefilter tests: the CPU and the device disagree on NaN signs.
Every case also requires the ids of a query to be pairwise distinct."""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PAD = np.iinfo(np.uint64).max
FUSED0 = 65536        # first row of the fused kernel's range
CAND_CAP = 4096       # its per-query candidate buffer
SLACK = 16            # window = k + SLACK rows
SDBV_ERR_BAD_ARG = -3


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_distinct(ids):
    for j, row in enumerate(np.atleast_2d(ids)):
        real = row[row != PAD]
        assert np.unique(real).size == real.size, f"q{j}: duplicate ids {row}"


def assert_oracle(metric, corpus, Q, k, ids, dists, queries, id_map=None):
    for j in queries:
        oids, odists = oracle.topk_f32(metric, corpus, Q[j], k)
        if id_map is not None:
            oids = id_map[oids.astype(np.int64)]
        m = oids.size
        assert np.array_equal(ids[j][:m], oids), f"{metric} q{j}: ids"
        assert np.array_equal(bits(dists[j][:m]), bits(odists)), \
            f"{metric} q{j}: distance bits"
        assert (ids[j][m:] == PAD).all() and np.isinf(dists[j][m:]).all()


def assert_single(ctx, table, Q, k, ids, dists, queries):
    """Against sdbv_knn_bruteforce on the same staged table."""
    for j in queries:
        sids, sdists = ctx.knn_bruteforce(table, Q[j], k)
        m = sids.size
        assert np.array_equal(ids[j][:m], sids), f"q{j}: ids {ids[j]} {sids}"
        assert np.array_equal(bits(dists[j][:m]), bits(sdists)), \
            f"q{j}: distance bits"
        assert (ids[j][m:] == PAD).all()


def batch(ctx, table, Q, k, legacy=False):
    """(ids, dists, exact-scan queries, refold) of one knn_batch call."""
    if legacy:
        os.environ["SDBV_BATCH_LEGACY"] = "1"
    try:
        ids, dists = ctx.knn_batch(table, Q, k)
    finally:
        if legacy:
            del os.environ["SDBV_BATCH_LEGACY"]
    st = ctx.stats()
    assert_distinct(ids)
    return ids, dists, st["last_batch_exact_queries"], st["last_batch_refold"]


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------------------
# 1. near-tie clusters
# ---------------------------------------------------------------------------
M_CLUSTER = 200


def ulp_cluster(q, step):
    """M rows = q -+ (M - i) * step ulps per element, signs alternating along
    the features: the last row is the nearest."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    qb = q.view(np.int32).astype(np.int64)
    sign = np.where(np.arange(q.size) % 2 == 0, 1, -1)
    rows = np.empty((M_CLUSTER, q.size), dtype=np.float32)
    for i in range(M_CLUSTER):
        # stepping the bit pattern moves the magnitude by whole ulps
        rows[i] = (qb + sign * (M_CLUSTER - i) * step).astype(
            np.int32).view(np.float32)
    return rows


def cluster_spread(metric, q, rows):
    """(largest spread of the cluster in the key's domain, the key's
    magnitude there), in f64: exact squared distance for euclidean (key about
    -|q|^2), |q| (1 - cos) for cosine (key about -|q|)."""
    q64, r64 = q.astype(np.float64), rows.astype(np.float64)
    qn = np.sqrt((q64 * q64).sum())
    if metric == "euclidean":
        return ((r64 - q64) ** 2).sum(axis=1).max(), qn * qn
    cos = (r64 @ q64) / (np.sqrt((r64 * r64).sum(axis=1)) * qn)
    return (qn * (1.0 - cos)).max(), qn


def near_tie_case(metric, n, d, b, planted):
    corpus = oracle.gen_f32(0x71E, 0, n, d)
    Q = oracle.gen_f32(0x71F, 0, b, d)
    # One-ulp steps for both metrics; the alternating signs make the
    # directions differ. A wider step for cosine breaks the precondition
    # below: at 4x the spread (2.1e-7 at d = 32) is only 35x below the key's
    # ulp, at 2x it is 90x below for a query norm under 64.
    step = 1
    for i, j in enumerate(planted):
        rows = ulp_cluster(Q[j], step)
        spread, mag = cluster_spread(metric, Q[j], rows)
        # far inside one ulp of the key: whatever the summation order, the
        # key cannot tell the cluster's rows apart, so their order in the
        # window is the row order, farthest first
        print(f"{metric} d={d} q{j}: spread {spread:.3e}, key ulp "
              f"{ulp32(mag):.3e}")
        assert spread * 100 <= ulp32(mag)
        hi = n - i * M_CLUSTER
        corpus[hi - M_CLUSTER:hi] = rows
    return corpus, Q


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", [32, 64])
def test_near_tie_cluster_legacy(ctx, metric, d):
    """200 near-duplicates of a query, nearest at the highest rows: more
    rows tie in the key than the window holds, so the window alone keeps the
    farthest of them."""
    n, b, k, planted = 3000, 7, 10, (1, 4)
    corpus, Q = near_tie_case(metric, n, d, b, planted)
    ctx.stage_corpus(31, corpus, metric=metric)
    ids, dists, nexact, refold = batch(ctx, 31, Q, k)
    ctx.drop_table(31)
    assert_oracle(metric, corpus, Q, k, ids, dists, range(b))
    # the planted queries cannot be certified (another query may have a
    # whole cluster at its window's edge and go the same way)
    assert nexact >= len(planted) and refold == 0


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", [32, 64])
def test_near_tie_cluster_fused(ctx, metric, d):
    n, b, k, planted = FUSED0 + 4096, 128, 10, (3, 77)
    corpus, Q = near_tie_case(metric, n, d, b, planted)
    ctx.stage_corpus(31, corpus, metric=metric)
    ids, dists, nexact, refold = batch(ctx, 31, Q, k)
    ctx.drop_table(31)
    assert_oracle(metric, corpus, Q, k, ids, dists,
                  sorted(set(range(0, b, 13)) | set(planted)))
    assert nexact >= len(planted) and refold == 0


# ---------------------------------------------------------------------------
# 2. hostile rows and queries
# ---------------------------------------------------------------------------
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]


def hostile_block(corpus, r0):
    """The prefilter tests' block of rows no bound covers, from row r0."""
    d = corpus.shape[1]
    corpus[r0 + 3] = 0.0                 # zero norm
    corpus[r0 + 9, 2] = np.nan
    corpus[r0 + 10, 0] = np.inf
    corpus[r0 + 11, 5] = -np.inf
    corpus[r0 + 12, 1] = 3e38            # finite, the norm overflows
    corpus[r0 + 13] = 1e-40              # all subnormal: the norm underflows
    corpus[r0 + 14, 4] = 1e-40           # one subnormal element: a safe row
    corpus[r0 + 15] = -corpus[r0 + 15]
    corpus[r0 + 17] = 1e-3               # one dominant element
    corpus[r0 + 17, 6] = -50.0
    corpus[-1, d - 1] = np.nan           # last row, last feature


def hostile_corpus(n, d, variant, fused):
    corpus = oracle.gen_f32(0x61, 0, n, d)
    r0 = FUSED0 + 100 if fused else 0
    hostile_block(corpus, r0)
    if fused:
        hostile_block(corpus, 500)       # the bootstrap range as well
    many = 48 + SLACK + 4                # kk + 4 at the largest k
    if variant == "zeros":
        corpus[r0 + 40:r0 + 40 + many] = 0.0
    elif variant == "nans":
        corpus[r0 + 40:r0 + 40 + many, 1] = np.nan
    elif variant == "negnan":
        corpus[r0 + 40, 7] = NEG_NAN
    return corpus


HOSTILE_SHAPES = [(3000, 7, False), (FUSED0 + 4096, 128, True)]


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("variant", ["zeros", "nans", "negnan"])
@pytest.mark.parametrize("n,b,fused", HOSTILE_SHAPES)
def test_hostile_rows(ctx, metric, variant, n, b, fused):
    """Rows without a usable key (a zero row's cosine key is 0 * inf = NaN,
    of either sign) neither crowd the real neighbours out of the window nor
    get lost to it: every query equals the single-query scan."""
    d = 32
    corpus = hostile_corpus(n, d, variant, fused)
    Q = oracle.gen_f32(0x62, 0, b, d)
    Q[2] = corpus[(FUSED0 + 100 if fused else 0) + 17]   # dominant element
    ctx.stage_corpus(32, corpus, metric=metric)
    queries = sorted(set(range(0, b, 9)) | {2, b - 1})
    for k in (1, 10, 48):
        ids, dists, nexact, refold = batch(ctx, 32, Q, k)
        assert_single(ctx, 32, Q, k, ids, dists, queries)
        assert refold == 0
        # hostile rows do not send ordinary queries to the exact scan
        # (euclidean zero rows have a key: 68 of them at one distance can
        # tie across a window's edge, which then cannot be certified)
        if not (metric == "euclidean" and variant == "zeros"):
            assert nexact == 0
    ctx.drop_table(32)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,b,fused", HOSTILE_SHAPES)
def test_hostile_queries(ctx, metric, n, b, fused):
    """Zero, NaN, infinite, huge and tiny queries among ordinary ones: each
    query's rows of the output equal the single-query scan's."""
    d = 32
    corpus = hostile_corpus(n, d, "negnan", fused)
    Q = oracle.gen_f32(0x63, 0, b, d)
    bad = {0: 0.0, 2: None, 3: np.inf, 4: -np.inf, 5: 1e30, b - 1: 1e-30}
    for j, v in bad.items():
        if v is None:
            Q[j, 7] = np.nan
        elif np.isinf(v):
            Q[j, 0] = v
        elif v == 0.0:
            Q[j] = 0.0
        else:
            Q[j] = Q[j] * np.float32(v / 10.0)
    ctx.stage_corpus(32, corpus, metric=metric)
    queries = sorted(set(range(0, b, 9)) | set(bad) | {1, 6})
    for k in (1, 10, 48):
        ids, dists, nexact, refold = batch(ctx, 32, Q, k)
        assert_single(ctx, 32, Q, k, ids, dists, queries)
        assert nexact >= len(bad) and refold == 0
        # ... and no more than the bad ones: the others keep the window
        assert nexact == len(bad)
    ctx.drop_table(32)


# ---------------------------------------------------------------------------
# 3. candidate-overflow refold
# ---------------------------------------------------------------------------
def ramp_case(metric, extra):
    """Uniform bootstrap rows, then `extra` rows on a ramp towards query 0,
    nearest last, that all beat its bootstrapped threshold: query 0 appends
    exactly `extra` candidates in the fused kernel."""
    b, d = 128, 32
    n = FUSED0 + extra
    corpus = oracle.gen_f32(0x0F1, 0, n, d)
    Q = oracle.gen_f32(0x0F2, 0, b, d)
    rng = np.random.default_rng(3)
    w = rng.standard_normal(d)
    q64 = Q[0].astype(np.float64)
    w -= q64 * (w @ q64) / (q64 @ q64)   # across the query: changes the angle
    w /= np.sqrt(w @ w)
    # squared distance 1000 down to 10, evenly spaced: noise of scale ~1 per
    # element that shrinks with the row index
    a = np.sqrt(np.linspace(1000.0, 10.0, extra))
    corpus[FUSED0:] = (q64[None, :] + a[:, None] * w[None, :]).astype(
        np.float32)
    # the reverse of the near-tie precondition: neighbouring rows of the
    # ramp are far more than an ulp of the key apart, so ties play no part
    r64 = corpus[FUSED0:].astype(np.float64)
    qn = np.sqrt(q64 @ q64)
    if metric == "euclidean":
        e = ((r64 - q64) ** 2).sum(axis=1)
        mag = qn * qn
    else:
        e = -qn * (r64 @ q64) / (np.sqrt((r64 * r64).sum(axis=1)) * qn)
        mag = qn
    gaps = e[:-1] - e[1:]
    print(f"{metric} extra={extra}: smallest gap {gaps.min():.3e}, key ulp "
          f"{ulp32(mag):.3e}")
    assert gaps.min() >= 100 * ulp32(mag)
    # all of them beat anything the uniform bootstrap rows offer
    boot = corpus[:FUSED0].astype(np.float64)
    if metric == "euclidean":
        assert e.max() < ((boot - q64) ** 2).sum(axis=1).min()
    else:
        bk = -(boot @ q64) / np.sqrt((boot * boot).sum(axis=1))
        assert e.max() < bk.min()
    return corpus, Q


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("extra", [257, 1025, 1500, CAND_CAP])
def test_fold_many_candidates(ctx, metric, extra):
    """More candidates than one thread each (256), than one fold tile (1024)
    and a full buffer, nearest last: the fold has to read every one of them.
    The flagship batch shape appends about 1200 per query."""
    k = 10
    corpus, Q = ramp_case(metric, extra)
    ctx.stage_corpus(33, corpus, metric=metric)
    ids, dists, nexact, refold = batch(ctx, 33, Q, k)
    ctx.drop_table(33)
    assert_oracle(metric, corpus, Q, k, ids, dists, range(Q.shape[0]))
    assert nexact == 0 and refold == 0


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_overflow_refold(ctx, metric):
    """5000 rows of the fused range beat query 0's bootstrapped threshold,
    nearest last: its 4096-slot candidate buffer overflows and the selection
    is redone through the legacy pass, for every query, without taking a
    row twice."""
    b, k, extra = 128, 10, 5000
    assert extra > CAND_CAP
    corpus, Q = ramp_case(metric, extra)
    ctx.stage_corpus(33, corpus, metric=metric)
    ids, dists, nexact, refold = batch(ctx, 33, Q, k)
    assert_oracle(metric, corpus, Q, k, ids, dists, range(b))
    assert refold == 1
    assert nexact == 0       # the window answers: this is the refold's result
    lids, ldists, lexact, lrefold = batch(ctx, 33, Q, k, legacy=True)
    assert lrefold == 0 and lexact == 0
    assert np.array_equal(ids, lids) and np.array_equal(bits(dists),
                                                        bits(ldists))
    ctx.drop_table(33)


# ---------------------------------------------------------------------------
# 4. fused-kernel tile edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("b,d", [(128, 32), (256, 32), (256, 64)])
def test_fused_tile_edges(ctx, metric, b, d):
    """One, 128 and 129 fused rows; one K stage (d = 32) and two; a second
    column block (b = 256); k = 1 and the full window (k = 48). Exact best
    matches sit at the first fused row and at the last row, for a query of
    each column block."""
    jlo, jhi = 5, b - 6                    # 250: second column block
    Q = oracle.gen_f32(0xED2, 0, b, d)
    base = oracle.gen_f32(0xED1, 0, FUSED0 + 129, d)
    for n in (FUSED0 + 1, FUSED0 + 128, FUSED0 + 129):
        corpus = base[:n].copy()
        if n == FUSED0 + 1:
            corpus[FUSED0 - 1] = Q[jlo]    # last bootstrap row
            corpus[FUSED0] = Q[jhi]        # the only fused row
            best = {jlo: FUSED0 - 1, jhi: FUSED0}
        else:
            corpus[FUSED0] = Q[jlo]
            corpus[n - 1] = Q[jhi]
            best = {jlo: FUSED0, jhi: n - 1}
        ctx.stage_corpus(34, corpus, metric=metric)
        queries = sorted({0, jlo, 127, b - 128, jhi, b - 1})
        for k in (1, 10, 48):
            ids, dists, nexact, refold = batch(ctx, 34, Q, k)
            assert nexact == 0 and refold == 0
            for j, row in best.items():
                assert ids[j][0] == row
            assert_oracle(metric, corpus, Q, k, ids, dists, queries)
            lids, ldists, lexact, lrefold = batch(ctx, 34, Q, k, legacy=True)
            assert lexact == 0 and lrefold == 0
            assert np.array_equal(ids, lids), f"n={n} k={k}: fused != legacy"
            assert np.array_equal(bits(dists), bits(ldists))
        ctx.drop_table(34)


def test_fused_explicit_ids(ctx):
    b, d, k, n = 128, 32, 10, FUSED0 + 129
    corpus = oracle.gen_f32(0xED3, 0, n, d)
    Q = oracle.gen_f32(0xED4, 0, b, d)
    corpus[n - 1] = Q[9]
    id_map = (7 * np.arange(n) + 100).astype(np.uint64)
    ctx.stage_corpus(34, corpus, ids=id_map, metric="euclidean")
    ids, dists, nexact, refold = batch(ctx, 34, Q, k)
    ctx.drop_table(34)
    assert nexact == 0 and refold == 0
    assert ids[9][0] == 7 * (n - 1) + 100
    assert_oracle("euclidean", corpus, Q, k, ids, dists, range(0, b, 8),
                  id_map=id_map)


# ---------------------------------------------------------------------------
# 5. legacy-pass edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("n,d,b,k", [
    (500, 4, 1, 5),        # b = 1; d < 8: only the chain's tail loop
    (500, 12, 3, 5),       # one unrolled step and a four-element tail
    (500, 20, 3, 5),       # two steps and the tail
    (1, 16, 3, 4),         # a single row
    (1023, 16, 1, 10),     # one row short of the select tile
    (1024, 16, 5, 48),     # exactly one tile, the full window
    (1025, 16, 5, 1),      # one row past it
])
def test_legacy_edges(ctx, metric, n, d, b, k):
    """Staging takes d % 4 == 0 only, so the tails of the 8-way chain that
    can be reached are the four-element ones (d = 4, 12, 20)."""
    corpus = oracle.gen_f32(0x1E6, 0, n, d)
    Q = oracle.gen_f32(0x1E7, 0, b, d)
    ctx.stage_corpus(35, corpus, metric=metric)
    ids, dists, nexact, refold = batch(ctx, 35, Q, k)
    ctx.drop_table(35)
    assert refold == 0
    print(f"{metric} n={n} d={d} b={b} k={k}: exact-scan queries {nexact}")
    assert_oracle(metric, corpus, Q, k, ids, dists, range(b))


@pytest.mark.parametrize("d", [1, 7, 9])
def test_unstageable_dims_are_bad_arg(ctx, d):
    """d = 1, 7, 9 would be the chain's other tails, but no table of such a
    dimension exists: staging rejects it, so no batch call can see one."""
    import surrealdb_amd
    corpus = oracle.gen_f32(0x1E6, 0, 50, d)
    with pytest.raises(surrealdb_amd.SdbvError, match="bad argument"):
        ctx.stage_corpus(35, corpus, metric="euclidean")


def test_legacy_second_gemm_chunk(ctx):
    """The best match in the second 262144-row GEMM chunk, 5 rows long."""
    n, d, b, k = 262144 + 5, 32, 4, 10
    corpus = oracle.gen_f32(0x1E8, 0, n, d)
    Q = oracle.gen_f32(0x1E9, 0, b, d)
    corpus[262144 + 2] = Q[1]
    corpus[n - 1] = Q[3]
    ctx.stage_corpus(35, corpus, metric="euclidean")
    ids, dists, nexact, refold = batch(ctx, 35, Q, k)
    ctx.drop_table(35)
    assert nexact == 0 and refold == 0
    assert ids[1][0] == 262144 + 2 and ids[3][0] == n - 1
    assert_oracle("euclidean", corpus, Q, k, ids, dists, range(b))


def test_k_above_48_is_bad_arg(ctx):
    import surrealdb_amd
    corpus = oracle.gen_f32(0x1EA, 0, 100, 16)
    Q = oracle.gen_f32(0x1EB, 0, 2, 16)
    ctx.stage_corpus(35, corpus, metric="cosine")
    ids, dists = ctx.knn_batch(35, Q, 48)
    assert_oracle("cosine", corpus, Q, 48, ids, dists, range(2))
    ids = np.empty((2, 49), dtype=np.uint64)
    dists = np.empty((2, 49), dtype=np.float64)
    import ctypes
    rc = surrealdb_amd.lib().sdbv_knn_batch(
        ctx._ptr, 35, Q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2, 16,
        49, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        dists.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    ctx.drop_table(35)
    assert rc == SDBV_ERR_BAD_ARG


def test_scratch_reuse_larger_then_smaller():
    """Two calls of different (b, k) back to back on one fresh context, the
    larger first: the smaller one runs in scratch sized and filled by the
    larger."""
    import surrealdb_amd
    c = surrealdb_amd.Context()
    try:
        n, d = 2000, 24
        corpus = oracle.gen_f32(0x1EC, 0, n, d)
        Q = oracle.gen_f32(0x1ED, 0, 40, d)
        c.stage_corpus(36, corpus, metric="cosine")
        for b, k in ((40, 48), (3, 2)):
            ids, dists, nexact, refold = batch(c, 36, Q[:b], k)
            assert nexact == 0 and refold == 0
            assert_oracle("cosine", corpus, Q[:b], k, ids, dists, range(b))
        c.drop_table(36)
    finally:
        c.close()


def test_flagship_shape_matches_single_query(ctx):
    """The benchmarked batch shape (3M x 768 cosine on-device synthetic rows,
    b = 1024, k = 10): about 1200 candidates per query reach the fold, no
    query needs the exact scan, and the results are the single-query
    scan's."""
    n, d, b, k = 3_000_000, 768, 1024, 10
    ctx.stage_synthetic(37, n, d, metric="cosine", seed=0x5DB1)
    Q = oracle.gen_f32(0xBEEF, 0, b, d)
    ids, dists, nexact, refold = batch(ctx, 37, Q, k)
    assert_single(ctx, 37, Q, k, ids, dists, range(0, b, 93))
    ctx.drop_table(37)
    assert nexact == 0 and refold == 0
