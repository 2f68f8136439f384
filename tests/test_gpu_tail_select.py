"""The kernels behind the single-query streams: the one-pass block select
(k_merge, k_pf_final, the row list's merge), the merge tree's level 2 folded
into k_pf4_threshold, and the exact chain on listed rows — GPU parity.

As in test_gpu_prefilter_h4.py every case compares ids and distance BITS with
the exact scan of the same rows (a shadowless copy staged under
SDBV_SCAN_PREFILTER=0 as table + 100) and with the CPU oracle, and the four
MIN_ROWS variables at 1 bring the shadow tiers down to small tables. Shapes:
the merge tree takes two levels when nblocks * k > 4096 and nblocks > 32; the
two-stage path gives a stream block 256 rows (at most 2048 blocks), the other
tiers 2048, the exact scan 1024. So n = 70 000 runs the two-stage path on 274
blocks (two levels for k = 63 and 64, one for 1 and 10), n = 524 288 with
k = 64 fills all 32 level-1 slices with 4096 entries, and n = 140 000 gives
every tier 69 blocks or more, two levels at k = 64.

Staged ids have to be strictly increasing (SDBV_ERR_IDS_UNSORTED), so the
tie tables carry explicit ids with irregular gaps; ids out of row order are
refused at staging and cannot reach a select."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PF_CAND_CAP = 16384
MIN_ROWS = ("SDBV_SCAN_PREFILTER_MIN_ROWS", "SDBV_SCAN_PREFILTER_I8_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_I6_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_H4_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_L2_MIN_ROWS")
KS = (1, 10, 63, 64)


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
    for name in ("SDBV_SCAN_PREFILTER_H4", "SDBV_SCAN_PREFILTER_H4_LIST_MAX",
                 "SDBV_FILTER_ROWLIST_MAX", "SDBV_FILTER_PREFILTER_MIN_ROWS"):
        monkeypatch.delenv(name, raising=False)


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run(ctx, table, q, k):
    """(ids, dists, path, candidates) of one call."""
    ids, dists = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    return (ids.copy(), dists.copy(), st["last_scan_path"],
            st["last_prefilter_candidates"])


def run_filtered(ctx, table, q, k, allow):
    ids, dists = ctx.knn_bruteforce_filtered(table, q, k, allow)
    return ids.copy(), dists.copy(), ctx.stats()["last_scan_path"]


def stage(ctx, table, corpus, ids=None, metric="cosine"):
    """corpus as table under the forced policy and as table + 100 with no
    shadow."""
    ctx.stage_corpus(table, corpus, ids=ids, metric=metric)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SDBV_SCAN_PREFILTER", "0")
        mp.setenv("SDBV_SCAN_PREFILTER_L2", "0")
        ctx.stage_corpus(table + 100, corpus, ids=ids, metric=metric)


def drop(ctx, table):
    ctx.drop_table(table)
    ctx.drop_table(table + 100)


def run_exact(ctx, table, q, k):
    off = run(ctx, table + 100, q, k)
    assert off[2] == 0 and off[3] == 0
    return off


def assert_same(on, off):
    assert np.array_equal(on[0], off[0]), "ids differ from the exact scan"
    assert np.array_equal(bits(on[1]), bits(off[1])), \
        "distance bits differ from the exact scan"


def assert_oracle(on, corpus, q, k, metric="cosine", ids=None):
    oids, odists = oracle.topk_f32(metric, corpus, q, k)
    if ids is not None:
        oids = ids[oids.astype(np.int64)]
    assert np.array_equal(on[0], oids), "ids differ from the oracle"
    assert np.array_equal(bits(on[1]), bits(odists)), \
        "distance bits differ from the oracle"


# ---------------------------------------------------------------------------
# merge shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(5, 64), (3000, 64), (70_000, 64)])
def test_merge_shapes(ctx, n, d):
    """n = 5: n < k, pads behind the rows. n = 3000: one level (12 blocks).
    n = 70 000: 274 blocks, two levels with slices of 9 * k entries for
    k = 63 and 64."""
    corpus = oracle.gen_f32(0x7A11, 0, n, d)
    q = oracle.gen_f32(0x7A12, 1, 1, d)[0]
    stage(ctx, 61, corpus)
    for k in KS:
        on = run(ctx, 61, q, k)
        off = run_exact(ctx, 61, q, k)
        print(f"n={n} k={k}: path {on[2]}, candidates {on[3]}")
        assert on[2] == 15 and len(on[0]) == min(n, k)
        assert_same(on, off)
        assert_oracle(on, corpus, q, k)
        assert_oracle(off, corpus, q, k)
    drop(ctx, 61)


def test_merge_full_slices(ctx):
    """n = 2048 * 256, k = 64: the two-stage stream runs 2048 blocks (fewer
    on a device with fewer block slots) and every level-1 slice holds the
    full 64 * 64 = 4096 entries; the exact scan of the same rows runs 512
    blocks, 16 to a slice."""
    n, d, k = 2048 * 256, 32, 64
    corpus = oracle.gen_f32(0x7A13, 0, n, d)
    q = oracle.gen_f32(0x7A14, 1, 1, d)[0]
    stage(ctx, 62, corpus)
    on = run(ctx, 62, q, k)
    off = run_exact(ctx, 62, q, k)
    assert on[2] == 15
    assert_same(on, off)
    assert_oracle(on, corpus, q, k)
    drop(ctx, 62)


def test_merge_full_slices_exact_scan(ctx):
    """The exact scan's own full slices: 2048 blocks of 1024 rows, k = 64."""
    n, d, k = 2048 * 1024, 4, 64
    corpus = oracle.gen_f32(0x7A15, 0, n, d)
    q = oracle.gen_f32(0x7A16, 1, 1, d)[0]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SDBV_SCAN_PREFILTER", "0")
        ctx.stage_corpus(163, corpus, metric="cosine")
    off = run(ctx, 163, q, k)
    assert off[2] == 0
    assert_oracle(off, corpus, q, k)
    ctx.drop_table(163)


@pytest.mark.parametrize("k", KS)
def test_merge_pads_reach_the_output(ctx, k):
    """Five rows carry a bound, the others are zero rows: every stream block
    hands pads to the merge, the K smallest upper bounds end in pads for
    k > 5 (the threshold is +inf), and every row reaches the exact stage.
    Zero rows have NaN distances, whose sign the oracle and the device give
    differently: the exact scan is the reference."""
    n, d = 3000, 32
    corpus = np.zeros((n, d), dtype=np.float32)
    keep = np.array([3, 300, 1024, 2047, 2999])
    corpus[keep] = oracle.gen_f32(0x7A17, 0, keep.size, d)
    q = oracle.gen_f32(0x7A18, 1, 1, d)[0]
    stage(ctx, 63, corpus)
    on = run(ctx, 63, q, k)
    assert on[2] == 15
    assert_same(on, run_exact(ctx, 63, q, k))
    drop(ctx, 63)


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
def gap_ids(n):
    """Strictly increasing ids with irregular gaps."""
    step = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)
            >> np.uint64(7)) % np.uint64(9) + np.uint64(1)
    return np.cumsum(step, dtype=np.uint64) + np.uint64(1000)


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("n,path", [(PF_CAND_CAP, 15), (PF_CAND_CAP + 1, 16)])
def test_ties_come_out_in_id_order(ctx, n, path, k):
    """Identical rows: every row passes both tests, so the final select sees
    exactly PF_CAND_CAP candidates of one key (four chunks, the walk on the
    ids alone), or one more: the overflow, which the exact scan serves."""
    d = 8
    row = oracle.gen_f32(0x7A19, 0, 1, d)[0]
    corpus = np.tile(row, (n, 1))
    ids = gap_ids(n)
    q = oracle.gen_f32(0x7A1A, 1, 1, d)[0]
    stage(ctx, 64, corpus, ids=ids)
    on = run(ctx, 64, q, k)
    assert on[2] == path and on[3] == n
    assert np.array_equal(on[0], ids[:k])
    assert np.all(bits(on[1]) == bits(on[1][:1]))
    assert_same(on, run_exact(ctx, 64, q, k))
    assert_oracle(on, corpus, q, k, ids=ids)
    drop(ctx, 64)


def test_ids_out_of_order_are_refused(ctx):
    corpus = oracle.gen_f32(0x7A1B, 0, 4, 8)
    with pytest.raises(Exception):
        ctx.stage_corpus(65, corpus, metric="cosine",
                         ids=np.array([5, 3, 9, 7], dtype=np.uint64))


# ---------------------------------------------------------------------------
# every caller of the shared select, at a two-level shape
# ---------------------------------------------------------------------------
N2, D2, K2 = 140_000, 32, 64


@pytest.fixture(scope="module")
def two_level(ctx):
    """(corpus, q, cosine reference, euclidean reference), the references
    from the oracle, computed once."""
    corpus = oracle.gen_f32(0x7A21, 0, N2, D2)
    q = oracle.gen_f32(0x7A22, 1, 1, D2)[0]
    ref = {m: oracle.topk_f32(m, corpus, q, K2)
           for m in ("cosine", "euclidean")}
    return corpus, q, ref


def assert_ref(got, ref):
    assert np.array_equal(got[0], ref[0]), "ids differ from the oracle"
    assert np.array_equal(bits(got[1]), bits(ref[1])), \
        "distance bits differ from the oracle"


def test_callers_cosine_tiers(ctx, two_level, monkeypatch):
    corpus, q, ref = two_level
    stage(ctx, 66, corpus)
    off = run_exact(ctx, 66, q, K2)                     # the exact scan
    assert_ref(off, ref["cosine"])
    on = run(ctx, 66, q, K2)                            # H-only, two-stage
    assert on[2] == 15
    assert_same(on, off)
    ctx.table_set_prefilter_i6(66)                      # plain int6
    on = run(ctx, 66, q, K2)
    assert on[2] == 5
    assert_same(on, off)
    # the masked stream over the int6 shadow, and the masked exact scan
    monkeypatch.setenv("SDBV_FILTER_ROWLIST_MAX", "0")
    monkeypatch.setenv("SDBV_FILTER_PREFILTER_MIN_ROWS", "0")
    allow = np.ones(N2, dtype=bool)
    allow[::3] = False
    rows = np.flatnonzero(allow)
    oids, odists = oracle.topk_f32("cosine", corpus[rows], q, K2)
    want = (rows[oids.astype(np.int64)].astype(np.uint64), odists)
    got = run_filtered(ctx, 66, q, K2, allow)
    assert got[2] == 13
    assert_ref(got, want)
    got = run_filtered(ctx, 166, q, K2, allow)
    assert got[2] == 7
    assert_ref(got, want)
    monkeypatch.delenv("SDBV_FILTER_ROWLIST_MAX")
    monkeypatch.delenv("SDBV_FILTER_PREFILTER_MIN_ROWS")
    for kind, path in ((2, 3), (1, 1)):                 # int8, bf16
        ctx.table_set_prefilter_kind(66, kind)
        on = run(ctx, 66, q, K2)
        assert on[2] == path
        assert_same(on, off)
    drop(ctx, 66)


def test_callers_l2_tier(ctx, two_level):
    corpus, q, ref = two_level
    stage(ctx, 67, corpus, metric="euclidean")
    ctx.table_set_prefilter_l2(67, True)
    off = run_exact(ctx, 67, q, K2)
    assert_ref(off, ref["euclidean"])
    on = run(ctx, 67, q, K2)
    assert on[2] == 17
    assert_same(on, off)
    drop(ctx, 67)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_callers_row_list(ctx, two_level, metric):
    """k_rows_exact and the single-block merge over cnt = 1, k - 1 and
    16 384 listed rows (four chunks of the select)."""
    corpus, q, _ = two_level
    k = 10
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SDBV_SCAN_PREFILTER", "0")
        mp.setenv("SDBV_SCAN_PREFILTER_L2", "0")
        ctx.stage_corpus(168, corpus, metric=metric)
    rng = np.random.default_rng(0x7A23)
    for cnt in (1, k - 1, PF_CAND_CAP):
        rows = np.sort(rng.choice(N2, size=cnt, replace=False))
        allow = np.zeros(N2, dtype=bool)
        allow[rows] = True
        got = run_filtered(ctx, 168, q, k, allow)
        assert got[2] == 8 and len(got[0]) == min(k, cnt)
        oids, odists = oracle.topk_f32(metric, corpus[rows], q, k)
        assert_ref(got, (rows[oids.astype(np.int64)].astype(np.uint64),
                         odists))
        # the chain of the listed rows is k_gather_dist's, bit for bit
        g = ctx.gather_distance(168, got[0].astype(np.uint32), q)
        assert np.array_equal(bits(g), bits(got[1]))
    ctx.drop_table(168)


# ---------------------------------------------------------------------------
# the threshold fold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [True, False])
def test_threshold_fold(ctx, spread):
    """274 stream blocks of 256 rows, k = 64: two levels, the second folded
    into k_pf4_threshold. The 64 rows next to the query, which have the
    smallest H-only upper bounds by far, lie one in each of 64 blocks (two
    in each level-1 slice that holds any), or all in block 100."""
    n, d, k = 70_000, 64, 64
    corpus = oracle.gen_f32(0x7A31, 0, n, d)
    q = oracle.gen_f32(0x7A32, 1, 1, d)[0]
    near = oracle.gen_f32(0x7A33, 2, k, d)
    planted = (np.arange(k) * 4 * 256 + 5 if spread
               else 100 * 256 + 3 * np.arange(k))
    corpus[planted] = q + np.float32(0.01) * near
    stage(ctx, 68, corpus)
    on = run(ctx, 68, q, k)
    assert on[2] == 15
    assert set(on[0]) == set(planted)
    assert_same(on, run_exact(ctx, 68, q, k))
    assert_oracle(on, corpus, q, k)
    # a tight threshold: the candidates are few
    print(f"spread={spread}: candidates {on[3]}")
    assert on[3] < n // 4
    drop(ctx, 68)


# ---------------------------------------------------------------------------
# the exact-row chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", [4, 8, 12, 20, 44, 768, 4092, 4096])
def test_exact_row_chain(ctx, d, metric):
    """k_rows_exact (the row list) on every row of a small table against the
    exact scan and k_gather_dist, bit for bit. Staging takes multiples of 4
    only (test_odd_dimensions_are_refused), so the tail loop runs 0 or 4
    steps: d = 4 is all tail, 8 has none, 12 one step of eight and the
    tail, 20 and 44 partial sums shorter than a quad and a quad plus one,
    4092 the longest padded staging with a tail, 4096 is MAX_D."""
    n, k = 300, 64
    corpus = oracle.gen_f32(0x7A41, d, n, d)
    q = oracle.gen_f32(0x7A42, d, 1, d)[0]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SDBV_SCAN_PREFILTER", "0")
        mp.setenv("SDBV_SCAN_PREFILTER_L2", "0")
        ctx.stage_corpus(169, corpus, metric=metric)
    off = run(ctx, 169, q, k)
    assert off[2] == 0
    got = run_filtered(ctx, 169, q, k, np.ones(n, dtype=bool))
    assert got[2] == 8
    assert_same(got, off)
    assert_oracle(got, corpus, q, k, metric=metric)
    g = ctx.gather_distance(169, got[0].astype(np.uint32), q)
    assert np.array_equal(bits(g), bits(got[1]))
    ctx.drop_table(169)


@pytest.mark.parametrize("d", [1, 7, 9])
def test_odd_dimensions_are_refused(ctx, d):
    with pytest.raises(Exception):
        ctx.stage_corpus(69, oracle.gen_f32(0x7A45, 0, 16, d),
                         metric="cosine")


@pytest.mark.parametrize("d", [8, 36, 768, 4096])
def test_exact_row_chain_two_stage(ctx, d):
    """The same chain as k_pf4_threshold and k_pf_rescore run it."""
    n, k = 600, 10
    corpus = oracle.gen_f32(0x7A43, d, n, d)
    q = oracle.gen_f32(0x7A44, d, 1, d)[0]
    stage(ctx, 70, corpus)
    on = run(ctx, 70, q, k)
    assert on[2] == 15
    assert_same(on, run_exact(ctx, 70, q, k))
    assert_oracle(on, corpus, q, k)
    drop(ctx, 70)
