"""sdbv_append_rows / sdbv_table_reserve on the GPU: a table that rows were
appended to answers every search entry point in every bit like a table
staged once with all the rows.

Every comparison is exact equality of ids and of distance BITS, held against
the CPU oracle over the rows so far and against a twin: the same rows, ids
and explicit shadow staged once. Each append must report in
last_append_realloc what append_capacity predicts from the capacity before
it, and leave that capacity behind.

Shapes: a wave of the append kernel owns 64 absolute-aligned rows and walks
the features in blocks of 64 (d = 36: one partial block with the d % 8 == 4
tail; d = 64: one full block); staging 1003 rows leaves a capacity of 1024, so
batches of 1, 20, 1 start in mid-wave, fill the store exactly, then force the
first growth; 63 / 64 / 65 straddle a wave; 3000 and 4103 grow again and span
several 256-row shadow blocks."""
import ctypes

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ERR_NO_TABLE, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_IDS_UNSORTED = -2, -3, -5, -6
MIN_ROWS = ("SDBV_SCAN_PREFILTER_MIN_ROWS", "SDBV_SCAN_PREFILTER_I8_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_I6_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_H4_MIN_ROWS")
T, TWIN = 61, 62


@pytest.fixture(scope="module")
def ctx():
    import surrealdb_amd
    c = surrealdb_amd.Context()
    yield c
    c.close()


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run(ctx, table, q, k):
    """(ids, dists, path, candidates, stage1) of one knn_bruteforce call."""
    ids, dists = ctx.knn_bruteforce(table, q, k)
    st = ctx.stats()
    return (ids.copy(), dists.copy(), st["last_scan_path"],
            st["last_prefilter_candidates"], st["last_prefilter_stage1"])


def assert_result(got, want, what):
    assert np.array_equal(got[0], want[0]), f"ids differ from {what}"
    assert np.array_equal(bits(got[1]), bits(want[1])), \
        f"distance bits differ from {what}"


def append(ctx, table, rows, ids=None):
    """append_rows, checked against the capacity rule."""
    from surrealdb_amd import append_capacity
    n, cap = ctx.table_rows(table), ctx.table_capacity(table)
    want_cap = append_capacity(cap, n + len(rows))
    ctx.append_rows(table, rows, ids=ids)
    st = ctx.stats()
    assert ctx.table_rows(table) == n + len(rows)
    assert ctx.table_capacity(table) == want_cap
    assert st["last_append_realloc"] == int(want_cap != cap)
    assert st["last_append_ms"] > 0 and st["last_append_kernel_ms"] > 0
    return st["last_append_realloc"]


def near(q, seed, scale):
    """q plus noise of relative size about `scale`."""
    return (q + oracle.gen_f32(seed, 0, 1, q.size)[0] *
            np.float32(scale)).astype(np.float32)


NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]


def hostile(rows, q, metric):
    """Put into rows[0:5] a near copy of q, a zero row, a row with a NaN, one
    with an inf and one scaled by 1e30.

    The NaN is the negative quiet NaN on a cosine table. The oracle restates
    KnnTopK, where a NaN distance never displaces a finite worst entry, so it
    is comparable only while the device sorts such rows last, as +NaN; and
    on a cosine table the CPU and the device disagree on the sign of a NaN
    distance (tests/test_gpu_batch_edges.py). The zero row, the inf row and a
    -NaN element come out +NaN on the device and sort last; a +NaN element
    comes out -NaN and sorts FIRST there, on a table staged once as well
    (measured with np.nan here: top-1 row 5002, the NaN row, on the table and
    on its twin, against the oracle's 5000). The shadow test appends such a
    row too and holds it against the twin alone. On a euclidean table np.nan
    gives +NaN on both."""
    rows[0] = near(q, 0xAA, 2.0 ** -6)
    rows[1] = 0.0
    rows[2, 3] = NEG_NAN if metric == "cosine" else np.nan
    rows[3, 0] = np.inf
    rows[4] *= np.float32(1e30)
    return rows


def rc_append(ctx, table, rows, ids, m, d):
    """The raw return code of sdbv_append_rows."""
    import surrealdb_amd
    f32p, u64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)
    return surrealdb_amd.lib().sdbv_append_rows(
        ctx._ptr, table,
        None if rows is None else rows.ctypes.data_as(f32p),
        None if ids is None else ids.ctypes.data_as(u64p), m, d)


# ---- 1. exact scan --------------------------------------------------------

@pytest.mark.parametrize("d", [36, 64])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_exact_scan_after_each_batch(ctx, metric, d):
    batches = [1, 20, 1, 63, 64, 65, 3000, 4103]
    total = 1003 + sum(batches)
    allrows = oracle.gen_f32(0x5DB1, 0, total, d)
    Q = oracle.gen_f32(0xBEEF, 0, 3, d)
    ctx.stage_corpus(T, allrows[:1003], metric=metric)
    assert ctx.table_capacity(T) == 1024
    n, grown = 1003, []
    for b, m in enumerate(batches):
        # one near copy of query b % 3, nearer than the copies before it
        j = b % 3
        pos = n + (m - 1) // 2
        allrows[pos] = near(Q[j], 0x100 + b, 2.0 ** -(4 + 2 * (b // 3)))
        grown.append(append(ctx, T, allrows[n:n + m]))
        n += m
        assert ctx.table_rows(T) == n
        for qi in range(3):
            for k in (1, 10, 64):
                got = run(ctx, T, Q[qi], k)
                assert got[2] == 0
                assert_result(got, oracle.topk_f32(metric, allrows[:n],
                                                   Q[qi], k), "the oracle")
        assert run(ctx, T, Q[j], 1)[0][0] == pos
    assert grown == [0, 0, 1, 0, 0, 0, 1, 1]
    ctx.drop_table(T)


# ---- 2. ids ---------------------------------------------------------------

def test_ids_continue_and_are_checked(ctx):
    n, d, k = 300, 36, 10
    rows = oracle.gen_f32(0x71, 0, n + 40, d)
    q = oracle.gen_f32(0x72, 0, 1, d)[0]
    ids = np.arange(n + 40, dtype=np.uint64) * 10
    ids[n + 10:n + 20] = ids[n + 9] + 1 + np.arange(10)   # ids=None: last + i
    ids[n + 20:] = ids[n + 19] + 7 * (1 + np.arange(20))

    def check(count):
        oids, odists = oracle.topk_f32("cosine", rows[:count], q, k)
        got = ctx.knn_bruteforce(T, q, k)
        assert np.array_equal(got[0], ids[oids.astype(np.int64)])
        assert np.array_equal(bits(got[1]), bits(odists))
        return got

    ctx.stage_corpus(T, rows[:n], ids=ids[:n], metric="cosine")
    append(ctx, T, rows[n:n + 10], ids=ids[n:n + 10])       # explicit, larger
    check(n + 10)
    append(ctx, T, rows[n + 10:n + 20])                     # None continues
    before = check(n + 20)
    # refused: first id equal to the last staged one; a batch not increasing
    bad = ids[n + 20:].copy()
    bad[0] = ids[n + 19]
    assert rc_append(ctx, T, rows[n + 20:], bad, 20, d) == ERR_IDS_UNSORTED
    bad = ids[n + 20:].copy()
    bad[7] = bad[6]
    assert rc_append(ctx, T, rows[n + 20:], bad, 20, d) == ERR_IDS_UNSORTED
    assert ctx.table_rows(T) == n + 20
    after = ctx.knn_bruteforce(T, q, k)
    assert np.array_equal(after[0], before[0])
    assert np.array_equal(bits(after[1]), bits(before[1]))
    append(ctx, T, rows[n + 20:], ids=ids[n + 20:])
    check(n + 40)
    ctx.drop_table(T)


# ---- 3. shadows -----------------------------------------------------------

SHADOWS = {"bf16": ("cosine", 1), "int8": ("cosine", 3), "int6": ("cosine", 5),
           "h4": ("cosine", 15), "l2": ("euclidean", 17)}


def stage_with_shadow(ctx, table, rows, kind):
    metric = SHADOWS[kind][0]
    ctx.stage_corpus(table, rows, metric=metric)
    if kind == "bf16":
        ctx.table_set_prefilter_kind(table, 1)
    elif kind == "int8":
        ctx.table_set_prefilter_kind(table, 2)
    elif kind == "int6":
        ctx.table_set_prefilter_i6(table)
    elif kind == "l2":
        ctx.table_set_prefilter_l2(table, True)
    # h4: staged by the policy, which the caller has brought down to this size


@pytest.mark.parametrize("kind", sorted(SHADOWS))
def test_shadowed_table_equals_twin_and_oracle(ctx, kind, monkeypatch):
    if kind == "h4":        # as tests/test_gpu_prefilter_h4.py does it
        for name in MIN_ROWS:
            monkeypatch.setenv(name, "1")
        monkeypatch.delenv("SDBV_SCAN_PREFILTER_H4", raising=False)
        monkeypatch.delenv("SDBV_SCAN_PREFILTER_H4_LIST_MAX", raising=False)
    metric, path = SHADOWS[kind]
    n0, d, k = 5000, 64, 10
    allrows = oracle.gen_f32(0x5DB1, 0, n0 + 3100, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    hostile(allrows[n0:], q, metric)
    hostile(allrows[n0 + 100:], q, metric)
    allrows[n0 + 100] = near(q, 0xAB, 2.0 ** -8)    # nearer than the first
    stage_with_shadow(ctx, T, allrows[:n0], kind)
    n = n0
    for m in (100, 3000):
        append(ctx, T, allrows[n:n + m])
        n += m
        stage_with_shadow(ctx, TWIN, allrows[:n], kind)
        for kk in (1, k, 64):
            got, twin = run(ctx, T, q, kk), run(ctx, TWIN, q, kk)
            print(f"{kind} n={n} k={kk}: path {got[2]}, candidates {got[3]}, "
                  f"stage 1 {got[4]}; twin {twin[2:]}")
            assert got[2] == path == twin[2]
            assert got[3] == twin[3]
            assert got[4] == twin[4]
            assert_result(got, twin, "the twin")
            assert_result(got, oracle.topk_f32(metric, allrows[:n], q, kk),
                          "the oracle")
    # a +NaN element, first on a cosine table (see hostile): the twin alone
    last = oracle.gen_f32(0x5DB1, n, 1, d)
    last[0, 5] = np.nan
    append(ctx, T, last)
    stage_with_shadow(ctx, TWIN, np.concatenate([allrows[:n], last]), kind)
    for kk in (1, k):
        got, twin = run(ctx, T, q, kk), run(ctx, TWIN, q, kk)
        assert got[2:] == twin[2:] and got[2] == path
        assert_result(got, twin, "the twin")
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


# ---- 4. filtered ----------------------------------------------------------

FILTERED = {"masked_scan": ("cosine", 7, None),
            "row_list": ("cosine", 8, None),
            "int6": ("cosine", 13, "int6"),
            "l2": ("euclidean", 19, "l2")}


@pytest.mark.parametrize("case", sorted(FILTERED))
def test_filtered_after_append(ctx, case, monkeypatch):
    import surrealdb_amd
    metric, path, kind = FILTERED[case]
    if path != 8:
        monkeypatch.setenv("SDBV_FILTER_ROWLIST_MAX", "0")
    else:
        monkeypatch.delenv("SDBV_FILTER_ROWLIST_MAX", raising=False)
    monkeypatch.setenv("SDBV_FILTER_PREFILTER_MIN_ROWS", "0")
    monkeypatch.delenv("SDBV_FILTER_PREFILTER", raising=False)
    n0, d, k = 5000, 64, 10
    allrows = oracle.gen_f32(0x5DB1, 0, n0 + 3100, d)
    q = oracle.gen_f32(0xBEEF, 2, 1, d)[0]
    allrows[n0 + 7] = near(q, 0xAC, 2.0 ** -6)
    if kind:
        stage_with_shadow(ctx, T, allrows[:n0], kind)
    else:
        ctx.stage_corpus(T, allrows[:n0], metric=metric)
    old_words = surrealdb_amd._allow_words(np.ones(n0, bool), n0)
    n = n0
    for m in (100, 3000):
        append(ctx, T, allrows[n:n + m])
        n += m
        # a bitmap of the old length no longer fits
        out_ids = np.empty(k, np.uint64)
        out_d = np.empty(k, np.float64)
        out_n = ctypes.c_uint32(0)
        rc = surrealdb_amd.lib().sdbv_knn_bruteforce_filtered(
            ctx._ptr, T, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), d,
            k, old_words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            old_words.size,
            out_ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            out_d.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            ctypes.byref(out_n))
        assert rc == ERR_BAD_ARG
        masks = {"appended": np.arange(n) >= n0, "old": np.arange(n) < n0,
                 "half": np.random.default_rng(7).random(n) < 0.5}
        masks["half"][n0 + 7] = True
        for name, allow in masks.items():
            rows = np.flatnonzero(allow)
            oids, odists = oracle.topk_f32(
                metric, np.ascontiguousarray(allrows[:n][rows]), q, k)
            gids, gdists = ctx.knn_bruteforce_filtered(T, q, k, allow)
            st = ctx.stats()
            assert st["last_scan_path"] == path, (name, st["last_scan_path"])
            assert st["last_filter_rows"] == rows.size
            assert np.array_equal(gids,
                                  rows[oids.astype(np.int64)].astype(np.uint64))
            assert np.array_equal(bits(gdists), bits(odists))
            if name != "old":
                assert gids[0] == n0 + 7
    ctx.drop_table(T)


# ---- 5. all-distances route -----------------------------------------------

@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("metric,k", [("manhattan", 10), ("jaccard", 10),
                                      ("cosine", 100)])
def test_all_distances_route_after_append(ctx, metric, k, device, monkeypatch):
    if device:
        monkeypatch.delenv("SDBV_SELECT_DEVICE", raising=False)
        monkeypatch.setenv("SDBV_SELECT_DEVICE_MIN_ROWS", "0")
    else:
        monkeypatch.setenv("SDBV_SELECT_DEVICE", "0")
    n0, d = 5000, 64
    allrows = oracle.gen_f32(0x5DB1, 0, n0 + 3100, d)
    q = oracle.gen_f32(0xBEEF, 3, 1, d)[0]
    ctx.stage_corpus(T, allrows[:n0], metric=metric)
    n = n0
    for m in (100, 3000):
        allrows[n + 5] = q                  # an exact copy: distance 0, first
        append(ctx, T, allrows[n:n + m])
        n += m
        got = run(ctx, T, q, k)
        assert got[2] == (21 if device else 0)
        assert_result(got, oracle.topk_f32(metric, allrows[:n], q, k),
                      "the oracle")
        if metric != "jaccard":             # (bit-pattern sets: no distance 0)
            assert n - m + 5 in got[0][:2]
        allow = np.random.default_rng(11).random(n) < 0.5
        rows = np.flatnonzero(allow)
        oids, odists = oracle.topk_f32(
            metric, np.ascontiguousarray(allrows[:n][rows]), q, k)
        gids, gdists = ctx.knn_bruteforce_filtered(T, q, k, allow)
        assert ctx.stats()["last_scan_path"] == (22 if device else 0)
        assert np.array_equal(gids,
                              rows[oids.astype(np.int64)].astype(np.uint64))
        assert np.array_equal(bits(gdists), bits(odists))
    ctx.drop_table(T)


# ---- 6. batch -------------------------------------------------------------

def batch_check(ctx, metric, staged, batches, b):
    """Stage `staged`, append each of `batches`; after each append every
    query of knn_batch equals the single-query scan, nothing refolds, and as
    many queries go to the exact scan as on the twin."""
    d, k = staged.shape[1], 10
    Q = oracle.gen_f32(0xBEEF, 4, b, d)
    Q[1] = batches[0][0]                    # an appended row as the query
    ctx.stage_corpus(T, staged, metric=metric)
    sofar = staged
    for rows in batches:
        append(ctx, T, rows)
        sofar = np.concatenate([sofar, rows])
        ctx.stage_corpus(TWIN, sofar, metric=metric)
        ids, dists = ctx.knn_batch(T, Q, k)
        st = ctx.stats()
        tids, tdists = ctx.knn_batch(TWIN, Q, k)
        tst = ctx.stats()
        assert st["last_batch_refold"] == 0
        assert st["last_batch_exact_queries"] == \
            tst["last_batch_exact_queries"]
        assert np.array_equal(ids, tids)
        assert np.array_equal(bits(dists), bits(tdists))
        for j in range(b):
            sids, sdists = ctx.knn_bruteforce(T, Q[j], k)
            assert np.array_equal(ids[j], sids), f"query {j}"
            assert np.array_equal(bits(dists[j]), bits(sdists)), f"query {j}"
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


def far_row(staged):
    """A row whose norm is 1e6 times the largest staged one."""
    norms = np.sqrt((staged.astype(np.float64) ** 2).sum(axis=1))
    return (staged[int(np.argmax(norms))] * np.float32(1e6)).astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_batch_legacy_shape(ctx, metric):
    d = 32
    staged = oracle.gen_f32(0x5DB1, 0, 2500, d)
    rows = oracle.gen_f32(0x5DB1, 2500, 500, d)
    hostile(rows[1:], oracle.gen_f32(0xBEEF, 4, 1, d)[0], metric)
    rows[7, 2] = np.nan                     # either sign: no oracle here
    if metric == "euclidean":
        rows[10] = far_row(staged)
    batch_check(ctx, metric, staged, [rows], 7)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_batch_fused_shape(ctx, metric):
    """(65536 + 2048) x 32 with b = 128 is the smallest shape that reaches
    k_mfma_scan_topk; the capacity is full, so the first append grows."""
    d, n0 = 32, 65536 + 2048
    staged = oracle.gen_f32(0x5DB1, 0, n0, d)
    first = oracle.gen_f32(0x5DB1, n0, 1024, d)
    second = oracle.gen_f32(0x5DB1, n0 + 1024, 1024, d)
    if metric == "euclidean":
        second[10] = far_row(staged)
    batch_check(ctx, metric, staged, [first, second], 128)


# ---- 7. reserve -----------------------------------------------------------

def test_reserve_then_appends_run_in_place(ctx):
    import surrealdb_amd
    d, k = 36, 10
    allrows = oracle.gen_f32(0x5DB1, 0, 3000 + 5289, d)
    q = oracle.gen_f32(0xBEEF, 5, 1, d)[0]
    ctx.stage_corpus(T, allrows[:3000], metric="euclidean")
    assert ctx.table_capacity(T) == 3072
    ctx.table_reserve(T, 10000)
    assert ctx.table_capacity(T) == 12288
    assert ctx.table_rows(T) == 3000
    assert_result(run(ctx, T, q, k),
                  oracle.topk_f32("euclidean", allrows[:3000], q, k),
                  "the oracle")
    ctx.table_reserve(T, 5000)              # below the capacity: a no-op
    ctx.table_reserve(T, 12288)
    assert ctx.table_capacity(T) == 12288
    n = 3000
    for m in (1, 63, 64, 65, 1000, 4096):
        assert append(ctx, T, allrows[n:n + m]) == 0
        n += m
        assert_result(run(ctx, T, q, k),
                      oracle.topk_f32("euclidean", allrows[:n], q, k),
                      "the oracle")
    assert ctx.table_capacity(T) == 12288
    ctx.drop_table(T)
    assert surrealdb_amd.lib().sdbv_table_reserve(ctx._ptr, T, 100) == \
        ERR_NO_TABLE
    assert ctx.table_capacity(T) == 0


# ---- 8. refusals ----------------------------------------------------------

def test_refusals_leave_the_table_alone(ctx):
    import math
    n, d, k = 200, 36, 5
    rows = oracle.gen_f32(0x5DB1, 0, n + 8, d)
    q = oracle.gen_f32(0xBEEF, 6, 1, d)[0]
    ctx.stage_corpus(T, rows[:n], metric="cosine")
    before = run(ctx, T, q, k)
    new = np.ascontiguousarray(rows[n:])
    assert rc_append(ctx, 999, new, None, 8, d) == ERR_NO_TABLE
    wide = oracle.gen_f32(1, 0, 8, d + 4)
    assert rc_append(ctx, T, wide, None, 8, d + 4) == ERR_BAD_ARG
    assert rc_append(ctx, T, None, None, 8, d) == ERR_BAD_ARG
    assert rc_append(ctx, T, new, None, 2 ** 32 - n, d) == ERR_BAD_ARG
    assert rc_append(ctx, T, new, None, 0, d) == 0
    assert rc_append(ctx, T, None, None, 0, d) == 0
    assert ctx.table_rows(T) == n and ctx.table_capacity(T) == 1024
    assert_result(run(ctx, T, q, k), before, "the call before")
    # a table staged for graph search
    pts = oracle.gen_f32(0x33, 0, 64, 20)
    h = ctx.hnsw_create(20, metric="euclidean", m=8, efc=100,
                        ml=1.0 / math.log(8.0), seed=0x5DB1)
    h.insert_batch(pts, nthreads=1)
    h.finalize(TWIN)
    assert rc_append(ctx, TWIN, pts, None, 8, 20) == ERR_UNSUPPORTED
    assert ctx.table_rows(TWIN) == 64
    h.destroy()
    ctx.drop_table(TWIN)
    ctx.drop_table(T)


# ---- 9. gather and byte count ---------------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_gather_and_bytes_staged(ctx, metric):
    n0, d = 1003, 36
    allrows = oracle.gen_f32(0x5DB1, 0, n0 + 121, d)
    q = oracle.gen_f32(0xBEEF, 7, 1, d)[0]
    base = ctx.stats()["bytes_staged"]
    ctx.stage_corpus(T, allrows[:n0], metric=metric)
    per_row = 4 * d + 12 + (8 if metric == "cosine" else 0)
    assert ctx.stats()["bytes_staged"] - base == 1024 * per_row
    append(ctx, T, allrows[n0:n0 + 21])             # in place
    assert ctx.stats()["bytes_staged"] - base == 1024 * per_row
    append(ctx, T, allrows[n0 + 21:])               # grows to 4096
    assert ctx.stats()["bytes_staged"] - base == 4096 * per_row
    idx = np.array([n0, n0 + 20, n0 + 21, n0 + 120, 0, n0 - 1], np.uint32)
    got = ctx.gather_distance(T, idx, q)
    want = np.array([oracle.dist_f32(metric, allrows[i], q) for i in idx])
    assert np.array_equal(bits(got), bits(want))
    ctx.drop_table(T)
    assert ctx.stats()["bytes_staged"] == base
