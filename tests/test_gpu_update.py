"""sdbv_update_rows on the GPU: a table whose staged rows were replaced in
place answers every search entry point in every bit like a table staged once
with the current rows.

Every comparison is exact equality of ids and of distance BITS, held against
the CPU oracle over the current rows and against a twin: the current rows and
the same explicit shadow staged once. Every update must leave the row count,
the capacity, bytes_staged and the append's stats fields alone and report in
last_update_blocks the number of 256-row blocks update_blocks predicts (0 on
a table without a shadow).

Shapes: a wave of the update kernel owns 64 consecutive entries of the row
list and walks the features in blocks of 64 (d = 36: one partial block with
the d % 8 == 4 tail; d = 132: two full blocks and a partial one). 1003 staged
rows leave a capacity of 1024; the lists are one row at either end, 64
adjacent rows across a 64-row boundary of the store, 65 entries (a second
wave with one live lane), four rows in three 256-row blocks, and all rows."""
import ctypes
import math

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ERR_NO_TABLE, ERR_BAD_ARG, ERR_UNSUPPORTED = -2, -3, -5
MIN_ROWS = ("SDBV_SCAN_PREFILTER_MIN_ROWS", "SDBV_SCAN_PREFILTER_I8_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_I6_MIN_ROWS",
            "SDBV_SCAN_PREFILTER_H4_MIN_ROWS")
T, TWIN = 71, 72
APPEND_FIELDS = ("last_append_ms", "last_append_kernel_ms",
                 "last_append_realloc")


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


def update(ctx, table, idx, rows, shadow=False):
    """update_rows, checked against everything it must leave alone."""
    from surrealdb_amd import update_blocks
    idx = np.asarray(idx, dtype=np.uint32)
    before = ctx.stats()
    n, cap = ctx.table_rows(table), ctx.table_capacity(table)
    ctx.update_rows(table, idx, rows)
    st = ctx.stats()
    assert ctx.table_rows(table) == n
    assert ctx.table_capacity(table) == cap
    assert st["bytes_staged"] == before["bytes_staged"]
    for f in APPEND_FIELDS:
        assert st[f] == before[f], f
    assert st["last_update_ms"] > 0 and st["last_update_kernel_ms"] > 0
    assert st["last_update_blocks"] == \
        (len(update_blocks(idx)) if shadow else 0)


def near(q, seed, scale):
    """q plus noise of relative size about `scale`."""
    return (q + oracle.gen_f32(seed, 0, 1, q.size)[0] *
            np.float32(scale)).astype(np.float32)


NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]


def hostile(rows, q, metric, scale=2.0 ** -6):
    """Put into rows[0:5] a near copy of q, a zero row, a row with a NaN, one
    with an inf and one scaled by 1e30. The NaN is the negative quiet NaN on
    a cosine table, where alone the device and the oracle agree on where a
    NaN distance sorts (tests/test_gpu_append.py, hostile)."""
    rows[0] = near(q, 0xAA, scale)
    rows[1] = 0.0
    rows[2, 3] = NEG_NAN if metric == "cosine" else np.nan
    rows[3, 0] = np.inf
    rows[4] *= np.float32(1e30)
    return rows


def scattered(rng, n, m, include=()):
    """About m distinct sorted positions below n, `include` among them."""
    idx = rng.choice(n, m, replace=False)
    return np.unique(np.concatenate([idx, np.asarray(include, np.int64)])
                     ).astype(np.uint32)


def rc_update(ctx, table, idx, rows, m, d):
    """The raw return code of sdbv_update_rows."""
    import surrealdb_amd
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    return surrealdb_amd.lib().sdbv_update_rows(
        ctx._ptr, table,
        None if idx is None else idx.ctypes.data_as(u32p),
        None if rows is None else rows.ctypes.data_as(f32p), m, d)


# ---- 1. kernel edges ------------------------------------------------------

LISTS = {"first": [0], "last": [1002], "adjacent64": list(range(30, 94)),
         "waves65": list(range(3, 3 + 65 * 15, 15)),
         "blocks": [5, 300, 301, 1000], "all": list(range(1003))}


def check_all(ctx, metric, cur, Q):
    """T against the oracle and a twin staged once with `cur`: the exact scan
    at k = 1, 10, 64 and the batch path (norms and aux of the written rows)."""
    ctx.stage_corpus(TWIN, cur, metric=metric)
    out = []
    for q in Q:
        for k in (1, 10, 64):
            got = run(ctx, T, q, k)
            assert got[2] == 0
            assert_result(got, oracle.topk_f32(metric, cur, q, k),
                          "the oracle")
            assert_result(got, run(ctx, TWIN, q, k), "the twin")
            out.append(got)
    ids, dists = ctx.knn_batch(T, Q, 10)
    st = ctx.stats()
    tids, tdists = ctx.knn_batch(TWIN, Q, 10)
    tst = ctx.stats()
    assert st["last_batch_refold"] == 0 == tst["last_batch_refold"]
    assert st["last_batch_exact_queries"] == tst["last_batch_exact_queries"]
    assert np.array_equal(ids, tids)
    assert np.array_equal(bits(dists), bits(tdists))
    return out


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("d", [36, 132])
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_kernel_edges(ctx, metric, d, name):
    n = 1003
    idx = np.array(LISTS[name], dtype=np.uint32)
    m = idx.size
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 3 * n, d)
    Q = oracle.gen_f32(0xBEEF, 0, 2, d)
    ctx.stage_corpus(T, cur, metric=metric)
    assert ctx.table_capacity(T) == 1024
    # A: new rows everywhere on the list, one of them a near copy of Q[0]
    a = (m - 1) // 2
    new = fresh[:m].copy()
    new[a] = near(Q[0], 0x100, 2.0 ** -4)
    update(ctx, T, idx, new)
    cur[idx] = new
    check_all(ctx, metric, cur, Q)
    assert run(ctx, T, Q[0], 1)[0][0] == idx[a]
    # B: the nearest row becomes an ordinary one and must disappear; on a
    # list of several rows another becomes a nearer copy
    new = fresh[n:n + m].copy()
    b = m - 1 if m > 1 else None
    if b is not None:
        new[b] = near(Q[0], 0x101, 2.0 ** -6)
    update(ctx, T, idx, new)
    cur[idx] = new
    res = check_all(ctx, metric, cur, Q)
    assert res[0][0][0] != idx[a]           # Q[0], k = 1
    if b is not None:
        assert res[0][0][0] == idx[b]
    # C: the rows' own content changes nothing
    update(ctx, T, idx, np.ascontiguousarray(cur[idx]))
    again = check_all(ctx, metric, cur, Q)
    for x, y in zip(res, again):
        assert_result(y, x, "the call before")
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_update_around_append_and_reserve(ctx, metric):
    d, n0 = 36, 1003
    allrows = oracle.gen_f32(0x5DB1, 0, n0 + 121, d)
    fresh = oracle.gen_f32(0x5DB1, 5000, 400, d)
    Q = oracle.gen_f32(0xBEEF, 1, 2, d)
    ctx.stage_corpus(T, allrows[:n0], metric=metric)
    ctx.append_rows(T, allrows[n0:n0 + 21])         # fills the 1024 exactly
    n = n0 + 21
    cur = allrows[:n].copy()
    # after an append: staged and appended rows, the last cell of the store
    idx = np.array([5, 1002, 1003, 1010, 1023], np.uint32)
    new = fresh[:5].copy()
    new[2] = near(Q[0], 0x110, 2.0 ** -4)
    update(ctx, T, idx, new)
    cur[idx] = new
    check_all(ctx, metric, cur, Q)
    assert run(ctx, T, Q[0], 1)[0][0] == 1003
    # after a reserve: capacity above roundup(n, 1024)
    ctx.table_reserve(T, 5000)
    assert ctx.table_capacity(T) == 8192
    idx = np.arange(900, 1024, dtype=np.uint32)
    new = fresh[5:5 + idx.size].copy()
    new[100] = near(Q[0], 0x111, 2.0 ** -6)         # row 1000; 1003 goes
    update(ctx, T, idx, new)
    cur[idx] = new
    check_all(ctx, metric, cur, Q)
    assert run(ctx, T, Q[0], 1)[0][0] == 1000
    # an append after an update, then an update of the appended rows
    ctx.append_rows(T, allrows[n:n + 100])
    cur = np.concatenate([cur, allrows[n:n + 100]])
    n += 100
    check_all(ctx, metric, cur, Q)
    idx = np.array([0, 1000, n - 100, n - 1], np.uint32)
    new = fresh[200:204].copy()
    new[3] = near(Q[0], 0x112, 2.0 ** -8)
    update(ctx, T, idx, new)
    cur[idx] = new
    check_all(ctx, metric, cur, Q)
    assert run(ctx, T, Q[0], 1)[0][0] == n - 1
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


# ---- 2. shadows -----------------------------------------------------------

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


def hostile_update(rng, n, m, fresh, q, metric, was_hostile, scale):
    """(idx, new, hostile positions): about m scattered rows, the rows that
    were hostile among them and now ordinary, and five rows that were
    ordinary now hostile, the first of them the nearest copy of q so far.
    The hostile rows lie behind row 1000: the oracle restates KnnTopK, which
    keeps a NaN distance that arrives before its k entries are full, so a
    NaN row among the first k rows is not comparable (hostile)."""
    idx = scattered(rng, n, m, include=was_hostile)
    new = fresh[:idx.size].copy()
    p = next(i for i in range(idx.size - 5) if idx[i] >= 1000 and
             not np.isin(idx[i:i + 5], was_hostile).any())
    hostile(new[p:], q, metric, scale)
    return idx, new, idx[p:p + 5].copy()


@pytest.mark.parametrize("kind", sorted(SHADOWS))
def test_shadowed_table_equals_twin_and_oracle(ctx, kind, monkeypatch):
    if kind == "h4":        # as tests/test_gpu_prefilter_h4.py does it
        for name in MIN_ROWS:
            monkeypatch.setenv(name, "1")
        monkeypatch.delenv("SDBV_SCAN_PREFILTER_H4", raising=False)
        monkeypatch.delenv("SDBV_SCAN_PREFILTER_H4_LIST_MAX", raising=False)
    metric, path = SHADOWS[kind]
    n, d, k = 5000, 64, 10
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 3200, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    hostile(cur[2040:], q, metric, 2.0 ** -4)
    was = np.arange(2040, 2045)
    stage_with_shadow(ctx, T, cur, kind)
    rng = np.random.default_rng(5)
    for step, m in enumerate((100, 3000)):
        idx, new, was = hostile_update(rng, n, m, fresh[100 * step:], q,
                                       metric, was, 2.0 ** -(6 + 2 * step))
        update(ctx, T, idx, new, shadow=True)
        cur[idx] = new
        stage_with_shadow(ctx, TWIN, cur, kind)
        for kk in (1, k, 64):
            got, twin = run(ctx, T, q, kk), run(ctx, TWIN, q, kk)
            print(f"{kind} m={idx.size} k={kk}: path {got[2]}, candidates "
                  f"{got[3]}, stage 1 {got[4]}; twin {twin[2:]}")
            assert got[2] == path == twin[2]
            assert got[3] == twin[3]
            assert got[4] == twin[4]
            assert_result(got, twin, "the twin")
            assert_result(got, oracle.topk_f32(metric, cur, q, kk),
                          "the oracle")
        assert run(ctx, T, q, 1)[0][0] == was[0]
    # a +NaN element, first on a cosine table (see hostile): the twin alone
    one = fresh[3199:3200].copy()
    one[0, 5] = np.nan
    update(ctx, T, [2500], one, shadow=True)
    cur[2500] = one[0]
    stage_with_shadow(ctx, TWIN, cur, kind)
    for kk in (1, k):
        got, twin = run(ctx, T, q, kk), run(ctx, TWIN, q, kk)
        assert got[2:] == twin[2:] and got[2] == path
        assert_result(got, twin, "the twin")
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


# ---- 3. filtered ----------------------------------------------------------

FILTERED = {"masked_scan": ("cosine", 7, None),
            "row_list": ("cosine", 8, None),
            "int6": ("cosine", 13, "int6"),
            "l2": ("euclidean", 19, "l2")}


@pytest.mark.parametrize("case", sorted(FILTERED))
def test_filtered_after_update(ctx, case, monkeypatch):
    metric, path, kind = FILTERED[case]
    if path != 8:
        monkeypatch.setenv("SDBV_FILTER_ROWLIST_MAX", "0")
    else:
        monkeypatch.delenv("SDBV_FILTER_ROWLIST_MAX", raising=False)
    monkeypatch.setenv("SDBV_FILTER_PREFILTER_MIN_ROWS", "0")
    monkeypatch.delenv("SDBV_FILTER_PREFILTER", raising=False)
    n, d, k = 5000, 64, 10
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 3200, d)
    q = oracle.gen_f32(0xBEEF, 2, 1, d)[0]
    cur[17] = near(q, 0xAC, 2.0 ** -4)      # nearest as staged
    if kind:
        stage_with_shadow(ctx, T, cur, kind)
    else:
        ctx.stage_corpus(T, cur, metric=metric)
    rng = np.random.default_rng(6)
    best = 17
    for step, m in enumerate((100, 3000)):
        idx = scattered(rng, n, m, include=[best])
        new = fresh[100 * step:100 * step + idx.size].copy()
        p = int(np.flatnonzero(idx == best)[0])
        p = p + 1 if p + 1 < idx.size else p - 1
        new[p] = near(q, 0xAD + step, 2.0 ** -(6 + 2 * step))
        update(ctx, T, idx, new, shadow=bool(kind))
        cur[idx] = new                      # the old nearest is ordinary now
        best = int(idx[p])
        touched = np.zeros(n, bool)
        touched[idx] = True
        masks = {"updated": touched, "untouched": ~touched,
                 "half": np.random.default_rng(7).random(n) < 0.5}
        masks["half"][best] = True
        for name, allow in masks.items():
            rows = np.flatnonzero(allow)
            oids, odists = oracle.topk_f32(
                metric, np.ascontiguousarray(cur[rows]), q, k)
            gids, gdists = ctx.knn_bruteforce_filtered(T, q, k, allow)
            st = ctx.stats()
            assert st["last_scan_path"] == path, (name, st["last_scan_path"])
            assert st["last_filter_rows"] == rows.size
            assert np.array_equal(gids,
                                  rows[oids.astype(np.int64)].astype(np.uint64))
            assert np.array_equal(bits(gdists), bits(odists))
            if name != "untouched":
                assert gids[0] == best
    ctx.drop_table(T)


# ---- 4. all-distances route -----------------------------------------------

@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("metric,k", [("manhattan", 10), ("jaccard", 10),
                                      ("cosine", 100)])
def test_all_distances_route_after_update(ctx, metric, k, device, monkeypatch):
    if device:
        monkeypatch.delenv("SDBV_SELECT_DEVICE", raising=False)
        monkeypatch.setenv("SDBV_SELECT_DEVICE_MIN_ROWS", "0")
    else:
        monkeypatch.setenv("SDBV_SELECT_DEVICE", "0")
    n, d = 5000, 64
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 3200, d)
    q = oracle.gen_f32(0xBEEF, 3, 1, d)[0]
    ctx.stage_corpus(T, cur, metric=metric)
    rng = np.random.default_rng(8)
    copy_at = None
    for step, m in enumerate((100, 3000)):
        # the exact copy of the step before is overwritten, a new one lands
        idx = scattered(rng, n, m,
                        include=[] if copy_at is None else [copy_at])
        new = fresh[100 * step:100 * step + idx.size].copy()
        p = 5 if copy_at is None or idx[5] != copy_at else 6
        new[p] = q                          # distance 0, first
        update(ctx, T, idx, new)
        cur[idx] = new
        copy_at = int(idx[p])
        got = run(ctx, T, q, k)
        assert got[2] == (21 if device else 0)
        assert_result(got, oracle.topk_f32(metric, cur, q, k), "the oracle")
        if metric != "jaccard":             # (bit-pattern sets: no distance 0)
            assert got[0][0] == copy_at
        allow = np.random.default_rng(11).random(n) < 0.5
        rows = np.flatnonzero(allow)
        oids, odists = oracle.topk_f32(
            metric, np.ascontiguousarray(cur[rows]), q, k)
        gids, gdists = ctx.knn_bruteforce_filtered(T, q, k, allow)
        assert ctx.stats()["last_scan_path"] == (22 if device else 0)
        assert np.array_equal(gids,
                              rows[oids.astype(np.int64)].astype(np.uint64))
        assert np.array_equal(bits(gdists), bits(odists))
    ctx.drop_table(T)


# ---- 5. batch, and the fold that forgets -----------------------------------

def batch_state(ctx, metric, cur, Q, k=10):
    """knn_batch on T equals the twin staged once with `cur` and the
    single-query scan, nothing refolds, and as many queries go to the exact
    scan as on the twin. Returns (that count, ids)."""
    ctx.stage_corpus(TWIN, cur, metric=metric)
    ids, dists = ctx.knn_batch(T, Q, k)
    st = ctx.stats()
    tids, tdists = ctx.knn_batch(TWIN, Q, k)
    tst = ctx.stats()
    assert st["last_batch_refold"] == 0 == tst["last_batch_refold"]
    assert st["last_batch_exact_queries"] == tst["last_batch_exact_queries"]
    assert np.array_equal(ids, tids)
    assert np.array_equal(bits(dists), bits(tdists))
    for j in range(len(Q)):
        sids, sdists = ctx.knn_bruteforce(T, Q[j], k)
        assert np.array_equal(ids[j], sids), f"query {j}"
        assert np.array_equal(bits(dists[j]), bits(sdists)), f"query {j}"
    return tst["last_batch_exact_queries"], ids


FAR = 1e6


def far_row(staged):
    """A row whose norm is FAR times the largest staged one."""
    norms = np.sqrt((staged.astype(np.float64) ** 2).sum(axis=1))
    return (staged[int(np.argmax(norms))] * np.float32(FAR)).astype(np.float32)


SHAPES = {"legacy": (2500, 7), "fused": (65536 + 2048, 128)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_batch_after_update(ctx, metric, shape):
    """The fused shape is the smallest that reaches k_mfma_scan_topk."""
    n, b = SHAPES[shape]
    d = 32
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 1100, d)
    Q = oracle.gen_f32(0xBEEF, 4, b, d)
    ctx.stage_corpus(T, cur, metric=metric)
    rng = np.random.default_rng(9)
    special = []
    for step, m in enumerate((64, 1000)):
        # the near copies of the step before are overwritten
        idx = scattered(rng, n, m, include=[n - 1] + special)
        new = fresh[64 * step:64 * step + idx.size].copy()
        hostile(new[1:], Q[0], metric, 2.0 ** -(6 + 2 * step))
        new[7, 2] = np.nan                  # either sign: no oracle here
        new[9] = Q[1] * np.float32(1e10)    # no usable key, yet the nearest
        update(ctx, T, idx, new)
        cur[idx] = new
        special = [int(idx[1]), int(idx[9])]
        _, ids = batch_state(ctx, metric, cur, Q)
        # (among the first ten: a row with a NaN may sort ahead)
        assert idx[1] in ids[0]
        if metric == "cosine":
            assert idx[9] in ids[1]
        Q[2] = new[20]                      # an updated row as the query
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fold_forgets_the_largest_norm(ctx, shape):
    """Euclidean: the key bound grows with the square of the largest keyed
    norm, so one row FAR = 1e6 times the rest sends queries to the exact
    scan that the window serves once that row is an ordinary one again. A
    header continued as the append does keeps the old maximum and with it
    the old count."""
    n, b = SHAPES[shape]
    d = 32
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    Q = oracle.gen_f32(0xBEEF, 4, b, d)
    at = n // 3
    ordinary = cur[at].copy()
    cur[at] = far_row(cur)
    ctx.stage_corpus(T, cur, metric="euclidean")
    with_far, _ = batch_state(ctx, "euclidean", cur, Q)
    update(ctx, T, [at], ordinary[None])
    cur[at] = ordinary
    without, _ = batch_state(ctx, "euclidean", cur, Q)
    print(f"exact queries of {b}: {with_far} with the far row, {without} "
          f"without")
    assert with_far != without
    # and back: the maximum grows again
    far = far_row(cur)
    update(ctx, T, [at + 1], far[None])
    cur[at + 1] = far
    again, _ = batch_state(ctx, "euclidean", cur, Q)
    assert again != without
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fold_forgets_a_row_without_a_key(ctx, shape):
    """Cosine: 1025 zero rows are one more than the batch call lists, so
    every query goes to the exact scan; with one of them an ordinary row
    again 1024 are left and the window serves; a zero written over an
    ordinary row brings the 1025 back. A count continued as the append does
    only ever grows."""
    n, b = SHAPES[shape]
    d = 32
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    fresh = oracle.gen_f32(0x5DB1, n, 4, d)
    Q = oracle.gen_f32(0xBEEF, 4, b, d)
    zeros = np.sort(np.random.default_rng(10).choice(n, 1025, replace=False))
    cur[zeros] = 0.0
    ctx.stage_corpus(T, cur, metric="cosine")
    c1025, _ = batch_state(ctx, "cosine", cur, Q)
    assert c1025 == b
    update(ctx, T, [zeros[500]], fresh[:1])
    cur[zeros[500]] = fresh[0]
    c1024, _ = batch_state(ctx, "cosine", cur, Q)
    print(f"exact queries of {b}: {c1025} with 1025 zero rows, {c1024} with "
          f"1024")
    assert c1024 != c1025
    other = int(np.setdiff1d(np.arange(n), zeros)[0])
    update(ctx, T, [other], np.zeros((1, d), np.float32))
    cur[other] = 0.0
    again, _ = batch_state(ctx, "cosine", cur, Q)
    assert again == c1025
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


# ---- 6. gather, invariants, refusals --------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_gather_of_updated_rows(ctx, metric):
    n, d = 1003, 36
    cur = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 7, 1, d)[0]
    ctx.stage_corpus(T, cur, metric=metric)
    idx = np.array([0, 63, 64, 500, 1002], np.uint32)
    new = oracle.gen_f32(0x5DB1, n, idx.size, d)
    update(ctx, T, idx, new)
    cur[idx] = new
    look = np.array([0, 1, 63, 64, 65, 500, 1002, 1001], np.uint32)
    got = ctx.gather_distance(T, look, q)
    want = np.array([oracle.dist_f32(metric, cur[i], q) for i in look])
    assert np.array_equal(bits(got), bits(want))
    ctx.drop_table(T)


def test_refusals_leave_the_table_alone(ctx):
    n, d, k = 200, 36, 5
    rows = oracle.gen_f32(0x5DB1, 0, n + 8, d)
    q = oracle.gen_f32(0xBEEF, 6, 1, d)[0]
    ctx.stage_corpus(T, rows[:n], metric="cosine")
    before = run(ctx, T, q, k)
    stats = ctx.stats()
    new = np.ascontiguousarray(rows[n:])
    idx = np.array([3, 9, 10, 50, 51, 52, 100, 199], np.uint32)
    assert rc_update(ctx, 999, idx, new, 8, d) == ERR_NO_TABLE
    wide = oracle.gen_f32(1, 0, 8, d + 4)
    assert rc_update(ctx, T, idx, wide, 8, d + 4) == ERR_BAD_ARG
    assert rc_update(ctx, T, idx, None, 8, d) == ERR_BAD_ARG
    assert rc_update(ctx, T, None, new, 8, d) == ERR_BAD_ARG
    bad = idx.copy()
    bad[7] = n                              # one past the last row
    assert rc_update(ctx, T, bad, new, 8, d) == ERR_BAD_ARG
    bad[7] = 2 ** 32 - 1
    assert rc_update(ctx, T, bad, new, 8, d) == ERR_BAD_ARG
    bad = idx.copy()
    bad[4] = bad[3]                         # a position twice
    assert rc_update(ctx, T, bad, new, 8, d) == ERR_BAD_ARG
    bad = idx.copy()
    bad[[1, 2]] = bad[[2, 1]]               # decreasing
    assert rc_update(ctx, T, bad, new, 8, d) == ERR_BAD_ARG
    assert rc_update(ctx, T, idx, new, 0, d) == 0
    assert rc_update(ctx, T, None, None, 0, d) == 0
    assert ctx.table_rows(T) == n and ctx.table_capacity(T) == 1024
    after = ctx.stats()
    for f in ("last_update_ms", "last_update_kernel_ms", "last_update_blocks",
              "bytes_staged"):
        assert after[f] == stats[f], f
    assert_result(run(ctx, T, q, k), before, "the call before")
    # a table staged for graph search
    pts = oracle.gen_f32(0x33, 0, 64, 20)
    h = ctx.hnsw_create(20, metric="euclidean", m=8, efc=100,
                        ml=1.0 / math.log(8.0), seed=0x5DB1)
    h.insert_batch(pts, nthreads=1)
    h.finalize(TWIN)
    assert rc_update(ctx, TWIN, idx[:4], pts, 4, 20) == ERR_UNSUPPORTED
    assert ctx.table_rows(TWIN) == 64
    h.destroy()
    ctx.drop_table(TWIN)
    ctx.drop_table(T)
