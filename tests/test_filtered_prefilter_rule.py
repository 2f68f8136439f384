"""The prefilter's selection rule on a row subset, checked on the CPU
(DESIGN.md §12b).

The three tiers' approximate sides are restated in numpy from the library's
own host quantisers (sdbv_bf16_rne, sdbv_prefilter_eps,
sdbv_prefilter_i8_row, sdbv_prefilter_i6_row, sdbv_prefilter_q12), as in the
three *_bound.py tests. Per tier a row is a candidate when

  bf16        a_i <= A_K + 2 eps(d),  A_K the Kth smallest a_i,
  int8, int6  l_i <= U_K,             U_K the Kth smallest u_i = a_i + e_i,

and the filtered call takes A_K / U_K over the ALLOWED rows and offers only
allowed rows. Then every row of the oracle's top K on the subset is a
candidate, for any mask. Taking the threshold over the whole table is not a
shortcut: when the best allowed row ranks behind the table's best rows, the
table's threshold passes fewer than K allowed rows, and the result would be
wrong."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

N, D, K = 2500, 32, 10
TIER_NAMES = ["bf16", "int8", "int6"]


def sumsq_f32(X):
    """The restated unrolled-8 f32 sum-of-squares chain, per row of X."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    m, d = X.shape
    p = np.zeros((m, 8), dtype=np.float32)
    d8 = d - d % 8
    for i in range(0, d8, 8):
        c = X[:, i:i + 8]
        p = p + c * c
    acc = np.zeros(m, dtype=np.float32)
    acc = acc + ((p[:, 0] + p[:, 4]) + (p[:, 1] + p[:, 5]))
    acc = acc + ((p[:, 2] + p[:, 6]) + (p[:, 3] + p[:, 7]))
    for i in range(d8, d):
        acc = acc + X[:, i] * X[:, i]
    return acc


def norms_f64(X):
    return np.sqrt(sumsq_f32(X).astype(np.float64))


def round_up_f32(e):
    f = np.float32(e)
    if np.float64(f) < e:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def bounds_bf16(q, X):
    """(lower, upper) as the rule uses them: a_i <= A_K + 2 eps is
    a_i - eps <= (A_K + eps), and the K rows with a_i <= A_K have exact
    distances <= A_K + eps."""
    Xs = np.array([surrealdb_amd.bf16_rne(v) for v in X.ravel()],
                  dtype=np.float32).reshape(X.shape)
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(X.shape[1]):
        acc = acc + Xs[:, k] * q[k]
    inv_i = (1.0 / norms_f64(X)).astype(np.float32)
    inv_q = np.float32(1.0 / norms_f64(q.reshape(1, -1))[0])
    a = (np.float32(1.0) - acc * inv_q * inv_i).astype(np.float64)
    eps = np.float64(surrealdb_amd.prefilter_eps(X.shape[1]))
    return a - eps, a + eps


def bounds_i8(q, X):
    nm = norms_f64(X)
    rows = [surrealdb_amd.prefilter_i8_row(x, n) for x, n in zip(X, nm)]
    codes = np.stack([r[0] for r in rows])
    scale = np.array([r[1] for r in rows], dtype=np.float32)
    eps = np.array([r[2] for r in rows], dtype=np.float32)
    b = codes.astype(np.float64) + 128.0
    t = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(X.shape[1]):
        t = (t.astype(np.float64) + b[:, k] * np.float64(q[k])).astype(
            np.float32)
    qbias = np.float32(128.0 * np.sum(q.astype(np.float64)))
    pscale = (scale.astype(np.float64) / nm).astype(np.float32)
    inv_q = np.float32(1.0 / norms_f64(q.reshape(1, -1))[0])
    a = np.float32(1.0) - (t - qbias) * inv_q * pscale
    assert a.dtype == np.float32 and eps.dtype == np.float32
    return (a - eps).astype(np.float64), (a + eps).astype(np.float64)


def bounds_i6(q, X):
    nm = norms_f64(X)
    rows = [surrealdb_amd.prefilter_i6_row(x, n) for x, n in zip(X, nm)]
    codes = np.stack([r[0] for r in rows]).astype(np.int64)
    scale = np.array([r[1] for r in rows], dtype=np.float32)
    eps = np.array([r[2] for r in rows], dtype=np.float32)
    cq, sq, rho_q, _ = surrealdb_amd.prefilter_q12(q)
    n = (codes @ cq.astype(np.int64)).astype(np.float32)  # exact integers
    qn = norms_f64(q.reshape(1, -1))[0]
    pscale = (scale.astype(np.float64) / nm).astype(np.float32)
    qscale = np.float32(np.float64(sq) / qn)
    qeps = round_up_f32(1.01 * np.float64(rho_q))
    one = np.float32(1.0)
    a = one - (n * pscale) * qscale
    e = eps + (one + eps) * qeps
    assert a.dtype == np.float32 and e.dtype == np.float32
    return (a - e).astype(np.float64), (a + e).astype(np.float64)


BOUNDS = {"bf16": bounds_bf16, "int8": bounds_i8, "int6": bounds_i6}


def candidates(lo, up, rows, k):
    """The rule with its threshold over `rows`: those of `rows` whose lower
    bound does not exceed the Kth smallest upper bound among `rows` (+inf
    when there are fewer than K)."""
    u = np.sort(up[rows])
    thr = u[k - 1] if u.size >= k else np.inf
    return rows[lo[rows] <= thr], thr


@pytest.fixture(scope="module", params=[0x5DB1, 0x77])
def case(request):
    """A seeded corpus and query, the exact distances, each tier's bounds,
    and the masks: random ones, and one whose best allowed row ranks behind
    a thousand disallowed ones."""
    X = oracle.gen_f32(request.param, 0, N, D)
    q = oracle.gen_f32(0xBEEF + request.param, 0, 1, D)[0]
    exact = np.array([oracle.dist_f32("cosine", q, np.ascontiguousarray(x))
                      for x in X])
    order = np.argsort(exact, kind="stable")
    masks = {}
    for seed, p in ((1, 0.5), (2, 0.02), (3, 0.002)):
        masks[f"random_{p}"] = np.random.default_rng(seed).random(N) < p
    behind = np.zeros(N, bool)
    behind[order[1000:]] = True
    behind &= np.random.default_rng(4).random(N) < 0.5
    masks["behind_1000"] = behind
    bounds = {t: BOUNDS[t](q, X) for t in TIER_NAMES}
    return X, q, exact, order, masks, bounds


@pytest.mark.parametrize("tier", TIER_NAMES)
def test_bounds_hold(case, tier):
    """The premise: every row's exact distance lies inside its bounds."""
    _, _, exact, _, _, bounds = case
    lo, up = bounds[tier]
    assert np.all(lo <= exact) and np.all(exact <= up)


@pytest.mark.parametrize("tier", TIER_NAMES)
def test_subset_threshold_keeps_the_subset_top_k(case, tier):
    X, q, exact, _, masks, bounds = case
    lo, up = bounds[tier]
    for name, allow in masks.items():
        rows = np.flatnonzero(allow)
        oids, odists = oracle.topk_f32(
            "cosine", np.ascontiguousarray(X[rows]), q, K)
        top = rows[oids.astype(np.int64)]
        assert np.array_equal(odists, exact[top])
        cand, thr = candidates(lo, up, rows, K)
        print(f"{tier} {name}: {rows.size} allowed, threshold {thr:.4f}, "
              f"{cand.size} candidates")
        assert top.size == min(K, rows.size)
        assert np.all(np.isin(top, cand)), f"{tier} {name}: a top row is lost"
        # ties included: every allowed row at the Kth distance is there too
        if top.size == K:
            tied = rows[exact[rows] <= odists[-1]]
            assert np.all(np.isin(tied, cand))


@pytest.mark.parametrize("tier", TIER_NAMES)
def test_whole_table_threshold_would_lose_rows(case, tier):
    """With the threshold taken over every row of the table, the mask whose
    best allowed row ranks behind a thousand disallowed ones passes fewer
    than K allowed rows: the threshold has to come from the subset."""
    _, _, _, _, masks, bounds = case
    lo, up = bounds[tier]
    rows = np.flatnonzero(masks["behind_1000"])
    assert rows.size >= 10 * K
    every = np.arange(N)
    table_thr = candidates(lo, up, every, K)[1]
    passed = rows[lo[rows] <= table_thr]
    print(f"{tier}: table threshold {table_thr:.4f} passes {passed.size} of "
          f"{rows.size} allowed rows")
    assert passed.size < K
    assert candidates(lo, up, rows, K)[0].size >= K
