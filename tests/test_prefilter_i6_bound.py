"""The int6 prefilter tier's bound, checked on the CPU.

The int6 shadow row (codes, scale, eps, xsum from the library's own
sdbv_prefilter_i6_row), the 12-bit query (codes, sq, rho_q, Qs from
sdbv_prefilter_q12) and the prefilter's arithmetic (biased digit sums in
wrapping u32, the bias removal, the f32 finish and the f32 bound
e = eps + (1 + eps) * qeps) are restated in numpy and compared with the
oracle's exact cosine distance: the exact distance must lie inside
[a - e, a + e] as the kernel rounds them, for every row and every query.
Both quantisers are restated too and must reproduce the library's codes,
xsum and Qs exactly."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

DIMS = [4, 16, 20, 36, 128, 768, 4096]
NAN32 = np.float32(np.nan)


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


def d_pad(d):
    return -(-d // 32) * 32


def np_quantise(x, levels):
    """Restatement of both quantisers: scale = f32(maxabs / levels) with the
    division in f64, codes = rint(x / scale) in f64 (ties to even), clamped
    to +-levels. Returns (codes int64, scale f32, sum of the biased codes
    over the padded vector), bias = levels + 1."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    scale = np.float32(np.float64(np.max(np.abs(x))) / levels)
    c = np.rint(x.astype(np.float64) / np.float64(scale))
    c = np.clip(c, -levels, levels).astype(np.int64)
    total = int(np.sum(c + levels + 1)) + (levels + 1) * (d_pad(x.size)
                                                          - x.size)
    return c, scale, total


def lib_rows(X):
    """(codes [m, d] int64, scale [m], eps [m], xsum [m]) from the library."""
    nm = norms_f64(X)
    out = [surrealdb_amd.prefilter_i6_row(x, n) for x, n in zip(X, nm)]
    return (np.stack([o[0] for o in out]).astype(np.int64),
            np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float32),
            np.array([o[3] for o in out], dtype=np.int64))


def round_up_f32(e):
    f = np.float32(e)
    if np.float64(f) < e:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def digit_dot(codes, xsum, cq, qs):
    """The kernel's integer arithmetic for every row, in wrapping u32: six
    digit sums over the padded, biased codes (high nibble and low pair of
    the row against the query's three nibbles), S, then the bias removal.
    Returns sum c * cq as int32 values."""
    m, d = codes.shape
    dp = d_pad(d)
    xu = np.full((m, dp), 32, dtype=np.uint32)
    xu[:, :d] = (codes + 32).astype(np.uint32)
    qu = np.full(dp, 2048, dtype=np.uint32)
    qu[:d] = (cq + 2048).astype(np.uint32)
    assert xu.min() >= 1 and xu.max() <= 63 and qu.min() >= 1 \
        and qu.max() <= 4095
    assert np.array_equal(xu.sum(axis=1, dtype=np.int64), xsum)
    assert int(qu.sum(dtype=np.int64)) == qs
    h, l = xu >> 2, xu & 3
    q2, q1, q0 = qu >> 8, (qu >> 4) & 15, qu & 15
    u32 = np.uint32
    with np.errstate(over="ignore"):
        a = [(p * q).sum(axis=1, dtype=np.uint32)
             for p in (h, l) for q in (q2, q1, q0)]
        s = (u32(4) * (u32(256) * a[0] + u32(16) * a[1] + a[2])
             + u32(256) * a[3] + u32(16) * a[4] + a[5])
        bias = u32((65536 * dp - 32 * qs) % 2 ** 32)
        n32 = s - u32(2048) * xsum.astype(np.uint32) + bias
    # nothing wrapped on the way to S
    assert np.array_equal(s.astype(np.int64),
                          (xu.astype(np.int64) * qu.astype(np.int64)).sum(1))
    return n32.view(np.int32)


def bounds(q, X, check_quantisers=True):
    """(exact [m] f64, lower [m] f32, upper [m] f32, eps [m], rho_x [m],
    rho_q) for every row of X against q, the approximate side restated from
    the library's codes as k_prefilter_i6 computes it."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    codes, scale, eps, xsum = lib_rows(X)
    cq, sq, rho_q, qs = surrealdb_amd.prefilter_q12(q)
    cq = cq.astype(np.int64)
    if check_quantisers:
        for i in range(X.shape[0]):
            want_c, want_s, want_sum = np_quantise(X[i], 31)
            assert np.array_equal(codes[i], want_c)
            assert scale[i].view(np.uint32) == want_s.view(np.uint32)
            assert xsum[i] == want_sum
        want_c, want_s, want_sum = np_quantise(q, 2047)
        assert np.array_equal(cq, want_c)
        assert sq.view(np.uint32) == want_s.view(np.uint32)
        assert qs == want_sum
    n = digit_dot(codes, xsum, cq, qs)
    assert np.array_equal(n.astype(np.int64), codes @ cq)  # exact integers
    xn = norms_f64(X)
    qn = norms_f64(q.reshape(1, -1))[0]
    # the query's residual, restated; the library's is rounded up
    rq = np.sqrt(np.sum((q.astype(np.float64) - np.float64(sq) * cq) ** 2)) \
        / qn
    assert rq <= np.float64(rho_q) <= rq * (1 + 1e-6) + 1e-45
    pscale = (scale.astype(np.float64) / xn).astype(np.float32)
    qscale = np.float32(np.float64(sq) / qn)
    qeps = round_up_f32(1.01 * np.float64(rho_q))
    one = np.float32(1.0)
    a = one - (n.astype(np.float32) * pscale) * qscale
    e = eps + (one + eps) * qeps
    assert a.dtype == np.float32 and e.dtype == np.float32
    exact = np.array([oracle.dist_f32("cosine", q, np.ascontiguousarray(x))
                      for x in X])
    r = X.astype(np.float64) - scale.astype(np.float64)[:, None] * codes
    rho_x = np.sqrt(np.sum(r * r, axis=1)) / xn
    assert np.all(eps > rho_x)
    return exact, a - e, a + e, e, rho_x, np.float64(rho_q)


def assert_inside(tag, exact, lo, up, e):
    a = (lo.astype(np.float64) + up.astype(np.float64)) / 2
    err = np.abs(exact - a)
    print(f"{tag}: max err = {err.max():.3e}, max err/e = "
          f"{(err / e).max():.3f}, e {e.min():.3e}..{e.max():.3e}")
    assert np.all(lo.astype(np.float64) <= exact)
    assert np.all(exact <= up.astype(np.float64))


def test_quantisers_match_numpy_restatement():
    for d in DIMS:
        X = oracle.gen_f32(0x16 + d, 0, 24, d)
        sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
        X = X * sc[np.arange(24) % sc.size, None]
        # exact rounding midpoints and the extremes of the code range
        X[0, :4] = np.float32([31.0, -15.5, 0.5, 1.5])
        X[0, 4:] = np.float32(0.25)
        X[1, :4] = np.float32([-62.0, 61.0, 1.0, -3.0])
        X[1, 4:] = np.float32(-0.75)
        q = oracle.gen_f32(0x17 + d, 0, 1, d)[0]
        q[:4] = np.float32([2047.0, -1023.5, 0.5, 1.5])
        q[4:] = np.clip(q[4:], -20, 20)
        bounds(q, X)  # asserts codes, scales, xsum, Qs and the digit sums
        codes = lib_rows(X)[0]
        assert np.all(np.abs(codes).max(axis=1) == 31)
    assert list(lib_rows(X)[0][0, :4]) == [31, -16, 0, 2]  # ties to even
    assert list(surrealdb_amd.prefilter_q12(q)[0][:4]) == [2047, -1024, 0, 2]


def test_uncovered_rows_carry_no_bound():
    d = 16
    X = oracle.gen_f32(0x19, 0, 5, d)
    X[0] = 0.0
    X[1, 3] = np.nan
    X[2, 0] = np.inf
    X[3] = 1e-40
    X[4, 1] = 3e38
    with np.errstate(all="ignore"):
        nm = norms_f64(X)
    for x, n in zip(X, nm):
        codes, scale, eps, xsum = surrealdb_amd.prefilter_i6_row(x, n)
        assert np.isnan(scale) and eps == 0.0 and not codes.any()
        assert xsum == 32 * d_pad(d)
    for x in X:  # the same vectors as queries: the prefilter never runs
        with np.errstate(all="ignore"):
            codes, sq, rho_q, qs = surrealdb_amd.prefilter_q12(x)
        assert np.isnan(sq) and rho_q == 0.0 and not codes.any()
        assert qs == 2048 * d_pad(d)


@pytest.mark.parametrize("d", DIMS)
def test_bound_random(d):
    m = 64 if d < 4096 else 16
    X = oracle.gen_f32(0x5DB1, 0, m, d)
    # rows of very different lengths: the bound is in cosine units
    sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
    X = X * sc[np.arange(m) % sc.size, None]
    for j, qscale in enumerate([1.0, 2.0 ** -17, 2.0 ** 19]):
        q = oracle.gen_f32(0xBEEF, j, 1, d)[0] * np.float32(qscale)
        exact, lo, up, e, _, _ = bounds(q, X)
        assert_inside(f"d={d} random q{j}", exact, lo, up, e)


@pytest.mark.parametrize("d", DIMS)
def test_bound_one_dominant_element(d):
    """One element carries the scale, every other one lies just under half a
    step and gets code 0: the residual is as large as this d allows, for
    rows (rho_x -> 0.49 sqrt(d - 1) / 31) and for a query built the same way
    (rho_q -> 0.49 sqrt(d - 1) / 2047)."""
    rng = np.random.default_rng(d)
    X = np.empty((8, d), dtype=np.float32)
    for i in range(8):
        x = (0.49 * rng.choice([-1.0, 1.0], size=d)).astype(np.float32)
        x[rng.integers(d)] = np.float32(31.0 if i % 2 else -31.0)  # scale 1
        X[i] = x * np.float32(2.0 ** (3 * i - 10))
    qd = (0.49 * rng.choice([-1.0, 1.0], size=d)).astype(np.float32)
    qd[rng.integers(d)] = np.float32(2047.0)
    qd = qd * np.float32(2.0 ** -5)
    R = oracle.gen_f32(0xD0, 0, 8, d)
    for tag, q, rows in (("sign", np.sign(X[0]).astype(np.float32), X),
                         ("random", oracle.gen_f32(0xBEEF, 2, 1, d)[0], X),
                         ("dominant q", qd, X),
                         ("dominant q, random rows", qd, R)):
        exact, lo, up, e, rho_x, rho_q = bounds(q, rows)
        assert_inside(f"d={d} dominant, q {tag}", exact, lo, up, e)
        if rows is X:
            assert np.all(np.sum(lib_rows(X)[0] != 0, axis=1) == 1)
            want = 0.49 * np.sqrt(d - 1) / np.sqrt(31.0 ** 2
                                                   + (d - 1) * 0.49 ** 2)
            assert np.all(np.abs(rho_x / want - 1.0) < 1e-3)
        if q is qd:
            want = 0.49 * np.sqrt(d - 1) / np.sqrt(2047.0 ** 2
                                                   + (d - 1) * 0.49 ** 2)
            assert abs(rho_q / want - 1.0) < 1e-3


@pytest.mark.parametrize("d", DIMS)
def test_bound_worst_case_coherent(d):
    """Every row element but the one that sets the scale sits just under a
    rounding midpoint, and so does every query element; the query has the
    row's signs and nearly equal magnitudes (2031..2047 steps). Every
    quantisation error of the row and of the query then pulls the same way,
    Cauchy-Schwarz on the row's residual is tight up to the one exact
    element and the query's spread (sqrt(3/4) * 2031/2047 = 0.859 at d = 4),
    so the error must reach 0.85 of rho_x and still stay under the bound."""
    rng = np.random.default_rng(2000 + d)
    step = np.float32(2.0 ** -3)
    n_k = rng.integers(0, 30, size=d).astype(np.float32)
    x = (n_k + np.float32(0.499)) * step
    x[rng.integers(d)] = np.float32(31.0) * step       # scale = step exactly
    sign = rng.choice([-1.0, 1.0], size=d).astype(np.float32)
    x = x * sign
    qstep = np.float32(2.0 ** -9)
    m_k = rng.integers(2031, 2046, size=d).astype(np.float32)
    q = (m_k + np.float32(0.499)) * qstep
    q[rng.integers(d)] = np.float32(2047.0) * qstep    # sq = qstep exactly
    q = q * sign
    X = x.reshape(1, -1)
    exact, lo, up, e, rho_x, rho_q = bounds(q, X)
    codes, scale, _, _ = lib_rows(X)
    assert scale[0] == step
    assert surrealdb_amd.prefilter_q12(q)[1] == qstep
    a = (np.float64(lo[0]) + np.float64(up[0])) / 2
    err = abs(exact[0] - a)
    print(f"d={d}: coherent err = {err:.6e}, rho_x = {rho_x[0]:.6e}, "
          f"rho_q = {rho_q:.6e}, e = {e[0]:.6e}")
    assert err >= 0.85 * rho_x[0]
    assert_inside(f"d={d} coherent", exact, lo, up, e)


@pytest.mark.parametrize("d", DIMS)
def test_bound_norm_window_ends(d):
    """Rows and queries with norms just inside both ends of [2^-30, 2^30]
    are covered and the bound holds for every pairing."""
    X = oracle.gen_f32(0x30, 0, 8, d)
    xn = norms_f64(X)
    f = np.where(np.arange(8) % 2 == 0, 2.0 ** -30 * 1.01, 2.0 ** 30 * 0.99)
    X = (X.astype(np.float64) * (f / xn)[:, None]).astype(np.float32)
    assert np.all(np.isfinite(lib_rows(X)[1]))
    for j, end in enumerate([2.0 ** -30 * 1.01, 2.0 ** 30 * 0.99]):
        q = oracle.gen_f32(0x31, j, 1, d)[0]
        q = (q.astype(np.float64)
             * (end / norms_f64(q.reshape(1, -1))[0])).astype(np.float32)
        assert np.isfinite(surrealdb_amd.prefilter_q12(q)[1])
        exact, lo, up, e, _, _ = bounds(q, X)
        assert_inside(f"d={d} window end {j}", exact, lo, up, e)
