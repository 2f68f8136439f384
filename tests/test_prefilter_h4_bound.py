"""The two-stage int6 prefilter's H-only bound and its selection rule, checked
on the CPU.

The first stage reads only the high nibbles h = (code + 32) >> 2 of the int6
shadow row and lets scale * (4 h + 1.5 - 32) stand for the element. The
library's row (codes_h, scale, eps4, xsum_h from sdbv_prefilter_h4_row), the
12-bit query (sdbv_prefilter_q12) and the stream's arithmetic (three biased
digit sums in wrapping u32, the bias removal N4 = 8 sum h qu - 8 * 2048
xsum_h - 61 sum cq, the f32 finish a = 1 - f32(N4) * (pscale / 2) * qscale
and the f32 bound e = eps4 + (1 + eps4) * qeps) are restated in numpy and
compared with the oracle's exact cosine distance: it must lie inside
[a - e, a + e] as the kernel rounds them, for every row and every query. The
nibbles and xsum_h must equal the restatement exactly.

The selection rule is restated too: T = the largest exact distance of ANY K
rows, then the H-only test, then the int6 test; the survivors must hold the
oracle's top-K, ties at the Kth place included."""
import numpy as np
import pytest

import oracle
import surrealdb_amd
from test_prefilter_i6_bound import (DIMS, bounds as bounds_i6, d_pad,
                                     lib_rows as lib_rows_i6, norms_f64,
                                     np_quantise, round_up_f32)


def lib_rows_h4(X):
    """(codes_h [m, d] int64, scale [m], eps4 [m], xsum_h [m]) from the
    library."""
    with np.errstate(all="ignore"):
        nm = norms_f64(X)
    out = [surrealdb_amd.prefilter_h4_row(x, n) for x, n in zip(X, nm)]
    return (np.stack([o[0] for o in out]).astype(np.int64),
            np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float32),
            np.array([o[3] for o in out], dtype=np.int64))


def digit_dot_h4(h, xsum_h, cq, qs):
    """The H-only stream's integer arithmetic for every row, in wrapping u32:
    three digit sums over the padded nibbles, then the bias removal. Returns
    N4 = sum (8 h - 61) cq as int32 values."""
    m, d = h.shape
    dp = d_pad(d)
    hp = np.full((m, dp), 8, dtype=np.uint32)
    hp[:, :d] = h.astype(np.uint32)
    qu = np.full(dp, 2048, dtype=np.uint32)
    qu[:d] = (cq + 2048).astype(np.uint32)
    assert hp.max() <= 15 and qu.min() >= 1 and qu.max() <= 4095
    assert np.array_equal(hp.sum(axis=1, dtype=np.int64), xsum_h)
    assert int(qu.sum(dtype=np.int64)) == qs
    q2, q1, q0 = qu >> 8, (qu >> 4) & 15, qu & 15
    u32 = np.uint32
    with np.errstate(over="ignore"):
        a = [(hp * q).sum(axis=1, dtype=np.uint32) for q in (q2, q1, q0)]
        sh = u32(256) * a[0] + u32(16) * a[1] + a[2]
        bias4 = u32((61 * (2048 * dp - qs)) % 2 ** 32)
        n32 = u32(8) * sh - u32(16384) * xsum_h.astype(np.uint32) + bias4
    # the ranges written above pf_i6_row
    exact_sh = (hp.astype(np.int64) * qu.astype(np.int64)).sum(1)
    assert np.array_equal(sh.astype(np.int64), exact_sh)
    assert exact_sh.max() < 2 ** 28
    n4 = n32.view(np.int32)
    assert np.abs(n4.astype(np.int64)).max() < 2 ** 30
    return n4


def bounds_h4(q, X, check_quantisers=True):
    """(exact [m] f64, lower [m] f32, upper [m] f32, e [m], rho4 [m]) for
    every row of X against q, the approximate side restated from the
    library's nibbles as k_prefilter_i6<false, true> computes it."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    h, scale, eps4, xsum_h = lib_rows_h4(X)
    cq, sq, rho_q, qs = surrealdb_amd.prefilter_q12(q)
    cq = cq.astype(np.int64)
    m, d = X.shape
    if check_quantisers:
        codes6, scale6, _, _ = lib_rows_i6(X)
        for i in range(m):
            want_c, want_s, _ = np_quantise(X[i], 31)
            assert np.array_equal(h[i], (want_c + 32) >> 2)
            assert np.array_equal(h[i], (codes6[i] + 32) >> 2)
            assert scale[i].view(np.uint32) == want_s.view(np.uint32)
            assert scale[i].view(np.uint32) == scale6[i].view(np.uint32)
            assert xsum_h[i] == int(h[i].sum()) + 8 * (d_pad(d) - d)
    n4 = digit_dot_h4(h, xsum_h, cq, qs)
    assert np.array_equal(n4.astype(np.int64), (8 * h - 61) @ cq)
    xn = norms_f64(X)
    qn = norms_f64(q.reshape(1, -1))[0]
    pscale = (scale.astype(np.float64) / xn).astype(np.float32)
    half = pscale * np.float32(0.5)
    assert np.array_equal(half.astype(np.float64),
                          pscale.astype(np.float64) / 2,
                          equal_nan=True)                 # exact in f32
    qscale = np.float32(np.float64(sq) / qn)
    qeps = round_up_f32(1.01 * np.float64(rho_q))
    one = np.float32(1.0)
    a = one - (n4.astype(np.float32) * half) * qscale
    e = eps4 + (one + eps4) * qeps
    assert a.dtype == np.float32 and e.dtype == np.float32
    exact = np.array([oracle.dist_f32("cosine", q, np.ascontiguousarray(x))
                      for x in X])
    r = X.astype(np.float64) \
        - scale.astype(np.float64)[:, None] * (4 * h + 1.5 - 32)
    rho4 = np.sqrt(np.sum(r * r, axis=1)) / xn
    cov = np.isfinite(scale)
    assert np.all(eps4[cov] > rho4[cov]) and np.all(eps4[~cov] == 0.0)
    return exact, a - e, a + e, e, rho4


def assert_inside(tag, exact, lo, up, e):
    a = (lo.astype(np.float64) + up.astype(np.float64)) / 2
    err = np.abs(exact - a)
    print(f"{tag}: max err = {err.max():.3e}, max err/e = "
          f"{(err / e).max():.3f}, e {e.min():.3e}..{e.max():.3e}")
    assert np.all(lo.astype(np.float64) <= exact)
    assert np.all(exact <= up.astype(np.float64))


def test_nibbles_match_numpy_restatement():
    for d in DIMS:
        X = oracle.gen_f32(0x16 + d, 0, 24, d)
        sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
        X = X * sc[np.arange(24) % sc.size, None]
        # the extremes of the code range: nibbles 0 and 15
        X[0, :4] = np.float32([31.0, -31.0, 0.5, 1.5])
        X[0, 4:] = np.float32(0.25)
        q = oracle.gen_f32(0x17 + d, 0, 1, d)[0]
        bounds_h4(q, X)  # asserts nibbles, scales, xsum_h and the digit sums
        h = lib_rows_h4(X)[0]
        assert h[0, 0] == 15 and h[0, 1] == 0 and h[0, 2] == 8


def test_uncovered_rows_carry_no_bound():
    d = 16
    X = oracle.gen_f32(0x19, 0, 5, d)
    X[0] = 0.0
    X[1, 3] = np.nan
    X[2, 0] = np.inf
    X[3] = 1e-40
    X[4, 1] = 3e38
    h, scale, eps4, xsum_h = lib_rows_h4(X)
    assert np.all(np.isnan(scale)) and np.all(eps4 == 0.0)
    assert np.all(h == 8) and np.all(xsum_h == 8 * d_pad(d))


def row_kinds(d, rng):
    """Uniform, Gaussian, one-hot and constant rows, and rows with norms at
    both ends of the window [2^-30, 2^30]."""
    X = np.empty((12, d), dtype=np.float32)
    X[0:3] = oracle.gen_f32(0x5DB1, 0, 3, d)
    X[3:6] = rng.standard_normal((3, d)).astype(np.float32)
    X[6] = 0.0
    X[6, rng.integers(d)] = 7.0                      # one-hot
    X[7] = 0.0
    X[7, rng.integers(d)] = -1e-3
    X[8] = 2.5                                       # constant
    X[9] = -1e-4
    base = oracle.gen_f32(0x30, 0, 2, d).astype(np.float64)
    bn = norms_f64(base.astype(np.float32))
    X[10] = (base[0] * (2.0 ** -30 * 1.01 / bn[0])).astype(np.float32)
    X[11] = (base[1] * (2.0 ** 30 * 0.99 / bn[1])).astype(np.float32)
    return X


@pytest.mark.parametrize("d", DIMS)
def test_bound_row_kinds(d):
    rng = np.random.default_rng(100 + d)
    X = row_kinds(d, rng)
    assert np.all(np.isfinite(lib_rows_h4(X)[1]))     # every row is covered
    qs = [oracle.gen_f32(0xBEEF, 0, 1, d)[0],
          rng.standard_normal(d).astype(np.float32),
          X[6].copy(), X[8].copy(),
          oracle.gen_f32(0xBEEF, 1, 1, d)[0] * np.float32(2.0 ** -17),
          oracle.gen_f32(0xBEEF, 2, 1, d)[0] * np.float32(2.0 ** 19)]
    for j, q in enumerate(qs):
        exact, lo, up, e, _ = bounds_h4(q, X, check_quantisers=(j == 0))
        assert_inside(f"d={d} kinds q{j}", exact, lo, up, e)


@pytest.mark.parametrize("d", DIMS)
def test_bound_random(d):
    m = 64 if d < 4096 else 16
    X = oracle.gen_f32(0x5DB1, 0, m, d)
    sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
    X = X * sc[np.arange(m) % sc.size, None]
    for j, qscale in enumerate([1.0, 2.0 ** -17, 2.0 ** 19]):
        q = oracle.gen_f32(0xBEEF, j, 1, d)[0] * np.float32(qscale)
        exact, lo, up, e, _ = bounds_h4(q, X, check_quantisers=(j == 0))
        assert_inside(f"d={d} random q{j}", exact, lo, up, e)


@pytest.mark.parametrize("d", DIMS)
def test_bound_largest_residual(d):
    """One element carries the scale, every other one is -0.501 steps: code
    -1, stored 31, nibble 7 with the low pair 3, so the approximant is -2.5
    steps and the truncation residual 1.999 steps per element, as large as
    the layout allows, on a row whose norm the small elements barely raise:
    rho4 = 2 sqrt(d - 1) / sqrt(961 + (d - 1) / 4), 1.63 at d = 768 and 2.9
    at 4096, above the 1.04 up to which the finish's rounding count holds as
    it stands and beyond which it leans on the slack of the factor 1.01. The
    query has one sign throughout, so the errors pull one way."""
    rng = np.random.default_rng(3000 + d)
    step = np.float32(2.0 ** -3)
    sign = rng.choice([-1.0, 1.0], size=d).astype(np.float32)
    x = np.full(d, np.float32(-0.501) * step, dtype=np.float32)
    x[rng.integers(d)] = np.float32(31.0) * step
    q = np.abs(oracle.gen_f32(0xBEEF, 3, 1, d)[0]) + np.float32(1.0)
    for tag, xx, qq in (("coherent", x, q), ("signed", x * sign, q * sign),
                        ("against", x, -q)):
        X = xx.reshape(1, -1)
        exact, lo, up, e, rho4 = bounds_h4(qq, X)
        print(f"d={d} {tag}: rho4 = {rho4[0]:.4f}")
        assert_inside(f"d={d} largest residual, {tag}", exact, lo, up, e)
    if d >= 768:
        assert rho4[0] > 1.04


def test_selection_rule_keeps_the_top_k():
    """T from the exact distances of any K rows, then the H-only test, then
    the int6 test: the survivors hold every row at or under the oracle's Kth
    distance. Duplicated rows tie at the Kth place; uncovered rows pass both
    tests."""
    n, d, k = 3000, 36, 10
    rng = np.random.default_rng(7)
    X = oracle.gen_f32(0x5E1, 0, n, d)
    q = oracle.gen_f32(0x5E2, 0, 1, d)[0]
    exact0 = np.array([oracle.dist_f32("cosine", q, x) for x in X])
    order = np.argsort(exact0, kind="stable")
    kth_row = order[k - 1]
    for r in (5, 1234, n - 1):        # ties straddling the Kth place
        X[r] = X[kth_row]
    X[17] = 0.0                       # uncovered: zero norm
    X[18, 3] = np.nan                 # uncovered: not finite
    with np.errstate(all="ignore"):
        exact, lo4, up4, _, _ = bounds_h4(q, X, check_quantisers=False)
        covered = np.isfinite(lib_rows_h4(X)[1])
    # the int6 restatement takes covered rows only
    lo6 = np.full(n, -np.inf, dtype=np.float32)
    lo6[covered] = bounds_i6(q, X[covered], check_quantisers=False)[1]
    oids, odists = oracle.topk_f32("cosine", X, q, k)
    dk = odists[k - 1]
    must = np.flatnonzero(exact <= dk)
    assert must.size >= k + 2         # the duplicates tie with the Kth row
    assert set(oids.astype(np.int64)) <= set(must)
    cov = np.flatnonzero(covered)
    picks = [cov[np.argsort(up4[cov], kind="stable")[:k]],  # as the kernel
             cov[np.argsort(exact[cov], kind="stable")[:k]],  # the tightest T
             rng.choice(cov, size=k, replace=False),
             rng.choice(cov, size=k, replace=False)]
    for rows in picks:
        T = exact[rows].max()
        assert T >= dk
        with np.errstate(invalid="ignore"):
            s1 = ~covered | ~(lo4.astype(np.float64) > T)
            s2 = s1 & (~covered | ~(lo6.astype(np.float64) > T))
        print(f"T = {T:.6f}: stage 1 keeps {int(s1.sum())}, stage 2 "
              f"{int(s2.sum())} of {n}")
        assert np.all(s2[must])
        assert s2[17] and s2[18]
        assert s2.sum() <= s1.sum()
    # the kernel's pick is far tighter than a random one
    T = exact[picks[0]].max()
    assert int((~(lo4[cov].astype(np.float64) > T)).sum()) < n // 2
