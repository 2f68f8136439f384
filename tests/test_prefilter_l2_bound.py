"""The euclidean (l2) prefilter tier's per-row interval, checked on the CPU.

The shadow row (codes, scale, xx, res from the library's own
sdbv_prefilter_l2_row) is restated in numpy and must agree bit for bit; the
interval [lo, up] of sdbv_prefilter_l2_interval, which runs the stream
kernel's FMA chain and finish on one row, must hold the oracle's exact
euclidean distance on random rows of very different lengths, on a query equal
to the row, on a query within 1e-6 of it (the cancellation case, where the
rounding term delta rules), on rows with one dominant element, on constant
rows and on rows whose quantisation errors all pull the same way."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

DIMS = [4, 16, 20, 128, 768, 4096]      # the quantiser, as for int8
BOUND_DIMS = [4, 20, 768, 4096]
PF_CAND_CAP = 16384
RES_ABS = 2.0 ** -68


def round_up_f32(e):
    f = np.float32(e)
    if np.float64(f) < e:
        f = (f.view(np.uint32) + np.uint32(1)).view(np.float32)
    return f


def np_row(x):
    """Restatement of pf_l2_row for a covered row: scale = f32(maxabs / 127)
    with the division in f64, codes = rint(x / scale) in f64 (ties to even)
    clamped to +-127 (all zero when the scale is zero), xx and res from the
    sequential f64 sums of (scale c)^2 and (x - scale c)^2."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    scale = np.float32(np.float64(np.max(np.abs(x))) / 127.0)
    xd, sd = x.astype(np.float64), np.float64(scale)
    if sd > 0.0:
        c = np.clip(np.rint(xd / sd), -127, 127)
    else:
        c = np.zeros_like(xd)
    xh = sd * c
    r = xd - xh
    xx2 = np.cumsum(xh * xh)[-1]             # cumsum: the sequential order
    res2 = np.cumsum(r * r)[-1]
    res = round_up_f32(np.sqrt(res2) * (1.0 + 2.0 ** -40) + RES_ABS)
    return c.astype(np.int8), scale, np.float32(xx2), res


def lib_rows(X):
    out = [surrealdb_amd.prefilter_l2_row(x) for x in X]
    return (np.stack([o[0] for o in out]),
            np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float32),
            np.array([o[3] for o in out], dtype=np.float32))


def residual_f64(X, codes, scale):
    r = X.astype(np.float64) - scale.astype(np.float64)[:, None] * codes
    return np.sqrt(np.sum(r * r, axis=1))


def intervals(q, rows):
    codes, scale, xx, res = rows
    lu = [surrealdb_amd.prefilter_l2_interval(q, codes[i], scale[i], xx[i],
                                              res[i])
          for i in range(codes.shape[0])]
    return (np.array([a for a, _ in lu], dtype=np.float32),
            np.array([b for _, b in lu], dtype=np.float32))


def exact_dist(q, X):
    q = np.ascontiguousarray(q, dtype=np.float32)
    return np.array([oracle.dist_f32("euclidean", q, np.ascontiguousarray(x))
                     for x in X])


def check(label, q, X, rows=None):
    """lo <= exact <= up for every row of X; returns (lo, up, exact)."""
    rows = lib_rows(X) if rows is None else rows
    assert not np.isnan(rows[1]).any(), "every row here must be covered"
    lo, up = intervals(q, rows)
    ex = exact_dist(q, X)
    width = (up.astype(np.float64) - lo) / np.maximum(ex, 1e-300)
    print(f"{label}: exact {ex.min():.3e}..{ex.max():.3e}, "
          f"(up - lo) / exact {width.min():.3e}..{width.max():.3e}, "
          f"min slack lo {np.min(ex - lo):.3e} up {np.min(up - ex):.3e}")
    assert np.all(lo >= 0.0)
    assert np.all(lo.astype(np.float64) <= ex), label
    assert np.all(ex <= up.astype(np.float64)), label
    return lo, up, ex


def scaled_rows(seed, m, d):
    X = oracle.gen_f32(seed, 0, m, d)
    sc = np.float32(2.0) ** np.arange(-20, 21, dtype=np.float32)
    s = sc[np.arange(m) % sc.size]
    return X * s[:, None], s


def test_quantiser_matches_numpy_restatement():
    for d in DIMS:
        X, _ = scaled_rows(0x18 + d, 48, d)
        # exact rounding midpoints and the extremes of the code range
        X[0, :4] = np.float32([127.0, -63.5, 0.5, 1.5])
        X[0, 4:] = np.float32(0.25)
        X[1, :4] = np.float32([-254.0, 253.0, 1.0, -3.0])
        X[1, 4:] = np.float32(-0.75)
        X[2] = 0.0                      # the zero row is covered
        X[3] = 1e-44                    # a scale that rounds to zero
        X[4] = 1e-40                    # subnormal scale
        codes, scale, xx, res = lib_rows(X)
        for i in range(X.shape[0]):
            c, s, x2, r = np_row(X[i])
            assert np.array_equal(codes[i], c), (d, i)
            assert scale[i].view(np.uint32) == s.view(np.uint32), (d, i)
            assert xx[i].view(np.uint32) == x2.view(np.uint32), (d, i)
            assert res[i].view(np.uint32) == r.view(np.uint32), (d, i)
        big = np.abs(codes.astype(np.int32)).max(axis=1)
        assert np.all(big[[0, 1]] == 127) and np.all(big[5:] == 127)
        assert scale[2] == 0.0 and xx[2] == 0.0 and not codes[2].any()
        assert scale[3] == 0.0 and not codes[3].any()
        # res is at least the f64 residual (and carries the 2^-68 on top)
        assert np.all(res.astype(np.float64)
                      >= residual_f64(X, codes, scale) + RES_ABS * 0.999)
    assert list(lib_rows(X)[0][0, :4]) == [127, -64, 0, 2]  # ties to even


def test_uncovered_rows_carry_no_bound():
    d = 16
    X = oracle.gen_f32(0x19, 0, 5, d)
    X[0, 3] = np.nan
    X[1, 0] = np.inf
    X[2, 7] = -np.inf
    X[3, 1] = 3e38                      # finite, the norm leaves the window
    X[4] = 2.0 ** 29                    # finite, norm 2^31 > 2^30
    q = oracle.gen_f32(0x1A, 0, 1, d)[0]
    for x in X:
        codes, scale, xx, res = surrealdb_amd.prefilter_l2_row(x)
        assert np.isnan(scale) and xx == 0.0 and res == 0.0
        assert not codes.any()          # neutral codes: stored byte 128
        lo, up = surrealdb_amd.prefilter_l2_interval(q, codes, scale, xx, res)
        assert lo == -np.inf and up == np.inf


def test_queries_outside_the_window_are_refused():
    d = 16
    x = oracle.gen_f32(0x1B, 0, 1, d)[0]
    row = surrealdb_amd.prefilter_l2_row(x)
    for bad in (np.nan, np.inf, 3e38):
        q = oracle.gen_f32(0x1C, 0, 1, d)[0]
        q[5] = bad
        with pytest.raises(surrealdb_amd.SdbvError):
            surrealdb_amd.prefilter_l2_interval(q, *row)


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_random(d):
    m = 82 if d < 4096 else 41
    X, s = scaled_rows(0x5DB1, m, d)
    q = oracle.gen_f32(0xBEEF, 0, 1, d)[0]
    rows = lib_rows(X)
    check(f"d={d} query of unit scale", q, X, rows)
    check(f"d={d} zero query", np.zeros(d, dtype=np.float32), X, rows)
    # a query at each row's own scale: distances of the row's magnitude
    for i in range(0, m, 5):
        one = tuple(a[i:i + 1] for a in rows)
        check(f"d={d} row {i} at scale 2^{np.log2(s[i]):.0f}", q * s[i],
              X[i:i + 1], one)


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_query_equals_row(d):
    X, _ = scaled_rows(0x71, 41, d)
    rows = lib_rows(X)
    for i in range(X.shape[0]):
        one = tuple(a[i:i + 1] for a in rows)
        lo, up, ex = check(f"d={d} q = row {i}", X[i].copy(), X[i:i + 1], one)
        assert ex[0] == 0.0 and lo[0] == 0.0


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_query_next_to_row(d):
    """q = x (1 + 1e-6 u): D is a millionth of |x| while |x^|^2, |q|^2 and
    2 x^.q cancel to it from values near |x|^2, so A2 is mostly rounding
    error and only delta keeps the interval honest."""
    rng = np.random.default_rng(300 + d)
    X, _ = scaled_rows(0x72, 41, d)
    rows = lib_rows(X)
    for i in range(X.shape[0]):
        u = rng.uniform(-1.0, 1.0, size=d)
        q = (X[i].astype(np.float64) * (1.0 + 1e-6 * u)).astype(np.float32)
        one = tuple(a[i:i + 1] for a in rows)
        check(f"d={d} q next to row {i}", q, X[i:i + 1], one)


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_one_dominant_element(d):
    """One element carries the scale, every other one lies just under half a
    step and gets code 0: the residual is as large as this d allows."""
    rng = np.random.default_rng(d)
    X = np.empty((8, d), dtype=np.float32)
    for i in range(8):
        x = (0.49 * rng.choice([-1.0, 1.0], size=d)).astype(np.float32)
        x[rng.integers(d)] = 127.0 if i % 2 else -127.0    # scale = 1
        X[i] = x * np.float32(2.0 ** (3 * i - 10))
    rows = lib_rows(X)
    assert np.all(np.sum(rows[0] != 0, axis=1) == 1)
    for q in (np.sign(X[0]).astype(np.float32),
              oracle.gen_f32(0xBEEF, 2, 1, d)[0], X[3].copy()):
        check(f"d={d} dominant element", q, X, rows)


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_constant_row(d):
    X = np.empty((4, d), dtype=np.float32)
    for i, v in enumerate((2.5, -1e-3, 7e5, 1.0)):
        X[i] = v
    rows = lib_rows(X)
    assert np.all(np.abs(rows[0].astype(np.int32)) == 127)
    for q in (oracle.gen_f32(0xBEEF, 3, 1, d)[0], X[0].copy(),
              np.full(d, 2.4999, dtype=np.float32)):
        check(f"d={d} constant row", q, X, rows)


@pytest.mark.parametrize("d", BOUND_DIMS)
def test_bound_worst_case_coherent(d):
    """Every element but the one that sets the scale sits just under a
    rounding midpoint, and the query lies along the residual: x^ - x and
    q - x^ point the same way, so |D - D^| comes close to the residual and
    the triangle bound is nearly tight on one side."""
    rng = np.random.default_rng(2000 + d)
    step = np.float32(2.0 ** -3)
    n_k = rng.integers(0, 126, size=d).astype(np.float32)
    x = (n_k + np.float32(0.499)) * step
    x[rng.integers(d)] = np.float32(127.0) * step     # scale = step exactly
    x = x * rng.choice([-1.0, 1.0], size=d).astype(np.float32)
    X = x.reshape(1, -1)
    rows = lib_rows(X)
    assert rows[1][0] == step
    xh = rows[1][0] * rows[0][0].astype(np.float32)
    resid = residual_f64(X, rows[0], rows[1])[0]
    for t in (-3.0, -1.0, 0.5, 2.0):                  # q = x^ + t (x - x^)
        q = (xh + np.float32(t) * (x - xh)).astype(np.float32)
        lo, up, ex = check(f"d={d} coherent t={t}", q, X, rows)
        # D^ = |t| resid and D = |1 - t| resid, a few thousandths of |x|: at
        # small d the interval's width is twice the residual, at large d the
        # FMA chain's worst-case term (d + 2) u 255 |q|_1 scale adds to it
        print(f"  width / residual = {(up[0] - lo[0]) / resid:.3f}")
        if d <= 20:
            assert up[0] - lo[0] <= 2.2 * resid


def test_candidate_count_stays_under_the_cap():
    """lo_i <= the K-th smallest up over 50 000 x 768 uniform rows at k = 10:
    a numpy model of the bare triangle bound, without the rounding terms,
    gives 30 candidates there."""
    n, d, k = 50_000, 768, 10
    X = oracle.gen_f32(0x5DB1, 0, n, d)
    q = oracle.gen_f32(0xBEEF, 1, 1, d)[0]
    lo = np.empty(n, dtype=np.float32)
    up = np.empty(n, dtype=np.float32)
    for i in range(n):
        row = surrealdb_amd.prefilter_l2_row(X[i])
        lo[i], up[i] = surrealdb_amd.prefilter_l2_interval(q, *row)
    u_k = np.partition(up, k - 1)[k - 1]
    count = int(np.sum(lo <= u_k))
    print(f"candidates at {n} x {d}, k = {k}: {count}")
    assert k <= count <= PF_CAND_CAP
