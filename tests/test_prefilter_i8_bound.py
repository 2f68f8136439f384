"""The int8 prefilter tier's per-row error bound, checked on the CPU.

The int8 shadow row (codes, scale, eps from the library's own
sdbv_prefilter_i8_row) and the prefilter's f32 arithmetic are restated in
numpy and compared with the oracle's exact cosine distance:
|exact - approx| must stay under the ROW's eps on random rows of very
different lengths, on rows with one dominant element, and on rows built so
that every quantisation error pulls the same way. The quantiser itself is
restated too and must reproduce the library's codes exactly."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

DIMS = [4, 16, 20, 128, 768, 4096]


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


def np_quantise(x):
    """Restatement: scale = f32(maxabs / 127) with the division in f64,
    codes = rint(x / scale) in f64 (ties to even), clamped to +-127."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    scale = np.float32(np.float64(np.max(np.abs(x))) / 127.0)
    c = np.rint(x.astype(np.float64) / np.float64(scale))
    return np.clip(c, -127, 127).astype(np.int8), scale


def lib_rows(X):
    """(codes [m, d] int8, scale [m], eps [m]) from the library."""
    nm = norms_f64(X)
    out = [surrealdb_amd.prefilter_i8_row(x, n) for x, n in zip(X, nm)]
    return (np.stack([o[0] for o in out]),
            np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float32))


def approx_dist(q, X, codes, scale):
    """The int8 prefilter's approximate cosine distance of every row:
    t = the sequential f32 FMA chain over (code + 128) * q_k (the product of
    an 8-bit and a 24-bit number is exact in f64, so one f64 add rounded to
    f32 is the FMA), s = t - f32(128 sum q), a = 1 - s * inv_q * pscale."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    b = codes.astype(np.float64) + 128.0
    t = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(X.shape[1]):
        t = (t.astype(np.float64) + b[:, k] * np.float64(q[k])).astype(
            np.float32)
    qbias = np.float32(128.0 * np.sum(q.astype(np.float64)))
    pscale = (scale.astype(np.float64) / norms_f64(X)).astype(np.float32)
    inv_q = np.float32(1.0 / norms_f64(q.reshape(1, -1))[0])
    return np.float32(1.0) - (t - qbias) * inv_q * pscale


def exact_dist(q, X):
    return np.array([oracle.dist_f32("cosine", q, np.ascontiguousarray(x))
                     for x in X])


def rho(X, codes, scale):
    """Per-row relative residual |x - scale c| / |x| in f64."""
    r = X.astype(np.float64) - scale.astype(np.float64)[:, None] * codes
    return np.sqrt(np.sum(r * r, axis=1)) / norms_f64(X)


def test_quantiser_matches_numpy_restatement():
    for d in DIMS:
        X = oracle.gen_f32(0x18 + d, 0, 24, d)
        sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
        X = X * sc[np.arange(24) % sc.size, None]
        # exact rounding midpoints and the extremes of the code range
        X[0, :4] = np.float32([127.0, -63.5, 0.5, 1.5])
        X[0, 4:] = np.float32(0.25)
        X[1, :4] = np.float32([-254.0, 253.0, 1.0, -3.0])
        X[1, 4:] = np.float32(-0.75)
        codes, scale, eps = lib_rows(X)
        for i in range(X.shape[0]):
            want_c, want_s = np_quantise(X[i])
            assert np.array_equal(codes[i], want_c)
            assert scale[i].view(np.uint32) == want_s.view(np.uint32)
        assert np.all(np.abs(codes.astype(np.int32)).max(axis=1) == 127)
        assert np.all(eps > rho(X, codes, scale))
    assert list(lib_rows(X)[0][0, :4]) == [127, -64, 0, 2]  # ties to even


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
        codes, scale, eps = surrealdb_amd.prefilter_i8_row(x, n)
        assert np.isnan(scale) and eps == 0.0 and not codes.any()


@pytest.mark.parametrize("d", DIMS)
def test_bound_random(d):
    m = 64 if d < 4096 else 16
    X = oracle.gen_f32(0x5DB1, 0, m, d)
    # rows of very different lengths: the bound is in cosine units
    sc = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
    X = X * sc[np.arange(m) % sc.size, None]
    q = oracle.gen_f32(0xBEEF, 0, 1, d)[0]
    codes, scale, eps = lib_rows(X)
    err = np.abs(exact_dist(q, X)
                 - approx_dist(q, X, codes, scale).astype(np.float64))
    r = rho(X, codes, scale)
    print(f"d={d}: max err = {err.max():.3e}, max err/eps = "
          f"{(err / eps).max():.3f}, rho {r.min():.3e}..{r.max():.3e}, "
          f"eps {eps.min():.3e}..{eps.max():.3e}")
    assert np.all(err <= eps)


@pytest.mark.parametrize("d", DIMS)
def test_bound_one_dominant_element(d):
    """One element carries the scale, every other one lies just under half a
    step and gets code 0: the row's residual is as large as this d allows
    (rho -> sqrt(d - 1) / 254 of the dominant element's share)."""
    rng = np.random.default_rng(d)
    big = np.float32(127.0)                       # scale = 1
    X = np.empty((8, d), dtype=np.float32)
    for i in range(8):
        x = (0.49 * rng.choice([-1.0, 1.0], size=d)).astype(np.float32)
        x[rng.integers(d)] = big if i % 2 else -big
        X[i] = x * np.float32(2.0 ** (3 * i - 10))
    codes, scale, eps = lib_rows(X)
    assert np.all(np.sum(codes != 0, axis=1) == 1)
    r = rho(X, codes, scale)
    for q in (np.sign(X[0]).astype(np.float32),
              oracle.gen_f32(0xBEEF, 2, 1, d)[0]):
        err = np.abs(exact_dist(q, X)
                     - approx_dist(q, X, codes, scale).astype(np.float64))
        print(f"d={d}: dominant-element err max = {err.max():.3e}, rho = "
              f"{r.max():.3e}, eps = {eps.max():.3e}")
        assert np.all(err <= eps)
    want = 0.49 * np.sqrt(d - 1) / np.sqrt(127.0 ** 2 + (d - 1) * 0.49 ** 2)
    assert np.all(np.abs(r / want - 1.0) < 1e-3)


@pytest.mark.parametrize("d", DIMS)
def test_bound_worst_case_coherent(d):
    """Every element but the one that sets the scale sits just under a
    rounding midpoint, and q = sign(x): every quantisation error pulls the
    same way and Cauchy-Schwarz is tight up to the one exact element, so the
    error must reach 0.85 of rho (sqrt(3/4) = 0.866 at d = 4) and still stay
    under the row's bound."""
    rng = np.random.default_rng(2000 + d)
    step = np.float32(2.0 ** -3)
    n_k = rng.integers(0, 126, size=d).astype(np.float32)
    x = (n_k + np.float32(0.499)) * step
    x[rng.integers(d)] = np.float32(127.0) * step     # scale = step exactly
    x = x * rng.choice([-1.0, 1.0], size=d).astype(np.float32)
    X = x.reshape(1, -1)
    q = np.sign(x).astype(np.float32)
    codes, scale, eps = lib_rows(X)
    assert scale[0] == step
    r = rho(X, codes, scale)[0]
    err = abs(exact_dist(q, X)[0]
              - np.float64(approx_dist(q, X, codes, scale)[0]))
    print(f"d={d}: coherent err = {err:.6e}, rho = {r:.6e}, "
          f"eps = {eps[0]:.6e}")
    assert err >= 0.85 * r
    assert err <= eps[0]
