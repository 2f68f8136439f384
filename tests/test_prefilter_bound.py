"""The single-query prefilter's error bound, checked on the CPU.

The bf16 shadow and the prefilter's f32 arithmetic are restated in numpy
(rounding through the library's own sdbv_bf16_rne) and compared with the
oracle's exact cosine distance: |exact - approx| must stay under
sdbv_prefilter_eps(d) on random vectors and on vectors built to come as
close to the bound as the arithmetic allows."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

DIMS = [4, 16, 20, 128, 768, 4096]


def np_bf16_rne(x):
    """Restatement: f32 -> bf16 round-to-nearest-even, as f32 (finite x)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = u.astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def lib_bf16_rne(x):
    flat = np.ascontiguousarray(x, dtype=np.float32).ravel()
    out = np.array([surrealdb_amd.bf16_rne(v) for v in flat],
                   dtype=np.float32)
    return out.reshape(np.shape(x))


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


def approx_dist(q, X):
    """The prefilter's approximate cosine distance of every row of X:
    bf16 shadow, f32 accumulation, a = 1 - s * inv_q * inv_i in f32."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    Xs = lib_bf16_rne(X)
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for k in range(X.shape[1]):
        acc = acc + Xs[:, k] * q[k]
    inv_i = (1.0 / np.sqrt(sumsq_f32(X).astype(np.float64))).astype(
        np.float32)
    inv_q = np.float32(
        1.0 / np.sqrt(np.float64(sumsq_f32(q.reshape(1, -1))[0])))
    return np.float32(1.0) - acc * inv_q * inv_i


def exact_dist(q, X):
    return np.array([oracle.dist_f32("cosine", q, np.ascontiguousarray(x))
                     for x in X])


def test_bf16_rne_matches_numpy_restatement():
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 1 << 32, size=2000, dtype=np.uint64).astype(
        np.uint32)
    special = np.array([
        0x3F808000,  # tie, even mantissa below: rounds down
        0x3F818000,  # tie, odd mantissa below: rounds up
        0x3F807FFF,  # just under the midpoint
        0x3F808001,  # just over the midpoint
        0x3F7FFFFF,  # carry out of the mantissa into the exponent -> 1.0
        0x3FFF8000,  # tie with an all-ones bf16 mantissa: carry -> 2.0
        0x7F7FFFFF,  # FLT_MAX: the rounding overflows to +inf
        0xFF7F8000,  # negative tie that overflows to -inf
        0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,  # subnormals
        0x00000000, 0x80000000,
    ], dtype=np.uint32)
    bits = np.concatenate([bits, special])
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    got = lib_bf16_rne(x).view(np.uint32)
    want = np_bf16_rne(x).view(np.uint32)
    assert np.array_equal(got, want)
    assert np.all(got & 0xFFFF == 0)
    one = np.array([0x3F7FFFFF], dtype=np.uint32).view(np.float32)
    assert lib_bf16_rne(one)[0] == np.float32(1.0)
    big = np.array([0x7F7FFFFF], dtype=np.uint32).view(np.float32)
    assert np.isinf(lib_bf16_rne(big)[0])


def test_eps_formula():
    for d in DIMS:
        e = surrealdb_amd.prefilter_eps(d)
        assert e > 2.0 ** -8 + 2 * d * 2.0 ** -24
        assert e < 1.15 * 2.0 ** -8 + 2.2 * d * 2.0 ** -24
    assert abs(surrealdb_amd.prefilter_eps(768) - 0.0041) < 1e-4


@pytest.mark.parametrize("d", DIMS)
def test_bound_random(d):
    m = 64 if d < 4096 else 16
    X = oracle.gen_f32(0x5DB1, 0, m, d)
    # rows of very different lengths: the bound is in cosine units
    scale = np.float32(2.0) ** np.arange(-20, 20, dtype=np.float32)
    X = X * scale[np.arange(m) % scale.size, None]
    q = oracle.gen_f32(0xBEEF, 0, 1, d)[0]
    err = np.abs(exact_dist(q, X) - approx_dist(q, X).astype(np.float64))
    eps = surrealdb_amd.prefilter_eps(d)
    print(f"d={d}: max |exact - approx| = {err.max():.3e}, eps = {eps:.3e}")
    assert np.all(err <= eps)


def just_under_midpoint(rng, d):
    """Elements 2^e * (1 + 2^-8 - 2^-23): the bf16 mantissa is zero and the
    discarded bits are 0x7FFF, one below the rounding midpoint, so every
    element loses (almost) the largest possible relative amount."""
    e = rng.integers(126, 129, size=d).astype(np.uint32)  # 2^-1 .. 2^1
    sign = rng.integers(0, 2, size=d).astype(np.uint32)
    bits = (sign << 31) | (e << 23) | 0x7FFF
    return bits.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("d", DIMS)
def test_bound_worst_case_parallel(d):
    """x parallel to q, every element just under a rounding midpoint: all
    quantisation errors pull the same way, so the error must come close to
    2^-8 and still stay under the bound."""
    rng = np.random.default_rng(d)
    x = just_under_midpoint(rng, d)
    X = x.reshape(1, -1)
    err = abs(exact_dist(x, X)[0] - np.float64(approx_dist(x, X)[0]))
    eps = surrealdb_amd.prefilter_eps(d)
    print(f"d={d}: parallel worst case err = {err:.6e}, 2^-8 = "
          f"{2.0 ** -8:.6e}, eps = {eps:.6e}")
    assert err >= 0.95 * 2.0 ** -8
    assert err <= eps


@pytest.mark.parametrize("d", DIMS)
def test_bound_worst_case_same_signs(d):
    """q with x's sign pattern but other magnitudes: every product is
    positive, so the quantisation errors still add up coherently."""
    rng = np.random.default_rng(1000 + d)
    x = just_under_midpoint(rng, d)
    mag = np.abs(oracle.gen_f32(0xABCD, 0, 1, d)[0]) + np.float32(0.5)
    q = np.copysign(mag, x).astype(np.float32)
    X = x.reshape(1, -1)
    exact = exact_dist(q, X)[0]
    err = abs(exact - np.float64(approx_dist(q, X)[0]))
    eps = surrealdb_amd.prefilter_eps(d)
    cos = 1.0 - exact
    print(f"d={d}: same-sign err = {err:.6e} at cos = {cos:.4f}, "
          f"eps = {eps:.6e}")
    # the coherent quantisation term is 2^-8 / (1 + 2^-8) of the cosine
    assert err >= 0.9 * cos * 2.0 ** -8
    assert err <= eps
