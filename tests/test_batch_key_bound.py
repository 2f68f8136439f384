"""The batch path's key bound, checked on the CPU.

sdbv_knn_batch selects a window of rows per query by an f32 key whose dot
products come out of a GEMM in an unknown summation order, and then proves
that the window holds the k nearest rows with sdbv_batch_key_bound: a bound
on |key - E|, E being the row's exact distance (the oracle's restated chain)
mapped into the key's domain in f64,

    cosine:    key = -(s * f32(1 / norm)),  E = -(1 - dist) * q_norm
    euclidean: key = sumsq - 2 s,           E = dist^2 - q_norm^2.

Here the key is restated in numpy f32 under several summation orders and the
bound must cover every one of them, on random vectors and on vectors built to
make f32 summation lose as much as it can."""
import numpy as np
import pytest

import oracle
import surrealdb_amd

DIMS = [1, 7, 32, 768, 4096]
ORDERS = ["forward", "reversed", "pairwise", "block2", "block8", "block32"]


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


def sum_f32(P, order):
    """Row sums of the f32 products P (m x d), every addition rounded to f32,
    in the given order."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    m, d = P.shape
    if order == "reversed":
        P, order = P[:, ::-1], "forward"
    if order == "forward":
        acc = np.zeros(m, dtype=np.float32)
        for k in range(d):
            acc = acc + P[:, k]
        return acc
    if order == "pairwise":
        while P.shape[1] > 1:
            if P.shape[1] % 2:
                P = np.concatenate(
                    [P, np.zeros((m, 1), dtype=np.float32)], axis=1)
            P = P[:, 0::2] + P[:, 1::2]
        return P[:, 0]
    blk = int(order[len("block"):])
    part = np.zeros((m, blk), dtype=np.float32)
    for k in range(d):
        part[:, k % blk] = part[:, k % blk] + P[:, k]
    return sum_f32(part, "forward")


def keys_and_exact(metric, q, X):
    """({order: f32 keys}, E in f64, q_norm, largest row norm)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    qn = np.sqrt(np.float64(sumsq_f32(q.reshape(1, -1))[0]))
    norms = np.sqrt(sumsq_f32(X).astype(np.float64))
    dist = np.array([oracle.dist_f32(metric, q, np.ascontiguousarray(x))
                     for x in X])
    keys = {}
    for order in ORDERS:
        s = sum_f32(X * q[None, :], order)
        if metric == "cosine":
            inv = (1.0 / norms).astype(np.float32)
            keys[order] = -(s * inv)
        else:
            # the staged sumsq follows the restated chain; any order of it
            # is covered as well, so it takes the order of s here
            aux = sum_f32(X * X, order)
            keys[order] = aux - np.float32(2.0) * s
    if metric == "cosine":
        E = -((1.0 - dist) * qn)
    else:
        E = dist * dist - qn * qn
    return keys, E, qn, norms.max()


def check(metric, q, X, what):
    d = X.shape[1]
    keys, E, qn, rmax = keys_and_exact(metric, q, X)
    bound = surrealdb_amd.batch_key_bound(metric, d, qn, rmax)
    worst = 0.0
    for order, key in keys.items():
        assert key.dtype == np.float32
        err = np.abs(key.astype(np.float64) - E)
        worst = max(worst, err.max())
        assert np.all(err <= bound), \
            f"{metric} d={d} {what} {order}: {err.max():.3e} > {bound:.3e}"
    print(f"{metric} d={d} {what}: max |key - E| = {worst:.3e}, "
          f"bound = {bound:.3e}")
    return worst, bound


def test_bound_formula():
    u = 2.0 ** -24
    for d in DIMS:
        c = surrealdb_amd.batch_key_bound("cosine", d, 1.0)
        assert 2 * (d + 1) * u + 3 * u < c < 1.02 * (2 * (d + 1) * u + 3 * u)
        # linear in the query norm, quadratic in the norms for euclidean
        assert surrealdb_amd.batch_key_bound("cosine", d, 8.0) == 8.0 * c
        e = surrealdb_amd.batch_key_bound("euclidean", d, 3.0, 5.0)
        assert 64 * (3 * (d + 2) * u + 2 * u) < e
        assert e < 64 * 1.02 * (3 * (d + 2) * u + 2 * u) + 1e-30
    # the estimate the fallback condition rests on: 768-d cosine, |q| = 320
    assert abs(surrealdb_amd.batch_key_bound("cosine", 768, 320.0)
               - 0.0297) < 1e-3


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", DIMS)
def test_bound_random(metric, d):
    m = 40 if d < 4096 else 12
    X = oracle.gen_f32(0x5DB1, 0, m, d)
    # rows of very different lengths (norms stay inside [2^-30, 2^30])
    scale = np.float32(2.0) ** np.arange(-12, 12, dtype=np.float32)
    X = X * scale[np.arange(m) % scale.size, None]
    for qscale in (1.0, 2.0 ** -10, 2.0 ** 10):
        q = oracle.gen_f32(0xBEEF, 0, 1, d)[0] * np.float32(qscale)
        check(metric, q, X, f"random q*{qscale:g}")


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", DIMS)
def test_bound_all_same_sign(metric, d):
    """Every product positive: the rounding errors of a running sum cannot
    cancel, and a forward sum's grow with the partial sum."""
    X = np.abs(oracle.gen_f32(0x71, 0, 8, d)) + np.float32(0.5)
    q = np.abs(oracle.gen_f32(0x72, 0, 1, d)[0]) + np.float32(0.5)
    check(metric, q, X, "same sign")
    # nearly identical elements, just under a rounding step
    x = np.full((1, d), np.float32(1.0) - np.float32(2.0 ** -24))
    check(metric, x[0].copy(), x, "same sign, constant")


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
@pytest.mark.parametrize("d", DIMS)
def test_bound_alternating_huge_tiny(metric, d):
    """Huge and tiny elements in turn, with and without cancellation: the
    tiny products are absorbed or not depending on the summation order."""
    rng = np.random.default_rng(d)
    mag = np.where(np.arange(d) % 2 == 0, 3.0e3, 3.0e-3).astype(np.float32)
    jitter = (1.0 + rng.random((6, d)) * 0.5).astype(np.float32)
    X = mag[None, :] * jitter
    X[1::2] *= np.where(rng.random((3, d)) < 0.5, -1.0, 1.0).astype(
        np.float32)
    q = (mag * (1.0 + rng.random(d) * 0.5)).astype(np.float32)
    check(metric, q, X, "huge/tiny")
    # the tiny elements carry the query: the huge products cancel in pairs
    q2 = q.copy()
    q2[0::4] = -q2[0::4]
    check(metric, q2, X, "huge/tiny, cancelling")
    # the query as a row of the table: distance (almost) zero, where the
    # euclidean key is a difference of two large numbers
    check(metric, q, np.vstack([X, q[None, :]]), "huge/tiny, self")
