#!/usr/bin/env python3
"""Measure sdbv_append_rows against the only other way to add rows, a restage.

One process, per metric and base size n, on synthetic tables (the appended
rows are sdbv_gen_f32 at the continuing row offset, so stage_synthetic over
all rows is the bit-identical twin):

  stage      stage_synthetic(n): the table the appends go to
  reserve    table_reserve(n + 200000): one growth (allocation, column copy,
             shadow rebuild)
  append     in-place appends of m = 1, 64, 1024, 65536 rows: host wall time
             around the call (it ends in a synchronise) and the library's
             own last_append_ms / last_append_kernel_ms
  restage    stage_synthetic(n + m) into another slot: what adding m rows
             costs without the feature. It pays no PCIe, so it is a lower
             bound on a real restage
  query      knn_bruteforce alternating between the appended table and a
             twin staged once with the same rows: p50 of each, the twin
             against itself (even against odd calls) as the spread, and 16
             seeded queries compared in ids and distance bits. A third
             table, staged once and then reserved to the appended table's
             capacity, takes part too: it has the appended table's strides
             without an append
  grow       one append that regrows the twin (wall), then the same growth
             without a shadow (table_reserve after the shadow is freed): the
             difference is the shadow rebuild

Every record is one JSON line in --out. A missing GPU is an error.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import surrealdb_amd  # noqa: E402
from surrealdb_amd.synth import gen_f32  # noqa: E402

SEED, QSEED = 0x5DB1, 0xBEEF
T, TWIN, SCRATCH, CONTROL = 1, 2, 3, 4
SIZES = ((1, 20), (64, 20), (1024, 20), (65536, 2))   # (m, calls)
RESERVE = 200_000


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(xs):
    xs = sorted(xs)
    return {"p50": statistics.median(xs), "min": xs[0], "max": xs[-1],
            "calls": len(xs)}


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def run_one(ctx, metric, n, d, k, emit):
    base = {"metric": metric, "n": n, "d": d}
    ms = wall_ms(lambda: ctx.stage_synthetic(T, n, d, metric=metric,
                                             seed=SEED))
    emit(dict(base, kind="stage", wall_ms=ms,
              capacity=ctx.table_capacity(T)))
    ms = wall_ms(lambda: ctx.table_reserve(T, n + RESERVE))
    emit(dict(base, kind="reserve", wall_ms=ms,
              capacity=ctx.table_capacity(T)))

    # warm-up on a table of its own: the first append of a size allocates
    # the context's staging buffer, and first launches load code objects
    ctx.stage_synthetic(SCRATCH, 4096, d, metric=metric, seed=SEED)
    ctx.append_rows(SCRATCH, gen_f32(SEED, 4096, 65536, d))
    ctx.append_rows(SCRATCH, gen_f32(SEED, 4096 + 65536, 64, d))
    ctx.drop_table(SCRATCH)
    cur = n
    for m, calls in SIZES:
        walls, libs, kerns = [], [], []
        for _ in range(calls):
            rows = gen_f32(SEED, cur, m, d)
            walls.append(wall_ms(lambda: ctx.append_rows(T, rows)))
            st = ctx.stats()
            assert st["last_append_realloc"] == 0, "append was not in place"
            libs.append(st["last_append_ms"])
            kerns.append(st["last_append_kernel_ms"])
            cur += m
        emit(dict(base, kind="append", m=m, wall_ms=summary(walls),
                  lib_ms=summary(libs), kernel_ms=summary(kerns)))
    assert ctx.table_rows(T) == cur

    for m, _ in SIZES:
        walls = [wall_ms(lambda: ctx.stage_synthetic(
            SCRATCH, n + m, d, metric=metric, seed=SEED)) for _ in range(3)]
        emit(dict(base, kind="restage", m=m, wall_ms=summary(walls)))
    ctx.drop_table(SCRATCH)

    # the twin: all rows staged once
    ctx.stage_synthetic(TWIN, cur, d, metric=metric, seed=SEED)
    Q = gen_f32(QSEED, 0, 16, d)
    same = True
    for q in Q:
        a, b = ctx.knn_bruteforce(T, q, k), ctx.knn_bruteforce(TWIN, q, k)
        pa = ctx.stats()["last_scan_path"]
        same &= bool(np.array_equal(a[0], b[0]) and
                     np.array_equal(bits(a[1]), bits(b[1])))
    emit(dict(base, kind="query_equal", rows=cur, queries=len(Q),
              identical=same, path=pa))
    # the control: staged once like the twin, then reserved to the appended
    # table's capacity, so that it has that table's strides and no append
    ctx.stage_synthetic(CONTROL, cur, d, metric=metric, seed=SEED)
    ctx.table_reserve(CONTROL, ctx.table_capacity(T))
    assert ctx.table_capacity(CONTROL) == ctx.table_capacity(T)
    for table in (T, TWIN, CONTROL):        # warm all
        for q in Q:
            ctx.knn_bruteforce(table, q, k)
    t_app, t_twin, t_ctl, t_even, t_odd = [], [], [], [], []
    for i in range(200):
        q = Q[i % len(Q)]
        t_app.append(wall_ms(lambda: ctx.knn_bruteforce(T, q, k)))
        t_twin.append(wall_ms(lambda: ctx.knn_bruteforce(TWIN, q, k)))
        t_ctl.append(wall_ms(lambda: ctx.knn_bruteforce(CONTROL, q, k)))
    ctx.drop_table(CONTROL)
    for i in range(400):
        q = Q[(i // 2) % len(Q)]
        (t_even if i % 2 == 0 else t_odd).append(
            wall_ms(lambda: ctx.knn_bruteforce(TWIN, q, k)))
    emit(dict(base, kind="query", rows=cur, k=k,
              appended_ms=summary(t_app), twin_ms=summary(t_twin),
              twin_reserved_ms=summary(t_ctl),
              capacity_appended=ctx.table_capacity(T),
              capacity_twin=ctx.table_capacity(TWIN),
              twin_even_ms=summary(t_even), twin_odd_ms=summary(t_odd)))
    ctx.drop_table(T)

    # growth on the twin: its spare capacity is below 1024 rows
    rows = gen_f32(SEED, cur, 1024, d)
    cap0 = ctx.table_capacity(TWIN)
    ms = wall_ms(lambda: ctx.append_rows(TWIN, rows))
    st = ctx.stats()
    assert st["last_append_realloc"] == 1
    emit(dict(base, kind="grow_append", rows=cur, m=1024, wall_ms=ms,
              lib_ms=st["last_append_ms"],
              kernel_ms=st["last_append_kernel_ms"], capacity_before=cap0,
              capacity=ctx.table_capacity(TWIN)))
    if metric == "cosine":
        ctx.table_set_prefilter_kind(TWIN, 0)
    else:
        ctx.table_set_prefilter_l2(TWIN, False)
    cap1 = ctx.table_capacity(TWIN)
    ms = wall_ms(lambda: ctx.table_reserve(TWIN, cap1 + 1))
    emit(dict(base, kind="grow_no_shadow", rows=cur + 1024, wall_ms=ms,
              capacity_before=cap1, capacity=ctx.table_capacity(TWIN)))
    ctx.drop_table(TWIN)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metrics", default="cosine,euclidean")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    ctx = surrealdb_amd.Context(device=0)   # raises without a GPU
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        for metric in args.metrics.split(","):
            for n in (int(x) for x in args.rows.split(",")):
                run_one(ctx, metric, n, args.dim, args.k, emit)
    ctx.close()


if __name__ == "__main__":
    main()
