#!/usr/bin/env python3
"""Measure sdbv_update_rows against the only other way to change a row, a
restage.

One process, per metric and size n, on synthetic tables staged with the
default policy (row r of the table is sdbv_gen_f32 row r):

  stage      stage_synthetic(n): the table the updates go to
  update     m = 1, 64, 1024, 65536 rows, each as scattered positions
             (uniform random, distinct, fresh for every call) and as one
             contiguous run at a random start: host wall time around the call
             (it ends in a synchronise) and the library's own last_update_ms /
             last_update_kernel_ms / last_update_blocks. The new content of
             row r is row r of another seed, so every call changes its rows
  restage    stage_synthetic(n) into another slot: what changing a row costs
             without the feature. It generates on the device and pays no
             PCIe, so it is a lower bound on a real restage
  restore    one update that gives every touched row its first content back:
             the table is again what stage_synthetic(n) stages
  query      knn_bruteforce alternating between the updated table and a twin
             staged once: p50 of each, the twin against itself (even against
             odd calls) as the spread, and 32 queries compared in ids and
             distance bits: 16 seeded ones and 16 touched rows as queries

--trace-seq FILE runs the updates alone (10 calls per cell) and writes the
label of every update call, in order, to FILE; run that under
`rocprofv3 --kernel-trace` and give its kernel trace to --split, which sums
each call's dispatches into scatter (k_update_rows), shadow (k_shadow*) and
refold (k_aux_refold). No GPU is needed for --split.

Every record is one JSON line in --out. A missing GPU is an error.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import surrealdb_amd  # noqa: E402
from surrealdb_amd.synth import gen_f32  # noqa: E402

SEED, NEW_SEED, QSEED = 0x5DB1, 0x5DB2, 0xBEEF
T, TWIN, SCRATCH = 1, 2, 3
SIZES = ((1, 20), (64, 20), (1024, 20), (65536, 2))   # (m, calls)
PATTERNS = ("scattered", "run")


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


def positions(rng, n, m, pattern):
    if pattern == "run":
        start = int(rng.integers(0, n - m + 1))
        return np.arange(start, start + m, dtype=np.uint32)
    return np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)


def rows_of(seed, idx, d):
    """Row r of `seed` for every r of idx (strictly increasing)."""
    if idx.size and int(idx[-1]) - int(idx[0]) + 1 == idx.size:
        return gen_f32(seed, int(idx[0]), idx.size, d)
    return np.concatenate([gen_f32(seed, int(r), 1, d) for r in idx])


def run_updates(ctx, metric, n, d, emit, sizes, labels=None):
    """The timed updates on T; returns the sorted touched positions."""
    base = {"metric": metric, "n": n, "d": d}
    # warm-up on a table of its own: the first update of a size allocates the
    # context's staging buffer, and first launches load code objects
    ctx.stage_synthetic(SCRATCH, 300_000, d, metric=metric, seed=SEED)
    rng = np.random.default_rng(1)
    for m in (65536, 64):
        idx = positions(rng, 300_000, m, "scattered")
        ctx.update_rows(SCRATCH, idx, rows_of(NEW_SEED, idx, d))
        if labels is not None:
            labels.append("warmup")
    ctx.drop_table(SCRATCH)
    touched = []
    rng = np.random.default_rng(2)
    for pattern in PATTERNS:
        for m, calls in sizes:
            walls, libs, kerns, blocks = [], [], [], []
            for _ in range(calls):
                idx = positions(rng, n, m, pattern)
                rows = rows_of(NEW_SEED, idx, d)
                walls.append(wall_ms(lambda: ctx.update_rows(T, idx, rows)))
                st = ctx.stats()
                libs.append(st["last_update_ms"])
                kerns.append(st["last_update_kernel_ms"])
                blocks.append(st["last_update_blocks"])
                touched.append(idx)
                if labels is not None:
                    labels.append(f"{metric} {n} {pattern} {m}")
            emit(dict(base, kind="update", pattern=pattern, m=m,
                      wall_ms=summary(walls), lib_ms=summary(libs),
                      kernel_ms=summary(kerns), blocks=summary(blocks)))
    return np.unique(np.concatenate(touched))


def run_one(ctx, metric, n, d, k, emit):
    base = {"metric": metric, "n": n, "d": d}
    ms = wall_ms(lambda: ctx.stage_synthetic(T, n, d, metric=metric,
                                             seed=SEED))
    emit(dict(base, kind="stage", wall_ms=ms, capacity=ctx.table_capacity(T),
              bytes_staged=ctx.stats()["bytes_staged"]))
    touched = run_updates(ctx, metric, n, d, emit, SIZES)

    walls = [wall_ms(lambda: ctx.stage_synthetic(
        SCRATCH, n, d, metric=metric, seed=SEED)) for _ in range(5)]
    emit(dict(base, kind="restage", wall_ms=summary(walls), each=walls))
    ctx.drop_table(SCRATCH)

    rows = rows_of(SEED, touched, d)
    ms = wall_ms(lambda: ctx.update_rows(T, touched, rows))
    st = ctx.stats()
    emit(dict(base, kind="restore", m=int(touched.size), wall_ms=ms,
              lib_ms=st["last_update_ms"],
              kernel_ms=st["last_update_kernel_ms"],
              blocks=st["last_update_blocks"]))

    ctx.stage_synthetic(TWIN, n, d, metric=metric, seed=SEED)
    pick = touched[:: max(1, touched.size // 16)][:16]
    Q = np.concatenate([gen_f32(QSEED, 0, 16, d), rows_of(SEED, pick, d)])
    same, top1 = True, True
    for i, q in enumerate(Q):
        a, b = ctx.knn_bruteforce(T, q, k), ctx.knn_bruteforce(TWIN, q, k)
        pa = ctx.stats()["last_scan_path"]
        same &= bool(np.array_equal(a[0], b[0]) and
                     np.array_equal(bits(a[1]), bits(b[1])))
        if i >= 16:
            top1 &= bool(a[0][0] == pick[i - 16])
    emit(dict(base, kind="query_equal", queries=len(Q), identical=same,
              touched_rows_are_their_own_top1=top1, path=pa))
    for table in (T, TWIN):                 # warm both
        for q in Q:
            ctx.knn_bruteforce(table, q, k)
    t_upd, t_twin, t_even, t_odd = [], [], [], []
    for i in range(200):
        q = Q[i % 16]
        t_upd.append(wall_ms(lambda: ctx.knn_bruteforce(T, q, k)))
        t_twin.append(wall_ms(lambda: ctx.knn_bruteforce(TWIN, q, k)))
    for i in range(400):
        q = Q[(i // 2) % 16]
        (t_even if i % 2 == 0 else t_odd).append(
            wall_ms(lambda: ctx.knn_bruteforce(TWIN, q, k)))
    emit(dict(base, kind="query", k=k, updated_ms=summary(t_upd),
              twin_ms=summary(t_twin), twin_even_ms=summary(t_even),
              twin_odd_ms=summary(t_odd)))
    ctx.drop_table(T)
    ctx.drop_table(TWIN)


def split(trace_csv, seq_file, emit):
    """Sum each update call's dispatches by kernel, per label of seq_file."""
    with open(seq_file) as f:
        labels = json.load(f)
    with open(trace_csv, newline="") as f:
        disp = sorted(
            ((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
              r["Kernel_Name"]) for r in csv.DictReader(f)),
            key=lambda x: x[0])
    calls = []                              # one dict per k_update_rows
    for t0, t1, name in disp:
        us = (t1 - t0) / 1e3
        if "k_update_rows" in name:
            calls.append({"scatter": us, "shadow": 0.0, "refold": 0.0,
                          "open": True})
        elif not calls or not calls[-1]["open"]:
            continue                        # staging, not an update
        elif "k_shadow" in name:
            calls[-1]["shadow"] += us
        elif "k_aux_refold" in name:
            calls[-1]["refold"] += us
            calls[-1]["open"] = False
    if len(calls) != len(labels):
        raise SystemExit(f"{len(calls)} update calls in the trace, "
                         f"{len(labels)} labels")
    cells = {}
    for label, c in zip(labels, calls):
        cells.setdefault(label, []).append(c)
    for label, cs in cells.items():
        if label == "warmup":
            continue
        metric, n, pattern, m = label.split()
        emit({"kind": "kernel_split", "metric": metric, "n": int(n),
              "pattern": pattern, "m": int(m),
              **{part + "_us": summary([c[part] for c in cs])
                 for part in ("scatter", "shadow", "refold")}})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--metrics", default="cosine,euclidean")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", required=True)
    ap.add_argument("--trace-seq", metavar="FILE")
    ap.add_argument("--split", nargs=2, metavar=("KERNEL_TRACE_CSV", "SEQ"))
    args = ap.parse_args()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
        if args.split:
            split(args.split[0], args.split[1], emit)
            return
        ctx = surrealdb_amd.Context(device=0)   # raises without a GPU
        labels = [] if args.trace_seq else None
        for metric in args.metrics.split(","):
            for n in (int(x) for x in args.rows.split(",")):
                if labels is None:
                    run_one(ctx, metric, n, args.dim, args.k, emit)
                    continue
                ctx.stage_synthetic(T, n, args.dim, metric=metric, seed=SEED)
                run_updates(ctx, metric, n, args.dim, emit,
                            [(m, 10 if m < 65536 else 2) for m, _ in SIZES],
                            labels)
                ctx.drop_table(T)
        if labels is not None:
            with open(args.trace_seq, "w") as g:
                json.dump(labels, g)
        ctx.close()


if __name__ == "__main__":
    main()
