/* sdbv.h — C-ABI of the MI355X-native SurrealDB vector-KNN hot path.
 *
 * This is the drop-in boundary: the Rust host (surrealdb) would bind these
 * entry points via hip-sys/bindgen (see INTEGRATION.md for the binding stub).
 * Each function cites the reference interface it replaces:
 *
 *  - sdbv_knn_bruteforce / sdbv_knn_batch replace the distance+top-K core of
 *    the brute-force KnnTopK operator
 *    (reference: surrealdb/core/src/exec/operators/knn_topk.rs:166-267 and the
 *    legacy KnnPriorityList path surrealdb/core/src/idx/planner/knn.rs:11-106).
 *    The host keeps: record streaming, Value->vector extraction
 *    (knn_topk.rs:274-288), WHERE filtering, and record materialisation.
 *    sdbv_knn_bruteforce_filtered takes the outcome of that filtering (and
 *    the rows deleted since staging) as an allowed-row bitmap.
 *  - sdbv_stage_corpus replaces the per-search scattered vector access of
 *    the reference (VectorCache LRU + He KV keys,
 *    surrealdb/core/src/idx/trees/hnsw/cache.rs,
 *    surrealdb/core/src/idx/trees/hnsw/elements.rs:94-140) with a one-time
 *    HBM-resident staging of a table's vectors.
 *  - sdbv_hnsw_* replace the layer-0 best-first search loop
 *    (surrealdb/core/src/idx/trees/hnsw/layer.rs:184-223) behind
 *    HnswIndex::knn_search (surrealdb/core/src/idx/trees/hnsw/index.rs:270-335),
 *    plus the graph build (sequential = parity; parallel/snapshot = bench
 *    mode) and element removal with neighbour repair.
 *  - sdbv_index_* replace the whole HnswIndex operator surface: the Hp
 *    pendings queue (index.rs:138-257), VecDocs/Ids64 doc expansion
 *    (docs.rs, knn.rs:163-326), doc-id allocation with recycling, the
 *    pendings-merged knn_search (index.rs:270-335) and the cond_filter
 *    flow (hnsw/filter.rs) behind a host truthiness callback. The host
 *    keeps only what touches the KV transaction: value->vector
 *    extraction, the RecordIdKey<->handle map, WHERE evaluation, record
 *    materialisation.
 *  - sdbv_kvload_* / sdbv_*_dump_kv speak the reference's on-disk formats
 *    (key/index/{he,hn,hs,hv,hp}.rs) for cold-start bulk loads and dumps.
 *
 * Plain pointers and sizes only; no torch types. All calls are synchronous
 * w.r.t. results and thread-safe (internal per-context mutex). The caller
 * owns all host buffers; the context owns all device memory.
 */
#ifndef SDBV_H
#define SDBV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes (negative) — 0 == OK. */
enum {
	SDBV_OK = 0,
	SDBV_ERR_HIP = -1,          /* HIP runtime error; see sdbv_last_error */
	SDBV_ERR_NO_TABLE = -2,     /* table id not staged */
	SDBV_ERR_BAD_ARG = -3,      /* dimension mismatch, k out of range, ... */
	SDBV_ERR_OOM = -4,          /* device allocation failed */
	SDBV_ERR_UNSUPPORTED = -5,  /* metric not GPU-supported (host fallback is the
	                               caller's oracle-free CPU path, not ours) */
	SDBV_ERR_IDS_UNSORTED = -6, /* ids must be strictly increasing (tie-break contract) */
};

/* Distance metric — mirrors catalog::Distance
 * (surrealdb/core/src/catalog/schema/index.rs:250-284), all 8 variants on
 * the GPU scan. COSINE/EUCLIDEAN run the LDS-tiled k_scan (the headline
 * path); the others run an all-distances kernel + exact top-k selection,
 * on the device for tables the policy admits and k <= 65536, on the host
 * otherwise (see sdbv_knn_bruteforce; the same at any metric for k > 64)
 * (each restating the reference's F32 chain, vector.rs:206-451 —
 * including jaccard's bit-pattern sets :317-340 and the F32 |I|/|U|
 * asymmetry, and pearson's similarity-as-distance :413-440). MINKOWSKI
 * takes its order from sdbv_table_set_order (default 0 — degenerate, like
 * the reference with order 0). */
enum {
	SDBV_METRIC_COSINE = 0,
	SDBV_METRIC_EUCLIDEAN = 1,
	SDBV_METRIC_MANHATTAN = 2,
	SDBV_METRIC_CHEBYSHEV = 3,
	SDBV_METRIC_HAMMING = 4,
	SDBV_METRIC_JACCARD = 5,
	SDBV_METRIC_MINKOWSKI = 6,
	SDBV_METRIC_PEARSON = 7,
};

typedef struct sdbv_ctx sdbv_ctx; /* owns HIP stream, device pools, staged tables */

typedef struct sdbv_stats {
	double last_scan_kernel_ms;  /* HIP-event time of the last call's distance-producing
	                                kernels (scan; or prefilter + compact + rescore) */
	double last_merge_kernel_ms; /* HIP-event time of the last call's top-K selects */
	double last_total_ms;        /* host wall of the last search call (incl. D2H of K results) */
	uint64_t bytes_staged;       /* device bytes held by staged tables */
	uint64_t last_rows_scanned;  /* rows the last scan covered */
	uint64_t last_prefilter_candidates; /* rows the last prefilter passed to the
	                                       exact rescore (0 on the exact scan) */
	uint32_t last_scan_path; /* sdbv_knn_bruteforce: 0 = exact scan, 1 = bf16
	                            prefilter, 2 = bf16 prefilter overflowed, then
	                            exact scan, 3 = int8 prefilter, 4 = int8
	                            prefilter overflowed, then exact scan, 5 = int6
	                            prefilter, 6 = int6 prefilter overflowed, then
	                            exact scan. sdbv_knn_bruteforce_filtered: 7 =
	                            masked scan, 8 = row-list path, 9 = bf16
	                            prefilter under the bitmap, 10 = that
	                            overflowed, then masked scan, 11 / 12 = the
	                            same for int8, 13 / 14 for int6, 0 = the
	                            all-distances route. sdbv_knn_bruteforce
	                            again: 15 = two-stage int6 prefilter (plane H
	                            streamed alone, survivors refined with plane
	                            L), 16 = its candidate list overflowed, then
	                            exact scan. Euclidean tables: 17 = l2 (int8)
	                            prefilter, 18 = that overflowed, then exact
	                            scan; sdbv_knn_bruteforce_filtered: 19 = l2
	                            prefilter under the bitmap, 20 = that
	                            overflowed, then masked scan. The
	                            all-distances route with the top-K selected
	                            on the device: 21 = sdbv_knn_bruteforce (and
	                            the per-query calls of sdbv_knn_batch on a
	                            non-GEMM metric), 22 = under the bitmap of
	                            sdbv_knn_bruteforce_filtered; with the host
	                            selection the route stays 0. On 21 / 22
	                            last_scan_kernel_ms is the all-distances
	                            launch, last_merge_kernel_ms the select
	                            passes and the emit */
	uint64_t last_filter_rows; /* allowed rows of the last filtered call (for
	                              such a call last_rows_scanned is the same
	                              count) */
	uint64_t last_prefilter_stage1; /* rows that passed the H-only test of the
	                                   last two-stage call, also when that
	                                   list overflowed and the plain int6
	                                   path served the call (path 5 / 6);
	                                   0 on every other path */
	uint64_t last_batch_exact_queries; /* queries of the last sdbv_knn_batch
	                                      call that the single-query exact
	                                      scan answered: norm outside
	                                      [2^-30, 2^30], window certificate
	                                      failed, or a table with more than
	                                      1024 rows without a usable key */
	uint32_t last_batch_refold; /* 1 if a candidate buffer of the fused kernel
	                               overflowed in the last sdbv_knn_batch call
	                               and all rows were selected again through
	                               the rocBLAS pass, else 0 */
	double last_append_ms;        /* host wall of the last sdbv_append_rows call
	                                 that added rows, its synchronisation
	                                 included */
	double last_append_kernel_ms; /* HIP-event time of that call's append
	                                 kernel and shadow update (a regrowth is
	                                 not in it) */
	uint32_t last_append_realloc; /* 0 if that call wrote in place, 1 if it
	                                 regrew the table's store first */
	double last_update_ms;        /* host wall of the last sdbv_update_rows call
	                                 that changed rows, its synchronisation
	                                 included */
	double last_update_kernel_ms; /* HIP-event time of that call's scatter
	                                 kernel, shadow update and header refold */
	uint64_t last_update_blocks;  /* 256-row shadow blocks that call rewrote
	                                 (0 on a table without a shadow) */
} sdbv_stats;

/* Create a context on HIP device `device` (-1 = current device). */
int sdbv_init(int device, sdbv_ctx **out);
void sdbv_shutdown(sdbv_ctx *);

const char *sdbv_last_error(sdbv_ctx *);
int sdbv_get_stats(sdbv_ctx *, sdbv_stats *out);

/* Stage a table's vectors into HBM as a feature-major f32 store
 * (column-major [d][n_pad]) plus per-row f64 norms precomputed with the
 * reference's norm semantics (vector.rs:244-249).
 * `rows` is row-major n x d host memory. `ids` maps row -> record/doc id and
 * must be strictly increasing (NULL => 0..n-1); result tie-break is
 * (distance asc, id asc), which equals the reference's orderings for
 * monotone ids (knn.rs:363 BTreeSet<(FloatKey, VectorId)>, knn_topk.rs:61-73
 * insertion-order seq). Restages (replaces) if `table` already staged;
 * sdbv_append_rows adds rows behind the staged ones without restaging,
 * sdbv_update_rows replaces the vectors of staged rows.
 *
 * Memory: d*4 + 20 B per row. A COSINE table of at least
 * SDBV_SCAN_PREFILTER_MIN_ROWS rows (environment, default 500000) also gets
 * a single-query prefilter shadow, unless the environment sets
 * SDBV_SCAN_PREFILTER=0 or the allocation fails: then the table simply has
 * no shadow and staging still succeeds. The shadow is the int8 one, d + 8 B
 * per row more (+25 %), if the table also has at least
 * SDBV_SCAN_PREFILTER_I8_MIN_ROWS rows (environment, default 500000,
 * independent of the first threshold) and SDBV_SCAN_PREFILTER_I8 is not 0;
 * otherwise the bf16 one, d*2 + 4 B per row more (+50 %). An int8-eligible
 * table gets the int6 shadow instead, 0.75 * d_pad + 12 B per row (d_pad = d
 * rounded up to a multiple of 32), if it also has at least
 * SDBV_SCAN_PREFILTER_I6_MIN_ROWS rows (environment, default 500000,
 * independent of the other thresholds) and SDBV_SCAN_PREFILTER_I6 is not 0.
 * An int6 shadow that staging builds for a table of at least
 * SDBV_SCAN_PREFILTER_H4_MIN_ROWS rows (environment, default 1000000) while
 * SDBV_SCAN_PREFILTER_H4 is not 0 carries 8 B per row more: the bound and
 * the code sum of its high-nibble plane read on its own, which the two-stage
 * path needs (see sdbv_knn_bruteforce).
 * A EUCLIDEAN table (the default metric of DEFINE INDEX ... HNSW) of at
 * least SDBV_SCAN_PREFILTER_L2_MIN_ROWS rows (environment, default 500000)
 * gets the l2 shadow, d + 12 B per row more (+25 %), unless
 * SDBV_SCAN_PREFILTER_L2 is 0 or the allocation fails. The pair is the
 * euclidean tier's own: the SDBV_SCAN_PREFILTER* variables above never give
 * a euclidean table a shadow, and these two never give a cosine table one.
 * A table holds at
 * most one shadow. The shadow never changes a result (see
 * sdbv_knn_bruteforce). Tables staged for graph search (sdbv_hnsw_finalize,
 * sdbv_index_*) never get one. */
int sdbv_stage_corpus(sdbv_ctx *, uint64_t table, const float *rows,
                      const uint64_t *ids, uint64_t n, uint32_t d,
                      uint8_t metric);

/* Stage a deterministic synthetic corpus directly on-device (no PCIe):
 * element (row_offset+i, j) = splitmix64-derived U[-20,20) f32 — the committed
 * restatement of the BASELINE synthetic-data contract (matches
 * RandomItemGenerator::Float(-20,20), knn.rs:633-643, by distribution;
 * exact bit-stream defined by oracle/orc_gen_f32). ids = id_base + i. */
int sdbv_stage_synthetic(sdbv_ctx *, uint64_t table, uint64_t n, uint32_t d,
                         uint8_t metric, uint64_t seed, uint64_t row_offset,
                         uint64_t id_base);

/* Build (on != 0) the bf16 prefilter shadow of a staged cosine table, or free
 * (on == 0) whichever shadow it has, explicitly, regardless of the staging
 * policy — for tests and for A/B in one process. SDBV_ERR_UNSUPPORTED for
 * non-cosine tables, SDBV_ERR_OOM when the shadow does not fit (the table
 * stays usable without it). */
int sdbv_table_set_prefilter(sdbv_ctx *, uint64_t table, int on);
/* The same with the kind spelled out: 0 = none, 1 = bf16, 2 = int8 (codes in
 * [-127, 127] with one f32 scale per row, plus the row's own proven error
 * bound: d + 8 B per row). Setting a kind frees a shadow of another kind;
 * any other value is SDBV_ERR_BAD_ARG. */
int sdbv_table_set_prefilter_kind(sdbv_ctx *, uint64_t table, int kind);
/* Give the table the int6 shadow (codes in [-31, 31], one f32 scale, the
 * row's bound and the sum of its stored codes: 0.75 * d_pad + 12 B per row),
 * freeing a shadow of another kind; without the side data of the two-stage
 * path, which only staging builds (a staged int6 shadow that carries it is
 * rebuilt without). Errors as for
 * sdbv_table_set_prefilter; free it with sdbv_table_set_prefilter(.., 0) or
 * sdbv_table_set_prefilter_kind(.., 0). */
int sdbv_table_set_prefilter_i6(sdbv_ctx *, uint64_t table);
/* Build (on != 0) or free (on == 0) the l2 shadow of a staged EUCLIDEAN
 * table, regardless of the staging policy: int8 codes as for kind 2 with
 * three f32 values per row, the scale, the squared length of the dequantised
 * row and the row's residual rounded up (d + 12 B per row).
 * SDBV_ERR_UNSUPPORTED for every other metric (the three entries above keep
 * refusing euclidean tables), SDBV_ERR_OOM when the shadow does not fit. */
int sdbv_table_set_prefilter_l2(sdbv_ctx *, uint64_t table, int on);
/* Host-only: the proven bound on |exact - prefilter| cosine distance at
 * dimension d, and f32 -> bf16 round-to-nearest-even (returned as f32) as
 * the shadow is built. */
float sdbv_prefilter_eps(uint32_t d);
float sdbv_bf16_rne(float x);
/* Host-only: the proven bound on |key - E| that sdbv_knn_batch's window
 * certificate uses, for a row and a query with norms in [2^-30, 2^30]
 * (euclidean rows: at most 2^30). key is the row's f32 selection key,
 * cosine -(s * f32(1 / norm)), euclidean sumsq - 2 s, with the f32 dot
 * products s and sumsq summed in ANY order; E is the row's exact distance
 * mapped into the key's domain in f64, cosine -(1 - dist) * q_norm, euclidean
 * dist^2 - q_norm^2. metric 0 = cosine, 1 = euclidean; max_row_norm (euclidean
 * only) is the largest staged row norm. */
double sdbv_batch_key_bound(uint8_t metric, uint32_t d, double q_norm,
                            double max_row_norm);
/* Host-only: quantise one row of d <= 4096 f32 elements for the int8 shadow
 * exactly as staging does. norm = the row's staged norm (sqrt of the restated
 * f32 sum-of-squares chain, in f64). codes[k] = rint(x[k] / scale) in
 * [-127, 127], *scale = f32(maxabs / 127), *eps = the proven bound on
 * |exact - prefilter| cosine distance of THIS row for any query with a norm
 * in [2^-30, 2^30]. A row the bound cannot cover (non-finite element, norm
 * outside [2^-30, 2^30]) gets zero codes, *scale = NaN and *eps = 0: the
 * prefilter always recomputes such a row. */
int sdbv_prefilter_i8_row(const float *x, uint32_t d, double norm,
                          int8_t *codes, float *scale, float *eps);
/* Host-only: quantise one row for the l2 shadow exactly as staging does.
 * codes and *scale as for int8; with x^ = scale * codes, *xx = |x^|^2 computed
 * in f64 and rounded once, *res = |x - x^| + 2^-68 computed in f64 and rounded
 * UP (the 2^-68 stands for squares that underflow in the exact chain). A row
 * the bound cannot cover (non-finite element, f64 norm above 2^30) gets zero
 * codes, *scale = NaN, *xx = *res = 0. The zero row is covered. */
int sdbv_prefilter_l2_row(const float *x, uint32_t d, int8_t *codes,
                          float *scale, float *xx, float *res);
/* Host-only: the interval the l2 stream computes for that row and the query
 * q, with the kernel's own operations: *lo <= exact euclidean distance <=
 * *up (-inf / +inf for an uncovered row). SDBV_ERR_UNSUPPORTED for a query
 * outside the window (non-finite element, f64 norm above 2^30); the zero
 * query is inside. */
int sdbv_prefilter_l2_interval(const float *q, uint32_t d, const int8_t *codes,
                               float scale, float xx, float res, float *lo,
                               float *up);
/* Host-only: the same for the int6 shadow. codes[k] = rint(x[k] / scale) in
 * [-31, 31], *scale = f32(maxabs / 31), *xsum = sum of the stored codes
 * (codes[k] + 32) over the row padded with zero codes to a multiple of 32
 * features, *eps = the proven bound of THIS row against an exactly
 * represented query; for a query with residual rho_q (sdbv_prefilter_q12)
 * the prefilter uses e = eps + (1 + eps) * qeps in f32, qeps = 1.01 * rho_q
 * rounded up to f32. Uncovered rows as for int8. */
int sdbv_prefilter_i6_row(const float *x, uint32_t d, double norm,
                          int8_t *codes, float *scale, float *eps,
                          uint32_t *xsum);
/* Host-only: the int6 row's high nibbles as the two-stage path reads them.
 * codes_h[k] = (code + 32) >> 2 in [0, 15] of sdbv_prefilter_i6_row's codes,
 * standing for scale * (4 * codes_h[k] + 1.5 - 32); *xsum_h = sum of
 * codes_h over the row padded with nibbles 8 to a multiple of 32 features;
 * *eps4 = the proven bound of THIS row for that approximant, used as *eps is
 * (e = eps4 + (1 + eps4) * qeps). Uncovered rows: nibbles 8, *scale = NaN,
 * *eps4 = 0. */
int sdbv_prefilter_h4_row(const float *x, uint32_t d, double norm,
                          uint8_t *codes_h, float *scale, float *eps4,
                          uint32_t *xsum_h);
/* Host-only: quantise one query of d <= 4096 f32 elements for the int6 tier
 * exactly as sdbv_knn_bruteforce does. codes[k] = rint(q[k] / sq) in
 * [-2047, 2047], *sq = f32(maxabs / 2047), *rho_q = |q - sq * codes| / |q|
 * (|q| = sqrt of the restated f32 sum-of-squares chain) computed in f64 and
 * rounded up to f32, *qs = sum of (codes[k] + 2048) over the query padded
 * with zero codes to a multiple of 32 features. A query the prefilter never
 * runs for (non-finite, norm outside [2^-30, 2^30]) gets zero codes,
 * *sq = NaN and *rho_q = 0. */
int sdbv_prefilter_q12(const float *q, uint32_t d, int16_t *codes, float *sq,
                       float *rho_q, uint32_t *qs);

uint64_t sdbv_table_rows(sdbv_ctx *, uint64_t table);
int sdbv_drop_table(sdbv_ctx *, uint64_t table);

/* Append m row-major rows to a table staged by sdbv_stage_corpus or
 * sdbv_stage_synthetic, without restaging it. `ids` must be strictly
 * increasing with ids[0] above the table's last staged id (NULL => last id
 * + 1, + 2, ...), which keeps the tie-break contract of sdbv_stage_corpus. A
 * row whose id sorts INSIDE the staged range still needs a restage; a change
 * to a staged row is sdbv_update_rows. After SDBV_OK every search entry point answers in
 * every bit (ids, distance bits, *out_n, and the path and candidate counts
 * of sdbv_stats) as if the table had been staged once with the concatenated
 * rows and ids. Synchronous; holds the context mutex.
 *
 * Capacity: a table's column stride n_pad is also its capacity
 * (sdbv_table_capacity). Rows that fit (n + m <= n_pad) are written in place
 * by one kernel: transpose into the feature-major store, norms, batch aux and
 * ids of the new rows only, then the table's prefilter shadow over the
 * 256-row blocks that hold them; the call allocates nothing once the
 * context's staging buffer exists (rows pass through it in chunks of at most
 * 256 MiB). Rows that do not fit regrow the store first, to
 * sdbv_append_capacity(n_pad, n + m): new arrays are allocated BEFORE the
 * old ones are freed (peak device memory: old plus new store), the store is
 * copied, and the shadow is rebuilt at the new capacity with its kind and
 * side data (one pass over the store; a shadow that no longer fits is
 * dropped and the append still succeeds). Growth is geometric, so a stream
 * of appends pays O(log n) regrowths; sdbv_table_reserve avoids them. A table
 * keeps the shadow it has: the staging policy's row thresholds are not asked
 * again. sdbv_stats.bytes_staged follows the capacity.
 *
 * Checked before anything is touched (a refused call leaves the table as it
 * was): SDBV_ERR_NO_TABLE; SDBV_ERR_UNSUPPORTED for a table staged for graph
 * search (sdbv_hnsw_finalize, sdbv_index_*); SDBV_ERR_BAD_ARG when d differs
 * from the table's, rows == NULL with m > 0, or n + m >= 2^32;
 * SDBV_ERR_IDS_UNSORTED when ids are not increasing or ids[0] is not above
 * the last staged id. m == 0 is SDBV_OK and nothing happens. A failed
 * regrowth is SDBV_ERR_OOM with the table intact. */
int sdbv_append_rows(sdbv_ctx *, uint64_t table, const float *rows,
                     const uint64_t *ids, uint64_t m, uint32_t d);
/* Replace the vectors of m staged rows in place, without restaging the
 * table. `row_idx` holds m row POSITIONS, strictly increasing and all < n
 * (the convention of sdbv_knn_bruteforce_filtered and sdbv_gather_distance:
 * ids are increasing, so the position of a record is the rank of its id);
 * `rows` is m x d row-major, row i replaces the vector at position
 * row_idx[i]. Ids, n, the capacity and bytes_staged do not change, and the
 * call allocates nothing once the context's staging buffer is large enough
 * (rows and their positions pass through it in chunks of at most 256 MiB):
 * there is never a regrowth. After SDBV_OK every search entry point answers
 * in every bit (ids, distance bits, *out_n, and the path and candidate
 * counts of sdbv_stats) as if the table had been staged once with the
 * current rows and ids and the same shadow kind and side data. A table keeps
 * the shadow it has. Synchronous; holds the context mutex.
 *
 * One kernel scatters the rows into the feature-major store and writes their
 * norms and batch aux; the table's prefilter shadow is rebuilt over exactly
 * the distinct 256-row blocks that hold a listed row (sdbv_update_blocks, one
 * launch); on cosine and euclidean tables the batch path's largest keyed norm
 * and its rows without a usable key are then recomputed from the per-row
 * arrays (4-12 B per row), since an overwritten row must be forgotten.
 *
 * Checked before anything is touched (a refused call leaves the table as it
 * was): SDBV_ERR_NO_TABLE; SDBV_ERR_UNSUPPORTED for a table staged for graph
 * search; SDBV_ERR_BAD_ARG when d differs from the table's, rows or row_idx
 * is NULL with m > 0, a position is >= n, or the positions are not strictly
 * increasing (so no position occurs twice). m == 0 is SDBV_OK and nothing
 * happens. */
int sdbv_update_rows(sdbv_ctx *, uint64_t table, const uint32_t *row_idx,
                     const float *rows, uint64_t m, uint32_t d);
/* Host-only: the distinct 256-row blocks (row / 256) that hold the m strictly
 * increasing positions, ascending; returns their number and writes the first
 * min(count, cap) to out_blocks (may be NULL with cap 0). */
uint64_t sdbv_update_blocks(const uint32_t *row_idx, uint64_t m,
                            uint32_t *out_blocks, uint64_t cap);
/* Grow the table's capacity to at least `rows` now (rounded up to a multiple
 * of 4096, no growth factor), as a regrowing append does; a no-op when the
 * capacity is already that large. A bulk loader reserves once and then
 * appends in place. Errors as for sdbv_append_rows; rows >= 2^32 is
 * SDBV_ERR_BAD_ARG. */
int sdbv_table_reserve(sdbv_ctx *, uint64_t table, uint64_t rows);
/* Rows the table's store holds without regrowing; 0 = not staged. */
uint64_t sdbv_table_capacity(sdbv_ctx *, uint64_t table);
/* Host-only: the capacity a table of capacity n_pad has after an append that
 * needs `need` rows: n_pad when need <= n_pad, otherwise
 * max(need, n_pad + n_pad / 2) rounded up to a multiple of 4096 (the least
 * common multiple of the scan tile and the shadow tiers' tiles). */
uint64_t sdbv_append_capacity(uint64_t n_pad, uint64_t need);

/* Minkowski order for a staged table (Distance::Minkowski(Number),
 * index.rs:258): call after staging; ignored by other metrics. */
int sdbv_table_set_order(sdbv_ctx *, uint64_t table, double order);

/* Host-side generator of the committed synthetic-data contract (bench/test
 * input prep; bit-identical to the device staging generator). */
void sdbv_gen_f32(uint64_t seed, uint64_t row0, uint64_t nrows, uint32_t d,
                  float *out);

/* Brute-force exact K-nearest-neighbour scan of a staged table.
 * Results sorted ascending by (distance f64-total_cmp, id).
 * Distances follow Distance::calculate F32 semantics (vector.rs:244-249 /
 * 282-283): f32 accumulation per the restated ndarray contract, f64 finish.
 * COSINE/EUCLIDEAN with k <= 64 run fully on-device (block-local exact
 * top-K). Larger k (the reference accepts any) and the six other metrics
 * take one all-distances launch into context-owned scratch, then an exact
 * selection under the same ordering contract:
 *  - on the device (last_scan_path 21) when k <= 65536, the table has fewer
 *    than 2^32 rows and at least SDBV_SELECT_DEVICE_MIN_ROWS of them
 *    (environment, read at each call, default 65536) and SDBV_SELECT_DEVICE
 *    is not 0 (read at each call): an MSB-first radix select over (distance
 *    total_cmp key, row), 8 bits per pass, finds the k-th smallest pair; the
 *    rows at or below it, k of them exactly, come back and the host sorts
 *    them. The pairs are distinct, so the set is unique and the result is
 *    the host selection's in every bit. A count other than min(k, n) is
 *    SDBV_ERR_HIP, never a shorter result;
 *  - on the host otherwise (last_scan_path 0), costing an n-f64 and an n-id
 *    transfer per query.
 * *out_n = min(k, n).
 *
 * On a cosine table with a prefilter shadow (k <= 64, finite query with a
 * norm in [2^-30, 2^30]) the call streams the shadow instead of the f32
 * store: bf16 (half the bytes), keeping every row within twice the proven
 * bound sdbv_prefilter_eps(d) of the Kth approximate distance; or int8 (a
 * quarter), keeping every row whose approximate distance minus its own
 * proven bound does not exceed the Kth smallest approximate distance plus
 * bound; or int6 (0.75 of int8), the same rule on an exact integer dot
 * product of 6-bit row codes and a 12-bit quantised query, whose own
 * quantisation error is part of each row's bound. It recomputes those rows with the exact chain. Exactness guarantee: ids and distance bits equal the exact scan's
 * for every input — rows the bound cannot cover are always recomputed, and
 * a query with more than 16384 candidates reruns the exact scan
 * (sdbv_stats.last_scan_path tells which path ran).
 *
 * Two-stage int6 path (last_scan_path 15), chosen at each call over an int6
 * shadow that carries the H-only side data, unless SDBV_SCAN_PREFILTER_H4 is
 * 0 or the table has fewer than SDBV_SCAN_PREFILTER_H4_MIN_ROWS rows
 * (default 1000000, the measured crossover): the
 * call streams the high-nibble plane alone (two thirds of the int6 bytes),
 * takes the threshold T from the EXACT distances of the K rows with the
 * smallest upper bounds, lists the rows whose H-only lower bound is not
 * above T (at most SDBV_SCAN_PREFILTER_H4_LIST_MAX of them, default and
 * ceiling 262144, read at each call), keeps of those the rows whose full
 * int6 lower bound is not above T, and recomputes these. A first list that
 * overflows hands the call to the plain int6 path (5 / 6); more than 16384
 * rows after the second test rerun the exact scan (16).
 *
 * On a euclidean table with the l2 shadow (k <= 64, finite query with an
 * f64 norm of at most 2^30, the zero query included) the call streams the
 * int8 codes and brackets every row's exact distance from the triangle
 * inequality, [lo, up] around |scale * codes - q| widened by the row's
 * residual and the proven rounding terms; it keeps every row whose lo does
 * not exceed the Kth smallest up and recomputes those with the exact chain
 * (last_scan_path 17; more than 16384 candidates rerun the exact scan, 18).
 * The same exactness guarantee holds. */
int sdbv_knn_bruteforce(sdbv_ctx *, uint64_t table, const float *q, uint32_t d,
                        uint32_t k, uint64_t *out_ids, double *out_dists,
                        uint32_t *out_n);

/* Filtered brute-force: sdbv_knn_bruteforce restricted to the rows a bitmap
 * allows. The reference's KnnTopK (knn_topk.rs:166-267) ranks the stream the
 * planner hands it, i.e. the rows that survive the residual WHERE and are not
 * deleted; this call gives a table staged once the same meaning.
 * `allow` is a bitmap over ROW POSITIONS of the staged table: row r is
 * allowed iff bit (r & 63) of word (r >> 6) is set. Staged ids are strictly
 * increasing, so the host's id -> row map is the rank of the id (row == id
 * when the table was staged with ids == NULL). allow_words must equal
 * ceil(n / 64); anything else, or allow == NULL, is SDBV_ERR_BAD_ARG. Bits at
 * positions >= n in the last word are ignored.
 * Result contract: that of sdbv_knn_bruteforce over the allowed rows only —
 * ascending (distance f64 total_cmp, id), distance bits of the exact chain,
 * *out_n = min(k, allowed rows); no allowed row gives *out_n = 0, SDBV_OK and
 * no launch. The path never changes a result.
 * COSINE/EUCLIDEAN with k <= 64 run on-device: at most
 * SDBV_FILTER_ROWLIST_MAX allowed rows (environment, read at each call,
 * default and ceiling 16384; 0 = never) are listed by the host and gathered
 * one workgroup per row (last_scan_path 8). More allowed rows than that
 * stream the table's prefilter shadow under the bitmap when the table is
 * cosine and has a shadow of any kind, the query norm lies in
 * [2^-30, 2^30], SDBV_FILTER_PREFILTER is not 0 and the table has at least
 * SDBV_FILTER_PREFILTER_MIN_ROWS rows (both environment, read at each call;
 * default 500000): the tier's prefilter with its threshold taken over the
 * allowed rows and only allowed rows as candidates, then the exact rescore
 * (last_scan_path 9 bf16, 11 int8, 13 int6). A wave skips the rows of its
 * span when none of them is allowed: 512 rows (bf16), 1024 (int8), 64
 * (int6). More than 16384 candidates rerun the call as the masked scan
 * (10, 12, 14). A euclidean table with the l2 shadow streams it under the
 * same two variables, for a query inside that tier's window (19; 1024 rows
 * per skipped wave span; overflow 20). Every other call runs the masked scan, k_scan with the
 * bitmap as a second validity test, which skips every 256-row segment
 * without an allowed row (last_scan_path 7). The shadow is only read: an
 * unfiltered call before or after is not disturbed. Other metrics and
 * larger k take the all-distances launch over every row, then a selection
 * that skips the rows not allowed: the device select of sdbv_knn_bruteforce
 * under the bitmap (last_scan_path 22) when k <= 65536 and
 * SDBV_SELECT_DEVICE / SDBV_SELECT_DEVICE_MIN_ROWS admit the table (the
 * minimum counts the table's rows, not the allowed ones), the host selection
 * otherwise (last_scan_path 0). */
int sdbv_knn_bruteforce_filtered(sdbv_ctx *, uint64_t table, const float *q,
                                 uint32_t d, uint32_t k,
                                 const uint64_t *allow, uint64_t allow_words,
                                 uint64_t *out_ids, double *out_dists,
                                 uint32_t *out_n);
/* Host-only: the bitmap walk of the filtered call. Returns the number of
 * allowed rows below n and writes the first min(count, cap) of them to
 * out_rows in ascending order (out_rows may be NULL with cap 0). Bits at or
 * past n are ignored. */
uint64_t sdbv_filter_rows(const uint64_t *allow, uint64_t allow_words,
                          uint64_t n, uint32_t *out_rows, uint64_t cap);
/* Host-only: the digit walk of the device select on host histograms, sharing
 * its per-pass step with the kernels. Of the n < 2^32 f64 values in dists,
 * restricted to the rows `allow` admits (NULL = all; else ceil(n / 64) words,
 * bits at or past n ignored), writes the rows of the min(k, rows considered)
 * smallest to out_rows in result order — ascending f64 total order (-NaN,
 * -inf, ..., -0, +0, ..., +inf, +NaN), ties by ascending row — and their
 * number to *out_n. SDBV_OK, or SDBV_ERR_BAD_ARG. */
int sdbv_select_topk(const double *dists, uint64_t n, const uint64_t *allow,
                     uint32_t k, uint32_t *out_rows, uint32_t *out_n);

/* Batched-query brute-force: Q is b x d row-major; out_ids/out_dists are
 * b x k row-major, a query with fewer than k rows padded with id ~0 and
 * distance +inf. The dense Q x corpus^T product runs on MFMA. Results (ids,
 * order, distance bits) equal sdbv_knn_bruteforce's for every query.
 *
 * k is at most 48 on cosine and euclidean tables (SDBV_ERR_BAD_ARG above):
 * per query the call selects a window of k + 16 <= 64 rows by an f32 key,
 * recomputes those exactly, and then proves per query that the window holds
 * the k nearest: the window's largest key must exceed the k-th exact distance
 * mapped into the key's domain by more than sdbv_batch_key_bound. A query
 * whose window fails that test (near-duplicate rows around the query), or
 * whose norm is outside [2^-30, 2^30] (zero and non-finite included), is
 * answered by the exact scan of sdbv_knn_bruteforce instead. Rows without a
 * usable key (norm non-finite or above 2^30; on cosine tables also below
 * 2^-30, zero included) never enter a window: staging lists them and every
 * query gets their exact distances as well; a table with more than 1024 such
 * rows is answered by the exact scan throughout.
 * sdbv_stats.last_batch_exact_queries counts the queries the exact scan
 * answered, last_batch_refold says whether a candidate buffer overflowed. */
int sdbv_knn_batch(sdbv_ctx *, uint64_t table, const float *Q, uint32_t b,
                   uint32_t d, uint32_t k, uint64_t *out_ids,
                   double *out_dists);

/* ---- HNSW (graph search; graph topology stays host-side) ---- */

/* Batched gather+distance for HNSW layer-0 neighbour expansion
 * (replaces the per-visit get_vector + Distance::calculate of
 * layer.rs:184-223): for frontier rows[i] (row indices into the staged
 * table), out_dists[i] = distance(q, row). */
int sdbv_gather_distance(sdbv_ctx *, uint64_t table, const uint32_t *rows,
                         uint32_t nrows, const float *q, uint32_t d,
                         double *out_dists);

/* HNSW index — the Hnsw/HnswIndex replacement (hnsw/mod.rs, hnsw/index.rs,
 * layer.rs, heuristic.rs). Graph topology and upper layers live host-side
 * (as in the reference engine); layer-0 neighbour expansion runs as the
 * batched gather+distance kernel over the staged table; doc-id expansion,
 * pendings merge and cond filtering stay with the caller.
 *
 * Element ids are insertion ordinals (the caller maps them to records, as
 * HnswDocs does, docs.rs:39-145).
 *
 * Defaults mirror DEFINE INDEX ... HNSW (syn/parser/stmt/define.rs:1102-1180):
 * m=12, m0=2m, efc=150, ml=1/ln(m), extend=keep=0, metric EUCLIDEAN, F32. */
typedef struct sdbv_hnsw sdbv_hnsw;
int sdbv_hnsw_create(sdbv_ctx *, uint32_t d, uint8_t metric, uint32_t m,
                     uint32_t m0, uint32_t efc, int extend_candidates,
                     int keep_pruned, uint64_t rng_seed, double ml,
                     sdbv_hnsw **out);
/* Insert one vector (Hnsw::insert, hnsw/mod.rs:389-394; level drawn from the
 * committed RNG restatement of :263-266). Sequential build — deterministic,
 * used for parity. */
int sdbv_hnsw_insert(sdbv_hnsw *, const float *pt);
/* Parallel bulk build (bench mode): levels are drawn deterministically per
 * ordinal, insert order is nondeterministic across threads (striped node
 * locks) — graph quality validated by the reference's recall bars, like the
 * reference's own lock-free enqueue + batched apply (index.rs:138-211). */
int sdbv_hnsw_insert_batch(sdbv_hnsw *, const float *pts, uint64_t n,
                           int nthreads);
/* Chunked SNAPSHOT bulk build (bench mode, one step beyond the parallel
 * build's relaxed ordering): per chunk, every level-0 element's efc-search
 * runs against the graph as of the chunk start (read-only, parallel, and —
 * round 2 — batched onto the persistent device kernel), then the apply
 * half runs under the striped node locks. Quality pinned by the same
 * recall bars as the parallel build. */
int sdbv_hnsw_insert_batch_snapshot(sdbv_hnsw *, const float *pts,
                                    uint64_t n, uint32_t chunk,
                                    int nthreads);
/* Snapshot build with the BATCHED apply schedule at layers 1 and 0 (one
 * fixed serialization of the parallel apply per layer: all selects, then
 * all appends in element order, then one prune pass). Levels >= 2 — the
 * tiny skeleton layers — insert classically (progressive), and a
 * 64-element classic warm-up bootstraps an empty graph (both measured
 * requirements). Same algorithm, quality pinned by the same
 * recall bars; the bit-exact host reference for the _gpu build below. */
int sdbv_hnsw_insert_batch_snapshot2(sdbv_hnsw *, const float *pts,
                                     uint64_t n, uint32_t chunk,
                                     int nthreads);
/* GPU-accelerated chunked snapshot build (hnsw/mod.rs:230-394 build hot
 * loop): bit-identical to
 * sdbv_hnsw_insert_batch_snapshot2 — each chunk's layer-1 and layer-0
 * efc-searches run as multi-ep persistent-kernel launches against
 * delta-updated padded device adjacencies (ef=1 launches carry the
 * level-0 elements' layer-1 descent hop), and the select/prune
 * pair-distance work (the RAM-bound part of the apply) runs on device
 * with the exact heuristic (k_pair_mats/k_heur_select). Requires a
 * device context; efc <= 512; extend-candidates falls back to the host
 * twin. */
int sdbv_hnsw_insert_batch_snapshot_gpu(sdbv_hnsw *, const float *pts,
                                        uint64_t n, uint32_t chunk,
                                        int nthreads);
/* Stage vectors (feature-major + norms) into the device table slot `table`;
 * required before sdbv_hnsw_knn. */
int sdbv_hnsw_finalize(sdbv_hnsw *, uint64_t table);
/* knn_search (hnsw/index.rs:270-335 minus host-kept parts): upper-layer
 * greedy descent host-side, layer-0 ef-search with GPU batched neighbour
 * expansion. Results ascending (dist total_cmp, id), truncated to k. */
int sdbv_hnsw_knn(sdbv_hnsw *, const float *q, uint32_t k, uint32_t ef,
                  uint64_t *out_ids, double *out_dists, uint32_t *out_n);
/* Host-side knn_search (no device): the build path's search algorithm over
 * the host graph — same exact result contract. For CPU-side tests, quality
 * audits and boxes without a staged device table. */
int sdbv_hnsw_knn_host(sdbv_hnsw *, const float *q, uint32_t k, uint32_t ef,
                       uint64_t *out_ids, double *out_dists, uint32_t *out_n);
/* Batched ef-search on the persistent kernel (one query per workgroup, the
 * whole layer-0 best-first loop in-kernel — same exact result contract as
 * sdbv_hnsw_knn). Q is b x d; outputs are b x k (+ out_ns per query).
 * ef <= 512. */
int sdbv_hnsw_knn_batch(sdbv_hnsw *, const float *Q, uint32_t b, uint32_t k,
                        uint32_t ef, uint64_t *out_ids, double *out_dists,
                        uint32_t *out_ns);
/* Full per-layer graph export (CSR + membership + enter point + zero-copy
 * vector view): lets a host-side searcher (the bench's oracle cpu_baseline
 * leg) run on the exact graph the device searches. */
uint64_t sdbv_hnsw_layer_edge_count(sdbv_hnsw *, uint32_t layer);
void sdbv_hnsw_layer_export(sdbv_hnsw *, uint32_t layer, uint32_t *offsets,
                            uint32_t *edges, uint8_t *in_layer);
int64_t sdbv_hnsw_enter_point(sdbv_hnsw *);
const float *sdbv_hnsw_vecs_ptr(sdbv_hnsw *);
void sdbv_hnsw_destroy(sdbv_hnsw *);
/* Remove one graph element with neighbour repair (Hnsw::remove,
 * hnsw/mod.rs:398-455 + layer.rs:408-460). Pre-finalize host graphs only;
 * a finalized index mutates through sdbv_index_* (which re-finalizes).
 * Returns 1 if removed, 0 if the element did not exist. */
int sdbv_hnsw_remove(sdbv_hnsw *, uint64_t e_id);
/* Introspection (parity tests): */
uint64_t sdbv_hnsw_n(sdbv_hnsw *);
uint32_t sdbv_hnsw_layers(sdbv_hnsw *);
uint64_t sdbv_hnsw_l0_edge_count(sdbv_hnsw *);
void sdbv_hnsw_l0_export(sdbv_hnsw *, uint32_t *offsets /* n+1 */,
                         uint32_t *edges);

/* ------------------------------------------------------------------------
 * Index layer — the HnswIndex operator surface (hnsw/index.rs) with the
 * KV-backed parts (Hp pendings queue, Hv vector->docs entries, hi/hd
 * record-key<->doc-id maps) held in host memory. The host binding passes
 * record keys as opaque u64 handles ordered like its RecordIdKey ordering
 * (INTEGRATION.md "record-key handles"); value->vector extraction
 * (content_to_vectors, index.rs:118-129) stays on the host side of this
 * boundary. ctx may be NULL for a host-only (CPU-testable) index; with a
 * ctx, searches run the GPU per-hop path, re-finalizing into device table
 * slot `table` after writes. */
typedef struct sdbv_index sdbv_index;
int sdbv_index_create(sdbv_ctx * /* nullable */, uint64_t table, uint32_t d,
                      uint8_t metric, uint32_t m, uint32_t m0, uint32_t efc,
                      int extend_candidates, int keep_pruned,
                      uint64_t rng_seed, double ml, sdbv_index **out);
void sdbv_index_destroy(sdbv_index *);
/* HnswIndex::index (index.rs:138-186): append one pending update (old/new
 * vectors, n*d f32 each; the id kind — DocId vs RecordKey — resolves via
 * the record-key map exactly as HnswDocs::get_doc_id does). */
int sdbv_index_enqueue(sdbv_index *, uint64_t record_key, const float *olds,
                       uint32_t n_old, const float *news, uint32_t n_new);
/* HnswIndex::index_pendings (index.rs:188-257): drain + apply the queue in
 * appending order through VecDocs (insert/remove, graph element removal
 * with repair, doc-id recycling). */
int sdbv_index_apply_pendings(sdbv_index *, uint64_t *out_count);
/* HnswIndex::knn_search (index.rs:270-335 minus record materialisation):
 * pendings overlay + graph search (pending docs excluded from the
 * expansion frontier, layer.rs:320-338) + Ids64 doc expansion through one
 * KnnResultBuilder. Out arrays sized k; entries ascending
 * (dist total_cmp, VectorId); kind 0 = DocId, 1 = RecordKey handle. */
int sdbv_index_knn(sdbv_index *, const float *q, uint32_t k, uint32_t ef,
                   uint8_t *out_kinds, uint64_t *out_ids, double *out_dists,
                   uint32_t *out_n);
/* Filtered KNN (cond_filter pushdown — hnsw/filter.rs + layer.rs:110-318):
 * the host evaluates the WHERE condition per VectorId (is_record_truthy,
 * filter.rs:111-138 — KV fetch + expression compute stay host-side); the
 * library keeps the FilterCache semantics (one evaluation per id while
 * cached; `expire` fires when the result builder evicts an id,
 * filter.rs:141-151) and all accept/expand gating (add_if_truthy,
 * layer.rs:278-306). `truthy` must be deterministic within one call;
 * `expire` may be NULL. */
typedef int (*sdbv_truthy_cb)(void *user, uint8_t kind, uint64_t id);
typedef void (*sdbv_expire_cb)(void *user, uint8_t kind, uint64_t id);
int sdbv_index_knn_filtered(sdbv_index *, const float *q, uint32_t k,
                            uint32_t ef, sdbv_truthy_cb truthy,
                            sdbv_expire_cb expire, void *user,
                            uint8_t *out_kinds, uint64_t *out_ids,
                            double *out_dists, uint32_t *out_n);
uint64_t sdbv_index_doc_count(sdbv_index *);
uint64_t sdbv_index_pending_count(sdbv_index *);
/* check_hnsw_properties (hnsw/mod.rs:561-570): 0 == OK. */
int sdbv_index_check_props(sdbv_index *, uint64_t expected_count);
/* Test access to the underlying graph (CSR parity vs the oracle). */
sdbv_hnsw *sdbv_index_hnsw(sdbv_index *);
/* Level-RNG state carry-over (extension): the reference's insert-level RNG
 * is entropy-seeded per process (hnsw/mod.rs:263-266) so any state is
 * conformant; persisting it keeps this framework's same-seed determinism
 * across cold starts. */
uint64_t sdbv_index_level_rng(sdbv_index *);
void sdbv_index_set_level_rng(sdbv_index *, uint64_t state);

/* ------------------------------------------------------------------------
 * KV codec + cold-start staging pipeline: bulk-load a
 * dumped surrealdb HNSW index — He element vectors (key/index/he.rs), Hn
 * per-node edge lists (hn.rs), Hs graph state (hs.rs), Hv vector->docs
 * entries (hv.rs) — straight into the host graph (no re-insertion), then
 * finalize stages it to the device SoA. Key/value byte formats are pinned
 * by the reference's own key tests (he.rs/hn.rs/hs.rs/hv.rs golden
 * bytes); values follow the `revision` 0.17.0 wire format. Post-Hl
 * (per-node Hn) storage only; legacy Hl chunks and Bits (roaring) doc
 * sets are rejected with SDBV_ERR_UNSUPPORTED. hd/hi/hp/hh pairs are
 * host-kept and skipped by the loader; the host re-binds record keys via
 * sdbv_index_bind_doc_key. */
typedef struct sdbv_kvload sdbv_kvload;
int sdbv_kvload_new(sdbv_ctx * /* nullable */, uint32_t d, uint8_t metric,
                    uint32_t m, uint32_t m0, uint32_t efc,
                    int extend_candidates, int keep_pruned, uint64_t rng_seed,
                    double ml, sdbv_kvload **out);
int sdbv_kvload_feed(sdbv_kvload *, const uint8_t *key, uint64_t klen,
                     const uint8_t *val, uint64_t vlen);
int sdbv_kvload_finish_hnsw(sdbv_kvload *, sdbv_hnsw **out);
int sdbv_kvload_finish_index(sdbv_kvload *, uint64_t table, sdbv_index **out);
void sdbv_kvload_abort(sdbv_kvload *);
int sdbv_index_bind_doc_key(sdbv_index *, uint64_t doc_id,
                            uint64_t record_key);
/* Export the doc-id <-> record-key map (the hi/hd state the host persists
 * for cold starts). Returns the total entry count; fills up to cap. */
uint64_t sdbv_index_doc_keys(sdbv_index *, uint64_t *out_docs,
                             uint64_t *out_keys, uint64_t cap);
/* Dump the graph / index back to reference-format KV pairs (round-trip +
 * migration tooling). The callback returns non-zero to abort. */
typedef int (*sdbv_kv_write_cb)(void *user, const uint8_t *key, uint64_t klen,
                                const uint8_t *val, uint64_t vlen);
int sdbv_hnsw_dump_kv(sdbv_hnsw *, uint32_t ns, uint32_t db, const char *tb,
                      uint32_t ix, sdbv_kv_write_cb, void *user);
int sdbv_index_dump_kv(sdbv_index *, uint32_t ns, uint32_t db, const char *tb,
                       uint32_t ix, sdbv_kv_write_cb, void *user);

#ifdef __cplusplus
}
#endif

#endif /* SDBV_H */
