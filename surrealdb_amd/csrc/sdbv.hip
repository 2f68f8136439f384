// sdbv.hip — MI355X-native (gfx950/CDNA4) implementation of the SurrealDB
// vector-KNN hot path behind the C-ABI declared in include/sdbv.h.
//
// THIS IS THE PRODUCT PATH. It never calls into oracle/ (the parity oracle is
// test infrastructure); results are defined by the same restated reference
// contracts:
//  - cosine distance: Distance::calculate F32 semantics
//    (surrealdb/core/src/idx/trees/vector.rs:244-249): f32 dot with the
//    ndarray 0.17.2 eightfold-unrolled accumulation, f32 sum-of-squares norms,
//    f64 finish 1 - dot/(|a||b|).
//  - euclidean: vector.rs:282-283 via ndarray-stats l2_dist: sequential f32
//    (a-b)^2 accumulation, f64 sqrt.
//  - result order: ascending (f64 total_cmp distance, id) — knn.rs:128-160
//    FloatKey + knn.rs:363 BTreeSet<(FloatKey, VectorId)>; equals KnnTopK's
//    insertion-order tie-break (knn_topk.rs:61-73) for monotone ids.
//
// Design (MI355X-first, see DESIGN.md for the full rationale):
//  - A table's vectors live in HBM FEATURE-MAJOR (column-major [d][n_pad]):
//    one lane owns one corpus row, a wave's 64 lanes own 64 consecutive rows,
//    so every k-step loads 64x4 B = one fully-coalesced 256 B line (float4 =
//    4 rows/lane = 1 KiB per instruction). Per-lane accumulation preserves
//    the reference's per-row summation order BIT-EXACTLY while the chip
//    streams at the HBM roofline — no cross-lane reduction anywhere on the
//    scan path.
//  - The scan is HBM-read bound (3072 B/row vs ~1.5 kFLOP/row at d=768);
//    MFMA would not help a single query. The batched-query path
//    (sdbv_knn_batch) is the genuinely-dense case and uses MFMA tiles.
//  - Top-K: per-block threshold + LDS candidate buffer + single-wave
//    (dist,id)-exact selection; a final single-block kernel merges per-block
//    winners. Selection is by value, so results are deterministic and
//    scheduling-independent.
//
// Compile: hipcc --offload-arch=gfx950 -O3 (NO -ffast-math; accumulation
// chains use __fmul_rn/__fadd_rn so the compiler cannot contract them into
// fma — the reference's mul-then-add rounding is the contract).

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <deque>
#include <limits>
#include <memory>
#include <thread>
#include <unordered_set>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <queue>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sdbv.h"

#define THREADS 256
#define ROWS_PER_LANE 4
#define TILE (THREADS * ROWS_PER_LANE) /* 1024 rows per block-sweep */
#define MAX_K 64
#define MAX_D 4096 /* query staged in LDS: 16 KiB cap */

// ---------------------------------------------------------------------------
// Error plumbing
// ---------------------------------------------------------------------------
#define HIP_CHECK(ctx, call)                                                   \
	do {                                                                       \
		hipError_t _e = (call);                                                \
		if (_e != hipSuccess) {                                                \
			(ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e);    \
			return SDBV_ERR_HIP;                                               \
		}                                                                      \
	} while (0)

// Single-query prefilter shadow of a cosine table (optional, at most one tier
// per table): two device allocations, everything else derived from them.
//  1 bf16: codes = bf16 of cm, feature-major [d][sn_pad], rounded to
//    nearest-even; side = pinv, the per-row f32 1/norm (NaN marks a row the
//    error bound cannot cover).
//  2 int8: codes = bias-128 bytes, feature-major [d][sn_pad]; side = pscale
//    (scale/norm per row, NaN marks an uncovered row), then peps, the row's
//    proven bound.
//  3 int6: 6-bit codes, bias 32, lane = row, features in groups of 32,
//    G = ceil(d / 32); codes = plane H [G][sn_pad][4 dwords] with the high
//    nibbles, then plane L [G][sn_pad][2 dwords] with the low pairs; side =
//    pscale, peps, then xsum (the row's sum of stored codes); with h4 also
//    peps4 and xsum_h, the bound and the code sum of plane H read on its own
//    (the two-stage path).
// A euclidean table has one tier, with an index of its own (4 is taken by
// the int6 H-only grid entry of SHADOW_TIERS and pf_slots):
//  5 l2: codes as int8; side = the scale (NaN marks an uncovered row), then
//    xx = |scale * c|^2, then res, the row's residual rounded up
//    (DESIGN.md §11e).
struct Shadow {
	int kind = 0;          // 0 none, 1 bf16, 2 int8, 3 int6, 5 l2
	bool h4 = false;       // int6 only: side holds peps4 and xsum_h too
	void *codes = nullptr; // owning
	float *side = nullptr; // owning: sn_pad floats per side array
	uint64_t sn_pad = 0;   // n rounded up to the tier's tile
	uint64_t bytes = 0;    // both allocations, counted in Table::bytes
	float *pinv() const { return side; }
	float *pscale() const { return side; }
	float *peps() const { return side + sn_pad; }
	// l2: the stream kernel finds res sn_pad floats behind xx
	float *l2_xx() const { return side + sn_pad; }
	float *l2_res() const { return side + 2 * sn_pad; }
	uint32_t *xsum() const { return (uint32_t *)(side + 2 * sn_pad); }
	float *peps4() const { return h4 ? side + 3 * sn_pad : nullptr; }
	uint32_t *xsum_h() const {
		return h4 ? (uint32_t *)(side + 4 * sn_pad) : nullptr;
	}
	uint32_t *plane_h() const { return (uint32_t *)codes; }
	uint32_t *plane_l(uint32_t d) const {
		return plane_h() + (uint64_t)((d + 31) / 32) * sn_pad * 4;
	}
};

struct Table {
	uint64_t n = 0;
	uint64_t n_pad = 0;       // column stride of cm and the table's capacity:
	                          // roundup(n, TILE) as staged, a multiple of 4096
	                          // once grown; cells [n, n_pad) are zero
	uint64_t last_id = 0;     // id of row n - 1 (n > 0): appended ids are larger
	bool scan_table = true;   // staged for scanning (sdbv_append_rows refuses
	                          // a table staged for graph search)
	uint32_t d = 0;
	uint8_t metric = 0;
	double order = 0.0;       // minkowski order (sdbv_table_set_order)
	float *cm = nullptr;      // [d][n_pad] feature-major
	double *norms = nullptr;  // per-row f64 norm (cosine only)
	float *aux = nullptr;     // per-row f32 selection key aux for the batch
	                          // path: cosine 1/norm, euclidean sum-of-squares;
	                          // NaN marks a row without a usable key
	uint32_t *bunc = nullptr; // [BATCH_UNC_CAP] rows without a usable key
	uint32_t bunc_n = 0;      // their count (may exceed the list's capacity)
	double bmax_norm = 0.0;   // largest norm among the rows with a key
	uint64_t *ids_dev = nullptr; // per-row id, device (merge kernel maps)
	Shadow sh;
	uint64_t bytes = 0;
};

struct sdbv_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	std::map<uint64_t, Table> tables;
	std::mutex mu;
	std::string err;
	sdbv_stats stats{};
	// scratch
	void *block_out = nullptr; // [max_blocks][MAX_K] Cand
	uint64_t block_out_cap = 0;
	void *final_out = nullptr; // [MAX_K] Cand + ids
	void *merge_tmp = nullptr; // [32][MAX_K] Cand (tree-merge level 1)
	float *q_dev = nullptr;
	float *q_pin = nullptr; // pinned H2D staging for the per-query upload
	uint32_t q_cap = 0;
	hipEvent_t ev0, ev1, ev2, ev3, ev4;
	// single-query prefilter scratch
	float *pf_scores = nullptr; // [sn_pad] approximate distances
	uint64_t pf_scores_cap = 0;
	uint32_t *pf_rows = nullptr; // [PF_CAND_CAP] candidate rows
	uint32_t *pf4_list = nullptr; // [PF4_LIST_CAP] rows that passed the H-only
	                              // test of the two-stage path
	void *pf4_thr = nullptr;      // [MAX_K] Cand: its threshold rows, exact
	void *pf_cands = nullptr;    // [PF_CAND_CAP] rescored Cand
	void *pf_res = nullptr;      // [MAX_K + 2] Cand: top-k, the count, counter
	uint64_t pf_slots[2][6] = {}; // by MASKED and Shadow::kind (4 = the int6
	                              // tier's H-only stream): blocks of that
	                              // prefilter kernel the device holds at once
	// batched path
	rocblas_handle blas = nullptr;
	float *S = nullptr; // chunk scores scratch, [chunk][b] col-major
	uint64_t S_cap = 0;
	void *bstate = nullptr; // [b][kk] running candidates
	uint64_t bstate_cap = 0;
	float *Q_dev = nullptr;
	uint64_t Q_cap = 0;
	double *qnorms = nullptr;
	uint64_t qnorms_cap = 0;
	double *bdists = nullptr; // [b][kk] exact distances
	uint64_t bdists_cap = 0;
	// fused MFMA batch path scratch
	uint32_t *btheta = nullptr; // [b] per-query kth-best u32 key
	uint64_t btheta_cap = 0;
	void *bcand = nullptr; // [b][FMM_CAND_CAP] BCand survivors
	uint64_t bcand_cap = 0;
	uint32_t *bcand_cnt = nullptr; // [b]
	uint64_t bcand_cnt_cap = 0;
	double ms_gemm = 0, ms_select = 0, ms_exact = 0; // last batch timings
	// filtered brute-force scratch (sdbv_knn_bruteforce_filtered), its own:
	// the unfiltered call touches nothing here
	uint64_t *flt_mask = nullptr;     // [max(n_pad, sn_pad) / 64] allowed-row
	                                  // bitmap, device
	uint64_t *flt_mask_pin = nullptr; // pinned copy with the tail bits cleared
	uint64_t flt_mask_cap = 0;        // words, both buffers
	uint32_t *flt_rows = nullptr;     // [PF_CAND_CAP] allowed rows, device
	uint32_t *flt_rows_pin = nullptr; // pinned: the host builds the list here
	void *flt_cands = nullptr;        // [PF_CAND_CAP] Cand of the listed rows
	// device select of the all-distances route, grown on
	// demand
	double *sel_dists = nullptr; // [n] the all-distances buffer
	uint64_t sel_dists_cap = 0;  // bytes
	void *sel_dev = nullptr;     // SelDev, then [k_eff] Cand
	uint64_t sel_dev_cap = 0;    // bytes
	void *sel_pin = nullptr;     // pinned: SelHead, then [k_eff] Cand
	uint64_t sel_pin_cap = 0;    // bytes
	// sdbv_append_rows: one chunk of new rows, row-major, then their ids
	void *app_buf = nullptr;
	uint64_t app_buf_cap = 0; // bytes
};

struct Cand {
	double dist;
	uint64_t id; // staged id (already mapped via ids_dev)
};

// ---------------------------------------------------------------------------
// Device helpers
// ---------------------------------------------------------------------------
__device__ __host__ static inline uint64_t d_splitmix64(uint64_t z) {
	z += 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}

// The committed synthetic-data contract — bit-identical to oracle orc_gen_elem.
__device__ __host__ static inline float d_gen_elem(uint64_t seed, uint64_t gidx) {
	uint64_t x = d_splitmix64(seed + gidx);
	double u = (double)(x >> 11) * 0x1.0p-53;
	return (float)(-20.0 + 40.0 * u);
}

// f64 total_cmp key (knn.rs:128-160): monotone u64.
__device__ static inline uint64_t d_total_key(double x) {
	uint64_t bits = __double_as_longlong(x);
	return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
}

// ---------------------------------------------------------------------------
// Staging kernels
// ---------------------------------------------------------------------------

// Fill feature-major store with synthetic data: cm[k][r] = elem(row_offset+r, k).
__global__ void k_gen_cm(float *cm, uint64_t n, uint64_t n_pad, uint32_t d,
                         uint64_t seed, uint64_t row_offset) {
	uint64_t total = (uint64_t)d * n_pad;
	for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	     idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t k = idx / n_pad;
		uint64_t r = idx % n_pad;
		float v = 0.0f;
		if (r < n)
			v = d_gen_elem(seed, (row_offset + r) * (uint64_t)d + k);
		cm[idx] = v;
	}
}

// Transpose row-major [n][d] -> feature-major [d][n_pad], LDS-tiled 32x32.
__global__ void k_transpose(const float *__restrict__ rm, float *__restrict__ cm,
                            uint64_t n, uint64_t n_pad, uint32_t d) {
	__shared__ float tile[32][33];
	uint64_t rb = (uint64_t)blockIdx.x * 32; // row base
	uint32_t kb = blockIdx.y * 32;           // feature base
	uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32x8
	for (uint32_t yy = ty; yy < 32; yy += 8) {
		uint64_t r = rb + yy;
		uint32_t k = kb + tx;
		tile[yy][tx] = (r < n && k < d) ? rm[r * d + k] : 0.0f;
	}
	__syncthreads();
	for (uint32_t yy = ty; yy < 32; yy += 8) {
		uint32_t k = kb + yy;
		uint64_t r = rb + tx;
		if (k < d && r < n_pad)
			cm[(uint64_t)k * n_pad + r] = tile[tx][yy];
	}
}

// Per-row norms for cosine (vector.rs:246-247): sqrt(f64(sum a*a)) with the
// restated unrolled_fold f32 chain. One lane per row, feature-major reads.
__global__ void k_norms(const float *__restrict__ cm, double *__restrict__ norms,
                        uint64_t n, uint64_t n_pad, uint32_t d) {
	uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n)
		return;
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t k = 0;
	for (; k + 8 <= d; k += 8) {
#pragma unroll
		for (uint32_t j = 0; j < 8; j++) {
			float x = cm[(uint64_t)(k + j) * n_pad + r];
			p[j] = __fadd_rn(p[j], __fmul_rn(x, x));
		}
	}
	float acc = 0.0f;
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[0], p[4]), __fadd_rn(p[1], p[5])));
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[2], p[6]), __fadd_rn(p[3], p[7])));
	for (; k < d; k++) {
		float x = cm[(uint64_t)k * n_pad + r];
		acc = __fadd_rn(acc, __fmul_rn(x, x));
	}
	norms[r] = sqrt((double)acc);
}

__global__ void k_fill_ids(uint64_t *ids, uint64_t n, uint64_t id_base) {
	uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r < n)
		ids[r] = id_base + r;
}

// ---------------------------------------------------------------------------
// Brute-force scan kernel.
// Each block owns a contiguous row span; per 1024-row tile each lane computes
// ROWS_PER_LANE distances with the reference's per-row accumulation chain,
// threshold-checks against the block's current kth-best, and appends rare
// survivors to an LDS candidate buffer; wave 0 then merges candidates into
// the block top-K by exact (total_key(dist), row) selection.
// METRIC: 0 = cosine, 1 = euclidean.
// ---------------------------------------------------------------------------
struct LCand {
	uint64_t key; // total_key(dist)
	double dist;
	uint32_t row;
};

// Block-wide exact top-k selection from an LDS candidate array by ascending
// (key, row). All THREADS threads participate; every cross-thread hand-off is
// ordered by __syncthreads(). Deterministic: selection is by value.
__device__ static void block_select_topk(LCand *buf, int total, LCand *topk,
                                         int k, int *out_n) {
	__shared__ uint64_t red_key[THREADS / 64];
	__shared__ uint32_t red_row[THREADS / 64];
	__shared__ int red_idx[THREADS / 64];
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	int out = total < k ? total : k;
	for (int slot = 0; slot < out; slot++) {
		uint64_t bk = ~0ULL;
		uint32_t br = ~0u;
		int bi = -1;
		for (int i = threadIdx.x; i < total; i += THREADS) {
			uint64_t ck = buf[i].key;
			uint32_t cr = buf[i].row;
			if (ck < bk || (ck == bk && cr < br)) {
				bk = ck;
				br = cr;
				bi = i;
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			uint64_t ok = __shfl_down(bk, off);
			uint32_t orr = __shfl_down(br, off);
			int oi = __shfl_down(bi, off);
			if (ok < bk || (ok == bk && orr < br)) {
				bk = ok;
				br = orr;
				bi = oi;
			}
		}
		if (lane == 0) {
			red_key[wave] = bk;
			red_row[wave] = br;
			red_idx[wave] = bi;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			int best = -1;
			uint64_t bbk = ~0ULL;
			uint32_t bbr = ~0u;
			for (int w = 0; w < THREADS / 64; w++) {
				if (red_idx[w] < 0)
					continue;
				if (red_key[w] < bbk ||
				    (red_key[w] == bbk && red_row[w] < bbr)) {
					bbk = red_key[w];
					bbr = red_row[w];
					best = red_idx[w];
				}
			}
			topk[slot] = buf[best];
			buf[best].key = ~0ULL;
			buf[best].row = ~0u;
		}
		__syncthreads();
	}
	*out_n = out;
}

// The running block top-K of k_scan: prologue and epilogue (the fold between
// them is written in the kernel). The state lives in the kernel's own
// __shared__ declarations and is passed in, so the helpers add no LDS.
// Prologue: thread 0 clears it; the barrier also publishes the LDS query.
__device__ __forceinline__ static void scan_topk_init(int &cnt, int &topk_n,
                                                      uint64_t &kth_key,
                                                      uint32_t &kth_row) {
	if (threadIdx.x == 0) {
		cnt = 0;
		topk_n = 0;
		kth_key = ~0ULL;
		kth_row = ~0u;
	}
	__syncthreads();
}

// Epilogue: block winners as Cand{dist, id} (pad with +inf) for k_merge.
__device__ __forceinline__ static void scan_topk_write(
    const LCand *topk, int topk_n, uint32_t k,
    const uint64_t *__restrict__ ids, Cand *__restrict__ block_out) {
	if (threadIdx.x < MAX_K && threadIdx.x < k) {
		Cand c;
		if ((int)threadIdx.x < topk_n) {
			c.dist = topk[threadIdx.x].dist;
			c.id = ids[topk[threadIdx.x].row];
		} else {
			c.dist = __longlong_as_double(0x7FF0000000000000LL); // +inf
			c.id = ~0ULL;
		}
		block_out[(uint64_t)blockIdx.x * k + threadIdx.x] = c;
	}
}

// MASKED (the filtered call) gives a row one more reason to
// be invalid. mask holds n_pad / 64 words with no bit set at or past n (the
// host clears the tail and zero-fills behind it). A lane's ROWS_PER_LANE rows
// start at a multiple of 4, so their bits are one nibble of one word; a wave
// covers 256 consecutive rows = four words, and when none of its lanes has a
// live row the wave skips the feature loop: no corpus loads, no arithmetic.
// The branch is wave-uniform (a ballot) and encloses only the feature loop,
// never a __syncthreads(). Without MASKED, mask is never read (nullptr).
template <int METRIC, bool MASKED>
__global__ __launch_bounds__(THREADS) void k_scan(
    const float *__restrict__ cm, const double *__restrict__ norms,
    uint64_t n, uint64_t n_pad, uint32_t d, const float *__restrict__ qg,
    double q_norm, uint32_t k, uint64_t rows_per_block,
    Cand *__restrict__ block_out, const uint64_t *__restrict__ ids,
    const uint64_t *__restrict__ mask) {
	__shared__ float qs[MAX_D];
	__shared__ LCand buf[TILE + MAX_K];
	__shared__ LCand topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth_key;
	__shared__ uint32_t kth_row;

	for (uint32_t i = threadIdx.x; i < d; i += THREADS)
		qs[i] = qg[i];
	scan_topk_init(cnt, topk_n, kth_key, kth_row);

	uint64_t row_begin = (uint64_t)blockIdx.x * rows_per_block;
	uint64_t row_end = row_begin + rows_per_block;
	if (row_end > n)
		row_end = n;

	for (uint64_t tile_base = row_begin; tile_base < row_end; tile_base += TILE) {
		uint64_t r0 = tile_base + (uint64_t)threadIdx.x * ROWS_PER_LANE;
		double dist[ROWS_PER_LANE];
		bool valid[ROWS_PER_LANE];
		bool live = true;
		if constexpr (MASKED) {
			// r0 < n_pad: tile_base is a multiple of TILE below n <= n_pad
			const uint32_t nib = (uint32_t)(mask[r0 >> 6] >> (r0 & 63)) & 0xFu;
			bool any = false;
#pragma unroll
			for (int c = 0; c < ROWS_PER_LANE; c++) {
				valid[c] = (r0 + c) < row_end && ((nib >> c) & 1u);
				any = any || valid[c];
				dist[c] = 0.0;
			}
			live = __ballot(any) != 0ULL;
		} else {
#pragma unroll
			for (int c = 0; c < ROWS_PER_LANE; c++)
				valid[c] = (r0 + c) < row_end;
		}

		if (live) {
			if (METRIC == 0) {
				// cosine: ndarray unrolled_dot restatement, per row (float4 =
				// 4 rows)
				float4 p[8];
#pragma unroll
				for (int j = 0; j < 8; j++)
					p[j] = make_float4(0.f, 0.f, 0.f, 0.f);
				uint32_t k8 = 0;
				for (; k8 + 8 <= d; k8 += 8) {
#pragma unroll
					for (uint32_t j = 0; j < 8; j++) {
						const float4 v = *(const float4 *)(cm +
						    (uint64_t)(k8 + j) * n_pad + r0);
						const float qk = qs[k8 + j];
						p[j].x = __fadd_rn(p[j].x, __fmul_rn(v.x, qk));
						p[j].y = __fadd_rn(p[j].y, __fmul_rn(v.y, qk));
						p[j].z = __fadd_rn(p[j].z, __fmul_rn(v.z, qk));
						p[j].w = __fadd_rn(p[j].w, __fmul_rn(v.w, qk));
					}
				}
				float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#define COMB(f)                                                                 \
	sum.f = __fadd_rn(sum.f, __fadd_rn(p[0].f, p[4].f));                        \
	sum.f = __fadd_rn(sum.f, __fadd_rn(p[1].f, p[5].f));                        \
	sum.f = __fadd_rn(sum.f, __fadd_rn(p[2].f, p[6].f));                        \
	sum.f = __fadd_rn(sum.f, __fadd_rn(p[3].f, p[7].f));
				COMB(x) COMB(y) COMB(z) COMB(w)
#undef COMB
				for (; k8 < d; k8++) {
					const float4 v =
					    *(const float4 *)(cm + (uint64_t)k8 * n_pad + r0);
					const float qk = qs[k8];
					sum.x = __fadd_rn(sum.x, __fmul_rn(v.x, qk));
					sum.y = __fadd_rn(sum.y, __fmul_rn(v.y, qk));
					sum.z = __fadd_rn(sum.z, __fmul_rn(v.z, qk));
					sum.w = __fadd_rn(sum.w, __fmul_rn(v.w, qk));
				}
				const float s[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
				for (int c = 0; c < ROWS_PER_LANE; c++) {
					double den = q_norm * norms[r0 + c < n_pad ? r0 + c : 0];
					dist[c] = 1.0 - (double)s[c] / den;
				}
			} else {
				// euclidean: ndarray-stats sq_l2_dist — sequential f32 chain
				// per row
				float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
				for (uint32_t kk = 0; kk < d; kk++) {
					const float4 v =
					    *(const float4 *)(cm + (uint64_t)kk * n_pad + r0);
					const float qk = qs[kk];
					float dx = v.x - qk, dy = v.y - qk, dz = v.z - qk,
					      dw = v.w - qk;
					acc.x = __fadd_rn(acc.x, __fmul_rn(dx, dx));
					acc.y = __fadd_rn(acc.y, __fmul_rn(dy, dy));
					acc.z = __fadd_rn(acc.z, __fmul_rn(dz, dz));
					acc.w = __fadd_rn(acc.w, __fmul_rn(dw, dw));
				}
				const float s[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
				for (int c = 0; c < ROWS_PER_LANE; c++)
					dist[c] = sqrt((double)s[c]);
			}
		}

		// threshold check + candidate append (rare path)
		uint64_t kk_key = kth_key;
		uint32_t kk_row = kth_row;
		int full = (topk_n >= (int)k);
#pragma unroll
		for (int c = 0; c < ROWS_PER_LANE; c++) {
			if (!valid[c])
				continue;
			uint64_t key = d_total_key(dist[c]);
			uint32_t row32 = (uint32_t)(r0 + c); // row index within shard
			bool take = !full || key < kk_key || (key == kk_key && row32 < kk_row);
			if (take) {
				int idx = atomicAdd(&cnt, 1);
				buf[idx].key = key;
				buf[idx].dist = dist[c];
				buf[idx].row = row32;
			}
		}
		__syncthreads();

		// fold: all threads select the new top-k from {candidates, current
		// topk}. The LCand twin of pf_topk_fold, written here: k_scan is its
		// one user, and as a helper it costs k_scan<0, false> two VGPRs
		// (profiles/scan_refactor.md).
		if (cnt > 0) {
			int m = cnt;
			for (int i = threadIdx.x; i < topk_n; i += THREADS)
				buf[m + i] = topk[i];
			int total = m + topk_n;
			__syncthreads();
			int new_n;
			block_select_topk(buf, total, topk, (int)k, &new_n);
			if (threadIdx.x == 0) {
				topk_n = new_n;
				if (new_n >= (int)k) {
					kth_key = topk[k - 1].key;
					kth_row = topk[k - 1].row;
				}
				cnt = 0;
			}
		}
		__syncthreads();
	}

	scan_topk_write(topk, topk_n, k, ids, block_out);
}

// Exact k-selection over a candidate slab, in one pass over its entries.
// Each BLOCK merges its slice [per_block*g, per_block*(g+1)) into
// out[g*k..]: grid 1 with per_block = total is the classic single-block
// merge; a two-level tree (G slices, then one block over G*k) cuts the
// 1954-block scan's merge latency (top-k of per-slice top-ks == the global
// top-k, exactly). The input is read once and never written.
//
// block_select_slice<NT, E> is the body, for a block of NT threads. A thread
// holds E strided entries of a chunk of NT * E in registers, as
// (total_key(dist), id), plus one survivor of the chunks before it. The
// block walks the 128-bit (key, id) from its top byte with a 256-bin LDS
// histogram over the entries under the prefix found so far, until the bin it
// steps into holds exactly the entries still needed (at most 16 passes of
// three barriers; the bytes all keys share are skipped). Entries below the
// prefix and as many under it as are still needed go to LDS: at most k, and
// entries that tie through all 16 bytes are the same value. The survivors of
// the last chunk are ordered by rank counting and written with their dist
// restored from the key (the key is a bijection of the bits). An entry
// {all-ones NaN, ~0} never compared below the old round loop's start value
// and is left out here as it was there. The round loop poisoned a winner
// with the pad value {+inf, ~0}, which then won every later round against
// an entry above it (a positive NaN): such an entry came out in slot 0 or
// not at all, the pad in its place, and so it does here. No barrier or memory round trip
// depends on k. out may be LDS or global; a closing barrier makes it
// visible to the block.
struct SliceSel {
	uint32_t hist[256];
	uint32_t wsum[4];
	unsigned long long k_and, k_or;
	uint64_t pk, pid; // the prefix: bytes of passes < pass, zero below
	uint32_t need;    // entries still to take from under the prefix
	uint32_t state;   // 0 walking, 1 prefix final after pend, 2 take all
	uint32_t pend;
	uint32_t nsel, neq;
	uint64_t skey[MAX_K], sid[MAX_K];
};

// Whether (key, id) lies under the prefix of passes 0..p-1.
__device__ __forceinline__ static bool slice_under(uint64_t key, uint64_t id,
                                                   uint64_t pk, uint64_t pid,
                                                   uint32_t p) {
	if (p == 0)
		return true;
	if (p < 8)
		return (key >> (64 - 8 * p)) == (pk >> (64 - 8 * p));
	if (key != pk)
		return false;
	if (p == 8)
		return true;
	return (id >> (128 - 8 * p)) == (pid >> (128 - 8 * p));
}

// Whether (key, id) lies below the prefix of passes 0..p-1 (p >= 1).
__device__ __forceinline__ static bool slice_below(uint64_t key, uint64_t id,
                                                   uint64_t pk, uint64_t pid,
                                                   uint32_t p) {
	if (p <= 8)
		return p == 8 ? key < pk : (key >> (64 - 8 * p)) < (pk >> (64 - 8 * p));
	if (key != pk)
		return key < pk;
	return p == 16 ? id < pid
	               : (id >> (128 - 8 * p)) < (pid >> (128 - 8 * p));
}

template <int NT, int E>
__device__ __forceinline__ static void block_select_slice(
    const Cand *__restrict__ in, uint64_t len, uint32_t k, Cand *out,
    SliceSel *S) {
	static_assert(NT >= MAX_K && NT <= 256 && 256 % NT == 0 && E < 32, "");
	constexpr int BPT = 256 / NT; // histogram bins a thread owns
	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63, wave = tid >> 6;
	uint64_t ek[E + 1], eid[E + 1];
	uint32_t vm = 0; // valid entries; bit E is the carried survivor

	for (uint64_t c0 = 0; c0 == 0 || c0 < len; c0 += (uint64_t)NT * E) {
		vm &= 1u << E;
#pragma unroll
		for (int e = 0; e < E; e++) {
			const uint64_t i = c0 + (uint64_t)e * NT + tid;
			ek[e] = ~0ULL;
			eid[e] = ~0ULL;
			if (i < len) {
				const Cand c = in[i];
				ek[e] = d_total_key(c.dist);
				eid[e] = c.id;
				if (ek[e] != ~0ULL || eid[e] != ~0ULL)
					vm |= 1u << e;
			}
		}
		// the bytes every key shares need no pass
		uint64_t ka = ~0ULL, ko = 0;
#pragma unroll
		for (int e = 0; e <= E; e++)
			if ((vm >> e) & 1u) {
				ka &= ek[e];
				ko |= ek[e];
			}
		for (int off = 32; off > 0; off >>= 1) {
			ka &= __shfl_xor(ka, off);
			ko |= __shfl_xor(ko, off);
		}
		if (tid == 0) {
			S->k_and = ~0ULL;
			S->k_or = 0;
			S->nsel = 0;
			S->neq = 0;
			S->state = 0;
		}
#pragma unroll
		for (int b = 0; b < BPT; b++)
			S->hist[tid * BPT + b] = 0;
		__syncthreads();
		if (lane == 0) {
			atomicAnd(&S->k_and, (unsigned long long)ka);
			atomicOr(&S->k_or, (unsigned long long)ko);
		}
		__syncthreads();
		const uint64_t kx = S->k_and ^ S->k_or;
		// all keys equal (or no entry at all): the walk starts on the ids
		uint32_t p = S->k_and > S->k_or ? 0u
		             : kx == 0         ? 8u
		                               : (uint32_t)__clzll((long long)kx) / 8u;
		uint64_t pk = p == 0 ? 0 : S->k_and & (~0ULL << (64 - 8 * p));
		uint64_t pid = 0;
		uint32_t need = k;
		uint32_t state = 0;

		for (; p < 16; p++) {
			const uint32_t sh = p < 8 ? 56 - 8 * p : 120 - 8 * p;
#pragma unroll
			for (int e = 0; e <= E; e++)
				if (((vm >> e) & 1u) &&
				    slice_under(ek[e], eid[e], pk, pid, p))
					atomicAdd(&S->hist[((p < 8 ? ek[e] : eid[e]) >> sh) & 255u],
					          1u);
			__syncthreads();
			uint32_t c[BPT], mine = 0;
#pragma unroll
			for (int b = 0; b < BPT; b++) {
				c[b] = S->hist[tid * BPT + b];
				S->hist[tid * BPT + b] = 0; // own bins: ready for the next pass
				mine += c[b];
			}
			uint32_t incl = mine;
			for (int off = 1; off < 64; off <<= 1) {
				const uint32_t o = __shfl_up(incl, off);
				if (lane >= (uint32_t)off)
					incl += o;
			}
			if (lane == 63)
				S->wsum[wave] = incl;
			__syncthreads();
			uint32_t acc = incl - mine, total = 0;
#pragma unroll
			for (int w = 0; w < NT / 64; w++) {
				const uint32_t ws = S->wsum[w];
				acc += (uint32_t)w < wave ? ws : 0u;
				total += ws;
			}
			if (total < need) { // only before the first step: fewer than k
				if (tid == 0)
					S->state = 2;
			} else {
#pragma unroll
				for (int b = 0; b < BPT; b++) {
					if (c[b] != 0 && acc < need && acc + c[b] >= need) {
						const uint64_t dg = (uint64_t)(tid * BPT + b) << sh;
						S->pk = p < 8 ? pk | dg : pk;
						S->pid = p < 8 ? 0 : pid | dg;
						S->need = need - acc;
						S->pend = p + 1;
						S->state = (c[b] == need - acc || p == 15) ? 1u : 0u;
					}
					acc += c[b];
				}
			}
			__syncthreads();
			state = S->state;
			if (state == 2)
				break;
			pk = S->pk;
			pid = S->pid;
			need = S->need;
			if (state == 1)
				break;
		}
		// state 0 here: every entry ties on the key and the walk never ran
		// (p started at 16 cannot happen; p == 8 start always steps), so
		// state is 1 or 2
		const uint32_t pend = state == 1 ? S->pend : 0;
#pragma unroll
		for (int e = 0; e <= E; e++) {
			if (!((vm >> e) & 1u))
				continue;
			bool take = state == 2;
			if (!take) {
				take = slice_below(ek[e], eid[e], pk, pid, pend);
				if (!take && slice_under(ek[e], eid[e], pk, pid, pend))
					take = atomicAdd(&S->neq, 1u) < need;
			}
			if (take) {
				const uint32_t pos = atomicAdd(&S->nsel, 1u);
				if (pos < MAX_K) { // always: at most k are taken
					S->skey[pos] = ek[e];
					S->sid[pos] = eid[e];
				}
			}
		}
		__syncthreads();
		const uint32_t m = S->nsel;
		if (c0 + (uint64_t)NT * E < len) { // carry the survivors
			vm = 0;
			if (tid < m) {
				ek[E] = S->skey[tid];
				eid[E] = S->sid[tid];
				vm = 1u << E;
			}
			__syncthreads();
			continue;
		}
		// last chunk: order by rank counting, ties broken by LDS position
		if (tid < m) {
			const uint64_t kt = S->skey[tid], it = S->sid[tid];
			uint32_t rank = 0;
			for (uint32_t j = 0; j < m; j++) {
				const uint64_t kj = S->skey[j], ij = S->sid[j];
				rank += (kj < kt ||
				         (kj == kt && (ij < it || (ij == it && j < tid))))
				            ? 1u
				            : 0u;
			}
			Cand o;
			o.dist = __longlong_as_double(
			    (long long)((kt >> 63) ? (kt & 0x7FFFFFFFFFFFFFFFULL) : ~kt));
			o.id = it;
			if (rank > 0 && kt > 0xFFF0000000000000ULL) { // above the pad
				o.dist = __longlong_as_double(0x7FF0000000000000LL);
				o.id = ~0ULL;
			}
			out[rank] = o;
		} else if (tid < k) { // slice shorter than k: pad
			Cand o;
			o.dist = __longlong_as_double(0x7FF0000000000000LL);
			o.id = ~0ULL;
			out[tid] = o;
		}
		__syncthreads();
	}
}

__device__ __forceinline__ static void merge_slice(
    const Cand *__restrict__ block_out, uint64_t total, uint32_t k,
    uint64_t per_block, Cand *__restrict__ out) {
	__shared__ SliceSel sel;
	const uint64_t s0 = (uint64_t)blockIdx.x * per_block;
	const uint64_t s1 = s0 + per_block < total ? s0 + per_block : total;
	out += (uint64_t)blockIdx.x * k;
	if (s0 >= total) {
		for (uint32_t i = threadIdx.x; i < k; i += THREADS) {
			out[i].dist = __longlong_as_double(0x7FF0000000000000LL);
			out[i].id = ~0ULL;
		}
		return;
	}
	block_select_slice<THREADS, 16>(block_out + s0, s1 - s0, k, out, &sel);
}

__global__ __launch_bounds__(THREADS) void k_merge(
    const Cand *__restrict__ block_out, uint64_t total, uint32_t k,
    uint64_t per_block, Cand *__restrict__ out) {
	merge_slice(block_out, total, k, per_block, out);
}

// ---------------------------------------------------------------------------
// Single-query cosine prefilter: stream a bf16 shadow of the corpus (half the
// bytes of the f32 store), keep every row whose approximate distance could
// reach the top K under the proven bound pf_eps(d), and recompute only those
// rows with the exact restated chain. Results are bit-identical to k_scan<0, .>
// by construction: the approximate scores only decide WHICH rows get the
// exact chain, never a result value or an order.
// ---------------------------------------------------------------------------
#define PF_ROWS_PER_LANE 8
#define PF_TILE (THREADS * PF_ROWS_PER_LANE) /* 2048 rows per block-sweep */
#define PF_CAND_CAP 16384u
#define PF_RESCORE_BLOCKS 2048
// Norm window (rows and query) in which neither chain can overflow and
// underflow stays negligible: |x_k| <= norm <= 2^30, so every product is
// <= 2^60 and every partial sum <= MAX_D * 2^60 < 2^73; norm products are
// >= 2^-60, so the <= 2^-149 absolute error of an underflowed product or
// of a bf16-subnormal rounding is < 2^-75 in cosine units.
#define PF_NORM_MIN 0x1p-30
#define PF_NORM_MAX 0x1p30

// Upper 16 bits of a FINITE f32 rounded to nearest-even bf16 (a carry out of
// the mantissa propagates into the exponent; 0x7F80 = overflowed to inf).
__host__ __device__ static inline uint32_t pf_bf16_bits(uint32_t u) {
	return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// Bound on |exact - approx| for a row and a query inside the norm window,
// exact = the restated f32 chain with its f64 finish (k_scan<0, .>),
// approx = 1 - s~ * inv_q * inv_i in f32 over the bf16 shadow (k_prefilter).
// In cosine units, i.e. divided by |x||q|, with u = 2^-24:
//  - quantisation: bf16 keeps 8 significant bits, so round-to-nearest moves
//    x_k by at most 2^-8 |x_k| (unit roundoff 2^-8, not 2^-9); by
//    Cauchy-Schwarz |sum (x~_k - x_k) q_k| <= 2^-8 |x||q|.
//  - accumulation: a d-term f32 dot in any order, fused or mul-then-add, is
//    within gamma(d + 8) <= 1.001 (d + 8) u of its exact sum relative to
//    sum |x_k q_k| <= |x||q| (the + 8 covers the partial-sum combine and the
//    product roundings of the unfused chain); the shadow chain's terms are
//    up to (1 + 2^-8) larger. Both chains: <= 2.006 (d + 8) u.
//  - norms: both sides divide by the SAME computed norms, which are within
//    (d + 8) u of the true ones, so the two terms above grow by at most
//    1 + 2 (d + 8) u <= 1.0005. The factor 1.01 below covers all of these.
//  - finish: inv_q, inv_i and the two f32 products round 4 times (4.1 u on
//    |cos| <= 1.001), the final subtraction rounds a value below 2.01
//    (<= 2u), f64 steps are ~2^-52: together < 7u < 2^-21. 2^-20 leaves the
//    rest for the underflow terms bounded at PF_NORM_MIN.
// Holds for every d <= MAX_D (e(4096) ~ 0.0044).
__host__ __device__ static inline float pf_eps(uint32_t d) {
	return 1.01f * (0x1p-8f + 2.0f * (float)(d + 8) * 0x1p-24f) + 0x1p-20f;
}

// f32 total order key and its inverse (same construction as d_total_key).
__device__ static inline uint32_t d_key32(float x) {
	uint32_t b = __float_as_uint(x);
	return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ static inline float d_unkey32(uint32_t k) {
	return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k);
}

// Build the shadow: one lane converts 8 consecutive rows per feature (two
// float4 loads, one 16-byte store). pinv[r] = f32 1/norm, or NaN when the
// bound cannot cover row r: a non-finite element, a bf16 rounding that
// overflows, a norm outside [PF_NORM_MIN, PF_NORM_MAX] (zero and non-finite
// norms included), or a padding row. row0 (a multiple of 256) is the first
// row of the launch, here and in the three builders below: 0 for a whole
// shadow, the block that holds the first new row after an in-place append.
// blist, when not null, lists 256-row blocks (row / 256, sdbv_update_rows)
// and replaces the contiguous range: workgroup j of the three builders below
// works on block blist[j], and here lane group j of n_list does.
__global__ void k_shadow(const float *__restrict__ cm,
                         const double *__restrict__ norms,
                         uint16_t *__restrict__ sh, float *__restrict__ pinv,
                         uint64_t n, uint64_t n_pad, uint64_t sn_pad,
                         uint32_t d, uint64_t row0,
                         const uint32_t *__restrict__ blist, uint32_t n_list) {
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t r0 = row0 + g * PF_ROWS_PER_LANE;
	if (blist) { // 256 / PF_ROWS_PER_LANE lanes per listed block
		const uint64_t j = g / (256 / PF_ROWS_PER_LANE);
		if (j >= n_list)
			return;
		r0 = (uint64_t)blist[j] * 256 +
		     g % (256 / PF_ROWS_PER_LANE) * PF_ROWS_PER_LANE;
	}
	if (r0 >= sn_pad)
		return;
	const bool in_cm = r0 < n_pad; // n_pad % 8 == 0: a group is all in or out
	uint32_t bad = 0;
	for (uint32_t k = 0; k < d; k++) {
		float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
		if (in_cm) {
			a = *(const float4 *)(cm + (uint64_t)k * n_pad + r0);
			b = *(const float4 *)(cm + (uint64_t)k * n_pad + r0 + 4);
		}
		const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
		uint32_t h[8];
#pragma unroll
		for (int c = 0; c < 8; c++) {
			uint32_t u = __float_as_uint(v[c]);
			h[c] = pf_bf16_bits(u) & 0xFFFFu;
			if ((u & 0x7F800000u) == 0x7F800000u ||
			    (h[c] & 0x7F80u) == 0x7F80u)
				bad |= 1u << c;
		}
		uint4 o;
		o.x = h[0] | (h[1] << 16);
		o.y = h[2] | (h[3] << 16);
		o.z = h[4] | (h[5] << 16);
		o.w = h[6] | (h[7] << 16);
		*(uint4 *)(sh + (uint64_t)k * sn_pad + r0) = o;
	}
#pragma unroll
	for (int c = 0; c < 8; c++) {
		uint64_t r = r0 + c;
		float inv = __uint_as_float(0x7FC00000u); // NaN = always rescore
		if (r < n && !((bad >> c) & 1u)) {
			double nm = norms[r];
			if (nm >= PF_NORM_MIN && nm <= PF_NORM_MAX)
				inv = (float)(1.0 / nm);
		}
		pinv[r] = inv;
	}
}

// Block-wide exact k-selection of the smallest packed (key32 << 32 | row)
// values (all distinct, all < ~0); same hand-off discipline as
// block_select_topk.
__device__ static void pf_block_select(uint64_t *buf, int total,
                                       uint64_t *topk, int k, int *out_n) {
	__shared__ uint64_t red_v[THREADS / 64];
	__shared__ int red_i[THREADS / 64];
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	int out = total < k ? total : k;
	for (int slot = 0; slot < out; slot++) {
		uint64_t bv = ~0ULL;
		int bi = -1;
		for (int i = threadIdx.x; i < total; i += THREADS) {
			uint64_t cv = buf[i];
			if (cv < bv) {
				bv = cv;
				bi = i;
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			uint64_t ov = __shfl_down(bv, off);
			int oi = __shfl_down(bi, off);
			if (ov < bv) {
				bv = ov;
				bi = oi;
			}
		}
		if (lane == 0) {
			red_v[wave] = bv;
			red_i[wave] = bi;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			uint64_t bbv = ~0ULL;
			int best = -1;
			for (int w = 0; w < THREADS / 64; w++)
				if (red_i[w] >= 0 && red_v[w] < bbv) {
					bbv = red_v[w];
					best = red_i[w];
				}
			topk[slot] = bbv;
			buf[best] = ~0ULL;
		}
		__syncthreads();
	}
	*out_n = out;
}

// The running block top-K of the three prefilter kernels, on packed keys:
// prologue, fold and epilogue, the packed-u64 twins of k_scan's, with the
// state in each kernel's own __shared__ declarations. Block 0's prologue
// also clears the candidate counter for k_pf_compact. Fold, once every
// thread has appended its survivors to buf[0..cnt) (at most PF_TILE of them
// into buf[PF_TILE + MAX_K]): if there are any, all threads select the new
// top-k from {candidates, current topk} and thread 0 moves the threshold.
__device__ __forceinline__ static void pf_topk_init(
    int &cnt, int &topk_n, uint64_t &kth, uint32_t *__restrict__ cand_cnt) {
	if (threadIdx.x == 0) {
		cnt = 0;
		topk_n = 0;
		kth = ~0ULL;
		if (blockIdx.x == 0)
			*cand_cnt = 0;
	}
	__syncthreads();
}

__device__ __forceinline__ static void pf_topk_fold(uint64_t *buf,
                                                    uint64_t *topk, int &cnt,
                                                    int &topk_n, uint64_t &kth,
                                                    uint32_t k) {
	__syncthreads();
	if (cnt > 0) {
		int m = cnt;
		for (int i = threadIdx.x; i < topk_n; i += THREADS)
			buf[m + i] = topk[i];
		int total = m + topk_n;
		__syncthreads();
		int new_n;
		pf_block_select(buf, total, topk, (int)k, &new_n);
		if (threadIdx.x == 0) {
			topk_n = new_n;
			if (new_n >= (int)k)
				kth = topk[k - 1];
			cnt = 0;
		}
	}
	__syncthreads();
}

// Block winners as Cand{approximate distance or upper bound, row} (pad with
// +inf), so that k_merge selects the K smallest of them.
__device__ __forceinline__ static void pf_topk_write(
    const uint64_t *topk, int topk_n, uint32_t k, Cand *__restrict__ block_out) {
	if (threadIdx.x < k) {
		Cand c;
		if ((int)threadIdx.x < topk_n) {
			c.dist = (double)d_unkey32((uint32_t)(topk[threadIdx.x] >> 32));
			c.id = (uint32_t)topk[threadIdx.x];
		} else {
			c.dist = __longlong_as_double(0x7FF0000000000000LL); // +inf
			c.id = ~0ULL;
		}
		block_out[(uint64_t)blockIdx.x * k + threadIdx.x] = c;
	}
}

// The k_scan skeleton over the shadow: contiguous row spans per block, 8
// rows per lane from one 16-byte load per feature, unpack by shift, f32 FMA
// accumulation, a_i = 1 - s~ * inv_q * inv_i stored to scores[] and fed to
// the block top-K. Rows the bound cannot cover (pinv NaN) and non-finite
// scores are stored as -inf, so k_pf_compact always passes them on, and are
// kept OUT of the top-K: the threshold must come from K rows that do carry
// the bound. Block 0 also clears the candidate counter for k_pf_compact.
//
// MASKED (the filtered call), in all three prefilter kernels:
// mask holds sn_pad / 64 words, no bit set at or past n. A row whose bit is
// clear is invalid for the block top-K like a row past row_end, and its
// score is stored as NaN, which k_pf_compact never passes, not even against
// a threshold of +inf; -inf stays what it is, an ALLOWED row the bound does
// not cover. Every row below n is written by every call, so no score of an
// earlier call survives. A wave none of whose rows is allowed skips the
// loads and the accumulation: a wave-uniform branch (a ballot) around the
// feature loop alone, never around a barrier or the scores[] store. Here a
// lane's 8 rows are one byte of one mask word, a wave's 512 rows 8 words.
// Without MASKED, mask is never read (nullptr).
template <bool MASKED>
__global__ __launch_bounds__(THREADS) void k_prefilter(
    const uint16_t *__restrict__ sh, const float *__restrict__ pinv,
    uint64_t n, uint64_t sn_pad, uint32_t d, const float *__restrict__ qg,
    float inv_qnorm, uint32_t k, uint64_t rows_per_block,
    float *__restrict__ scores, Cand *__restrict__ block_out,
    uint32_t *__restrict__ cand_cnt, const uint64_t *__restrict__ mask) {
	__shared__ uint64_t buf[PF_TILE + MAX_K];
	__shared__ uint64_t topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth;

	pf_topk_init(cnt, topk_n, kth, cand_cnt);

	uint64_t row_begin = (uint64_t)blockIdx.x * rows_per_block;
	uint64_t row_end = row_begin + rows_per_block;
	if (row_end > n)
		row_end = n;
	const float ninf = __uint_as_float(0xFF800000u);
	const float qnan = __uint_as_float(0x7FC00000u);

	for (uint64_t tile_base = row_begin; tile_base < row_end;
	     tile_base += PF_TILE) {
		const uint64_t r0 =
		    tile_base + (uint64_t)threadIdx.x * PF_ROWS_PER_LANE;
		const uint16_t *p = sh + r0;
		float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
		uint32_t mb = 0xFFu; // the lane's 8 mask bits
		bool live = true;
		if constexpr (MASKED) {
			// r0 + 8 <= tile_base + PF_TILE <= sn_pad
			mb = (uint32_t)(mask[r0 >> 6] >> (r0 & 63)) & 0xFFu;
			live = __ballot(mb != 0u) != 0ULL;
		}
#define PF_ACC(V, qk)                                                          \
	acc[0] = __fmaf_rn(__uint_as_float((V).x << 16), qk, acc[0]);              \
	acc[1] = __fmaf_rn(__uint_as_float((V).x & 0xFFFF0000u), qk, acc[1]);      \
	acc[2] = __fmaf_rn(__uint_as_float((V).y << 16), qk, acc[2]);              \
	acc[3] = __fmaf_rn(__uint_as_float((V).y & 0xFFFF0000u), qk, acc[3]);      \
	acc[4] = __fmaf_rn(__uint_as_float((V).z << 16), qk, acc[4]);              \
	acc[5] = __fmaf_rn(__uint_as_float((V).z & 0xFFFF0000u), qk, acc[5]);      \
	acc[6] = __fmaf_rn(__uint_as_float((V).w << 16), qk, acc[6]);              \
	acc[7] = __fmaf_rn(__uint_as_float((V).w & 0xFFFF0000u), qk, acc[7]);
		if (live) {
			uint32_t kk = 0;
			for (; kk + 8 <= d; kk += 8) {
				uint4 w[8];
#pragma unroll
				for (uint32_t j = 0; j < 8; j++)
					w[j] = *(const uint4 *)(p + (uint64_t)(kk + j) * sn_pad);
#pragma unroll
				for (uint32_t j = 0; j < 8; j++) {
					const float qk = qg[kk + j]; // uniform: scalar load
					PF_ACC(w[j], qk)
				}
			}
			for (; kk < d; kk++) {
				const uint4 w1 = *(const uint4 *)(p + (uint64_t)kk * sn_pad);
				const float qk = qg[kk];
				PF_ACC(w1, qk)
			}
		}
#undef PF_ACC
		const float4 i0 = *(const float4 *)(pinv + r0);
		const float4 i1 = *(const float4 *)(pinv + r0 + 4);
		const float inv[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
		float a[8];
		bool ok[8];
#pragma unroll
		for (int c = 0; c < 8; c++) {
			float s = 1.0f - acc[c] * inv_qnorm * inv[c];
			ok[c] = (r0 + c) < row_end &&
			        (__float_as_uint(s) & 0x7F800000u) != 0x7F800000u;
			a[c] = ok[c] ? s : ninf;
			if constexpr (MASKED) {
				const bool allowed = (mb >> c) & 1u;
				ok[c] = ok[c] && allowed;
				a[c] = allowed ? a[c] : qnan;
			}
		}
		*(float4 *)(scores + r0) = make_float4(a[0], a[1], a[2], a[3]);
		*(float4 *)(scores + r0 + 4) = make_float4(a[4], a[5], a[6], a[7]);

		// threshold check + candidate append (rare path)
		const uint64_t kthv = kth;
		const int full = (topk_n >= (int)k);
#pragma unroll
		for (int c = 0; c < 8; c++) {
			if (!ok[c])
				continue;
			uint64_t v = ((uint64_t)d_key32(a[c]) << 32) | (uint32_t)(r0 + c);
			if (!full || v < kthv) {
				int idx = atomicAdd(&cnt, 1);
				buf[idx] = v;
			}
		}
		pf_topk_fold(buf, topk, cnt, topk_n, kth, k);
	}

	pf_topk_write(topk, topk_n, k, block_out);
}

// ---------------------------------------------------------------------------
// Int8 tier of the prefilter: a quarter of the f32 store's bytes. Row r is
// stored as symmetric codes c_k in [-127, 127] with one f32 scale_r =
// maxabs_r / 127, as bias-128 bytes b_k = c_k + 128 so that one
// v_cvt_f32_ubyteN unpacks an element; the kernel accumulates sum b_k q_k
// and removes 128 * sum q_k once per row. Each row carries its own proven
// bound peps[r] (below) instead of the global pf_eps(d).
// ---------------------------------------------------------------------------
#define PF8_ROWS_PER_LANE 16
#define PF8_TILE (THREADS * PF8_ROWS_PER_LANE) /* 4096 rows per block-sweep */

// Quantise one row (elements x[k * xstride], k < d; norm = the row's staged
// f64 norm) and derive its bound. The one routine behind both k_shadow_i8
// and sdbv_prefilter_i8_row. Writes the d stored bytes to codes[k * cstride],
// *scale, *pscale = f32(scale / norm) and *eps. A row the bound cannot cover
// (a non-finite element, a norm outside [PF_NORM_MIN, PF_NORM_MAX], which
// includes the zero row and a non-finite norm) gets zero codes (byte 128),
// scale = pscale = NaN and eps = 0: the prefilter always rescores it.
//
// Bound on |exact - approx| for a covered row and a query inside the norm
// window, exact = the restated f32 chain with its f64 finish (k_scan<0, .>),
// approx = 1 - (t - B) * inv_q * pscale in f32 (k_prefilter_i8), where
// t = the sequential f32 FMA chain over b_k q_k and B = f32(128 sum q_k).
// In cosine units, i.e. divided by |x||q|, with u = 2^-24:
//  - quantisation: |sum (x_k - scale c_k) q_k| <= |x - scale c| |q| by
//    Cauchy-Schwarz, i.e. rho = |x - scale c| / |x|, the row's ACTUAL
//    residual: computed here in f64 from the f32 elements and the products
//    scale * c_k (31 significant bits: exact in f64) and rounded up
//    (the d + 3 f64 roundings are below 2^-40 relative).
//  - exact chain: within 1.001 (d + 8) u of its exact sum relative to
//    sum |x_k q_k| <= |x||q|, as for pf_eps.
//  - approx chain: t carries d FMA roundings on terms b_k |q_k| <= 255 |q_k|:
//    |t - sum b_k q_k| <= 1.001 d u 255 |q|_1. B is an f64 sum rounded once
//    to f32: <= 1.001 u 128 |q|_1. The subtraction t - B rounds once on
//    |sum c_k q_k| + the above <= 1.01 * 127 |q|_1. Together
//    <= 1.001 (d + 2) u 255 |q|_1, and |q|_1 <= sqrt(d) |q|. Scaled by
//    scale / |x| = maxabs / (127 |x|) this is
//    <= 2.012 (d + 2) u sqrt(d) maxabs / |x| in cosine units: the price of
//    the cancelled bias, per row because it depends on maxabs_r / norm_r.
//  - norms: rho and maxabs / |x| are taken against the computed norm, both
//    chains divide by the same computed norms, within (d + 8) u of the true
//    ones: the factor 1.01 covers it, as for pf_eps.
//  - finish: |approx cosine| <= 1 + rho <= 1.26 (each element is within
//    scale / 2 of its product, so rho <= sqrt(d) / 254 <= 0.252 at MAX_D);
//    scale, pscale, inv_q and the two f32 products round 5 times
//    (<= 6.4 u), the final subtraction rounds a value below 2.3 (<= 2.3 u),
//    and the kernel's a + eps / a - eps round once more (<= 2.6 u):
//    < 12 u < 2^-20; f64 steps and the underflow terms bounded at
//    PF_NORM_MIN are far below the remaining 4 u.
// eps = 1.01 (rho + acc) + 2^-20, acc = (d + 8) u (1.001 + 2.012 sqrt(d)
// maxabs / norm), evaluated in f64 and rounded UP to f32.
__host__ __device__ static inline void pf_i8_row(
    const float *x, uint64_t xstride, uint32_t d, double norm, uint8_t *codes,
    uint64_t cstride, float *scale, float *pscale, float *eps) {
	float m = 0.f;
	bool bad = false;
	for (uint32_t k = 0; k < d; k++) {
		const float v = x[(uint64_t)k * xstride];
		if ((__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u)
			bad = true;
		m = fmaxf(m, fabsf(v));
	}
	if (bad || !(norm >= PF_NORM_MIN && norm <= PF_NORM_MAX) || !(m > 0.f)) {
		for (uint32_t k = 0; k < d; k++)
			codes[(uint64_t)k * cstride] = 128;
		*scale = *pscale = __builtin_bit_cast(float, 0x7FC00000u);
		*eps = 0.f;
		return;
	}
	const float sc = (float)((double)m / 127.0);
	const double sd = (double)sc;
	double res2 = 0.0;
	for (uint32_t k = 0; k < d; k++) {
		const double xv = (double)x[(uint64_t)k * xstride];
		double c = rint(xv / sd);
		c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
		const double r = xv - sd * c;
		res2 += r * r;
		codes[(uint64_t)k * cstride] = (uint8_t)((int)c + 128);
	}
	const double rho = sqrt(res2) / norm * (1.0 + 0x1p-40);
	const double acc = (double)(d + 8) * 0x1p-24 *
	                   (1.001 + 2.012 * sqrt((double)d) * ((double)m / norm));
	const double e = 1.01 * (rho + acc) + 0x1p-20;
	float ef = (float)e;
	if ((double)ef < e) // round up: e is positive and finite
		ef = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, ef) + 1u);
	*scale = sc;
	*pscale = (float)(sd / norm);
	*eps = ef;
}

// Build the int8 shadow: one lane per row (coalesced f32 reads across the
// wave, two passes over the row: maxabs, then codes and residual).
__global__ void k_shadow_i8(const float *__restrict__ cm,
                            const double *__restrict__ norms,
                            uint8_t *__restrict__ sh,
                            float *__restrict__ pscale,
                            float *__restrict__ peps, uint64_t n,
                            uint64_t n_pad, uint64_t sn_pad, uint32_t d,
                            uint64_t row0,
                            const uint32_t *__restrict__ blist) {
	const uint64_t r = (blist ? (uint64_t)blist[blockIdx.x] * 256
	                          : row0 + (uint64_t)blockIdx.x * blockDim.x) +
	                   threadIdx.x;
	if (r >= sn_pad)
		return;
	float sc, ps = __uint_as_float(0x7FC00000u), pe = 0.f;
	if (r < n) {
		pf_i8_row(cm + r, n_pad, d, norms[r], sh + r, sn_pad, &sc, &ps, &pe);
	} else { // padding row: never covered
		for (uint32_t k = 0; k < d; k++)
			sh[(uint64_t)k * sn_pad + r] = 128;
	}
	pscale[r] = ps;
	peps[r] = pe;
}

// ---------------------------------------------------------------------------
// Euclidean int8 tier (Shadow::kind 5): the codes and the
// stream of the cosine int8 tier, three f32 side values per row (scale, xx,
// res) and an interval [lo, up] around the exact distance from the triangle
// inequality. With x^ = scale * c the dequantised row, D = |x - q| and
// D^ = |x^ - q| in the reals, |D - D^| <= |x - x^|.
// ---------------------------------------------------------------------------

// e > 0 finite, rounded up to f32.
__host__ __device__ static inline float pf_round_up_f32(double e) {
	float ef = (float)e;
	if ((double)ef < e)
		ef = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, ef) + 1u);
	return ef;
}

// The query's constants of the euclidean finish, computed on the host in f64
// and rounded once (pf_l2_query); they ride behind the query in ctx->q_dev.
struct PfL2Q {
	float qbias; // f32(128 sum q)
	float qq;    // f32(|q|^2)
	float c1;    // delta's factor of the row's scale, rounded up
	float c2;    // delta's factor of xx + qq
	float kl;    // 1 - rel, rounded down
	float ku;    // 1 + rel, rounded up
};
#define PF_L2_C2 0x1.5p-21f  /* 10.5 u */
#define PF_L2_C3 0x1p-112f   /* delta's absolute part */
#define PF_L2_RES_ABS 0x1p-68 /* res carries this much more than |x - x^| */

// Quantise one row for the euclidean int8 shadow (elements x[k * xstride],
// k < d). The one routine behind both k_shadow_l2 and sdbv_prefilter_l2_row.
// Codes and scale as pf_i8_row: scale = f32(maxabs / 127), c_k = rint(x_k /
// scale) clamped to +-127, stored as bias-128 bytes at codes[k * cstride].
// *xx = |x^|^2 and *res = |x - x^| + PF_L2_RES_ABS are computed in f64 from
// the f32 elements and the products scale * c_k (31 significant bits: exact
// in f64); their d + 3 f64 roundings are below 2^-40 relative. xx is rounded
// once to f32, res is rounded UP.
// Window: finite elements and an f64 norm sqrt(sum x_k^2) <= PF_NORM_MAX. A
// row outside it is uncovered: neutral codes (byte 128), scale = NaN, xx =
// res = 0, and the prefilter always rescores it. There is no lower limit:
// the zero row is covered (scale = xx = 0, zero codes, x^ = x exactly), and
// so is a row whose squares underflow, because every term of the bound below
// keeps an absolute part for it.
__host__ __device__ static inline void pf_l2_row(
    const float *x, uint64_t xstride, uint32_t d, uint8_t *codes,
    uint64_t cstride, float *scale, float *xx, float *res) {
	float m = 0.f;
	double n2 = 0.0;
	bool bad = false;
	for (uint32_t k = 0; k < d; k++) {
		const float v = x[(uint64_t)k * xstride];
		if ((__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u)
			bad = true;
		m = fmaxf(m, fabsf(v));
		n2 += (double)v * (double)v;
	}
	if (bad || !(n2 <= PF_NORM_MAX * PF_NORM_MAX)) {
		for (uint32_t k = 0; k < d; k++)
			codes[(uint64_t)k * cstride] = 128;
		*scale = __builtin_bit_cast(float, 0x7FC00000u);
		*xx = *res = 0.f;
		return;
	}
	const float sc = (float)((double)m / 127.0);
	const double sd = (double)sc;
	double res2 = 0.0, xx2 = 0.0;
	for (uint32_t k = 0; k < d; k++) {
		const double xv = (double)x[(uint64_t)k * xstride];
		// sd == 0: maxabs below 127 * 2^-150 rounds the scale to zero (the
		// zero row included); every code is 0 and the row is its residual
		double c = sd > 0.0 ? rint(xv / sd) : 0.0;
		c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
		const double xh = sd * c;
		const double r = xv - xh;
		res2 += r * r;
		xx2 += xh * xh;
		codes[(uint64_t)k * cstride] = (uint8_t)((int)c + 128);
	}
	*scale = sc;
	*xx = (float)xx2;
	*res = pf_round_up_f32(sqrt(res2) * (1.0 + 0x1p-40) + PF_L2_RES_ABS);
}

// The query side: false for a query outside the window (a non-finite
// element, or |q| above PF_NORM_MAX), which takes the exact scan. No lower
// limit: the zero query is covered (t = qbias = qq = 0 and A2 = xx).
// |q|_1, |q|^2 and sum q are f64 sums of f32 values (d + 1 roundings of
// 2^-53 each, far inside the slack of the constants).
__host__ __device__ static inline bool pf_l2_query(const float *q, uint32_t d,
                                                   PfL2Q *c) {
	double q1 = 0.0, q2 = 0.0, qs = 0.0;
	bool bad = false;
	for (uint32_t k = 0; k < d; k++) {
		if ((__builtin_bit_cast(uint32_t, q[k]) & 0x7F800000u) == 0x7F800000u)
			bad = true;
		const double v = (double)q[k];
		q1 += fabs(v);
		q2 += v * v;
		qs += v;
	}
	if (bad || !(q2 <= PF_NORM_MAX * PF_NORM_MAX))
		return false;
	const double u = 0x1p-24;
	const double g = (double)(d + 2) * u / (1.0 - (double)(d + 2) * u);
	c->qbias = (float)(128.0 * qs);
	c->qq = (float)q2;
	const double c1 = 2.01 * (double)(d + 2) * u * 255.0 * q1;
	c->c1 = c1 > 0.0 ? pf_round_up_f32(c1) : 0.f;
	c->c2 = PF_L2_C2;
	const double kl = 1.0 - (0.5001 * g + 3.0 * u); // in (0.999, 1)
	float klf = (float)kl;
	if ((double)klf > kl) // round down: the f32 below
		klf = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, klf) - 1u);
	c->kl = klf;
	c->ku = pf_round_up_f32(1.0 + 0.5 * g + 3.0 * u);
	return true;
}

// The finish of the euclidean stream, one row: the one routine behind both
// k_prefilter_i8<., true> and sdbv_prefilter_l2_interval. t = the sequential
// f32 FMA chain over b_k q_k (b_k the stored bytes). Returns A2; the caller
// treats a non-finite A2 (an uncovered row: scale NaN) as no bound.
//   w  = t - qbias                  a     = xx + qq
//   A2 = fma(-2 scale, w, a)        delta = fma(scale, c1, fma(a, c2, C3))
//   lo = max(0, sqrt(max(0, A2 - delta)) - res) * kl
//   up = (sqrt(A2 + delta) + res) * ku
// Every operation below is one f32 operation written out (fmaf, or a single
// + - * that -ffp-contract=off keeps single), so host and device agree bit
// for bit. sqrtf must be correctly rounded on the device as on the host: the
// build passes -fhip-fp32-correctly-rounded-divide-sqrt and no fast-math
// flag. f32 subnormals are kept, not flushed (the compiler's default for
// gfx9; the build passes no -fgpu-flush-denormals-to-zero).
//
// Claim: lo <= exact <= up for a covered row and a query in the window,
// exact = the chain of k_scan<1, .>: acc = the sequential f32 sum of
// fl(fl(x_k - q_k)^2), exact = sqrt((double)acc). With u = 2^-24, gamma(m) =
// m u / (1 - m u), X = |x^|^2, Q = |q|^2, C = sum c_k q_k in the reals, so
// that D^^2 = X + Q - 2 scale C exactly (scale the stored f32). Every f32
// result fl(z) is within u |z| of z, or within 2^-150 when it is subnormal
// (sums and differences are then exact).
//  - t: d FMA roundings on terms b_k |q_k| <= 255 |q_k|: |t - sum b_k q_k|
//    <= gamma(d) 255 |q|_1 <= 1.001 d u 255 |q|_1. qbias is an f64 sum
//    rounded once: within 1.001 u 128 |q|_1 of 128 sum q. w rounds once on
//    |t - qbias| <= 1.01 * 127 |q|_1. Together |w - C| <= e_w =
//    1.001 (d + 2) u 255 |q|_1, as for pf_i8_row, with |q|_1 the query's
//    own, not sqrt(d) |q|.
//  - a: xx and qq are each within 1.001 u of X and Q, the sum rounds once:
//    |a - (X + Q)| <= 2.01 u (X + Q).
//  - A2: -2 scale is exact, the FMA rounds z = a - 2 scale w once, and
//    |z| <= D^^2 + |z - D^^2|, D^^2 <= 2 (X + Q):
//    |A2 - D^^2| <= (1 + u) (2.01 u (X + Q) + 2 scale e_w) + 2 u (X + Q)
//               <= 4.011 u (X + Q) + 2.0021 (d + 2) u 255 |q|_1 scale.
//  - underflow: the d + 2 roundings behind w add at most 2^-150 each, times
//    2 scale (1 + u) < 2^25 (scale <= 2^30 / 127); xx, qq and A2 add 2^-150
//    each: below 2^-113 in all.
//  - the roots: delta carries 6.02 u (X + Q) more than the above, which is
//    >= 3.01 u D^^2. Then fl(A2 - delta) (1 + u)^2 <= D^^2 and
//    fl(A2 + delta) (1 - u)^2 >= D^^2, so the correctly rounded roots obey
//    sqrtf(fl(max(0, A2 - delta))) <= D^ <= sqrtf(fl(A2 + delta)). (A
//    root of a subnormal is normal: no absolute part.)
//  - delta itself: c1 = 2.01 (d + 2) u 255 |q|_1 rounded up (0.4 % above
//    2.0021), c2 = 10.5 u against the 10.031 u needed, relative to a >=
//    (X + Q) (1 - 2.01 u), C3 = 2^-112 against 2^-113: each slack exceeds
//    the two FMA roundings of delta (its value is >= C3, so normal).
//  - the exact chain: acc is a sum of d non-negative terms, each carrying
//    the roundings of one difference (twice) and one product, then at most
//    d - 1 additions: acc = D^2 (1 + theta), |theta| <= gamma(d + 2), plus
//    at most d 2^-150 <= 2^-138 for products that underflow (differences
//    and sums in the subnormal range are exact). The f64 root is correctly
//    rounded: exact is within D sqrt(1 -+ gamma(d + 2)) -+ 2^-69, times
//    1 -+ 2^-53. res carries PF_L2_RES_ABS = 2^-68 more than |x - x^|, so
//    with D <= D^ + |x - x^| and D >= D^ - |x - x^|:
//      exact <= (D^ + res) (1 + gamma / 2) (1 + 2^-53)
//      exact >= (D^ - res) (1 - 0.5001 gamma) (1 - 2^-53)   when D^ > res.
//  - the finish: the sum root + res and the product with ku round once each
//    (res >= 2^-68 keeps them normal), so up >= (D^ + res) ku (1 - u)^2, and
//    ku = 1 + gamma / 2 + 3 u rounded up covers it. The difference root -
//    res and the product with kl round once each, lo <= (D^ - res) kl
//    (1 + u)^2 + 2^-150, kl = 1 - (0.5001 gamma + 3 u) rounded down; the
//    2^-150 of a subnormal product is inside the 2^-69 that res has in
//    hand. A root at or below res gives lo = 0 <= exact.
// Nothing overflows: |t| <= 255 sqrt(d) 2^30 < 2^45, scale |w| < 2^69,
// xx, qq <= 2^61, up < 2^33.
__host__ __device__ static inline float pf_l2_finish(float t, float scale,
                                                     float xx, float res,
                                                     const PfL2Q &c, float *lo,
                                                     float *up) {
	const float w = t - c.qbias;
	const float a = xx + c.qq;
	const float A2 = fmaf(-2.0f * scale, w, a);
	const float delta = fmaf(scale, c.c1, fmaf(a, c.c2, PF_L2_C3));
	const float rl = sqrtf(fmaxf(A2 - delta, 0.f));
	const float ru = sqrtf(A2 + delta);
	*lo = fmaxf(rl - res, 0.f) * c.kl;
	*up = (ru + res) * c.ku;
	return A2;
}

// Build the euclidean int8 shadow: one lane per row, two passes, as
// k_shadow_i8 (pass one also sums the squares for the norm window: a
// euclidean table stages no norms).
__global__ void k_shadow_l2(const float *__restrict__ cm,
                            uint8_t *__restrict__ sh, float *__restrict__ scale,
                            float *__restrict__ xx, float *__restrict__ res,
                            uint64_t n, uint64_t n_pad, uint64_t sn_pad,
                            uint32_t d, uint64_t row0,
                            const uint32_t *__restrict__ blist) {
	const uint64_t r = (blist ? (uint64_t)blist[blockIdx.x] * 256
	                          : row0 + (uint64_t)blockIdx.x * blockDim.x) +
	                   threadIdx.x;
	if (r >= sn_pad)
		return;
	float sc = __uint_as_float(0x7FC00000u), x2 = 0.f, rs = 0.f;
	if (r < n) {
		pf_l2_row(cm + r, n_pad, d, sh + r, sn_pad, &sc, &x2, &rs);
	} else { // padding row: never covered
		for (uint32_t k = 0; k < d; k++)
			sh[(uint64_t)k * sn_pad + r] = 128;
	}
	scale[r] = sc;
	xx[r] = x2;
	res[r] = rs;
}

// k_prefilter over the int8 shadow: 16 rows per lane from one 16-byte load
// per feature, 8 loads in flight, one convert and one FMA per element.
// a_i = 1 - (t_i - qbias) * inv_q * pscale_i. The block top-K and the merge
// run on the UPPER bounds u_i = a_i + peps_i; scores[] receives the LOWER
// bounds l_i = a_i - peps_i (uncovered rows and non-finite scores -inf, kept
// out of the top-K, as in k_prefilter). k_pf_compact then passes every row
// with l_i <= U_K, the Kth smallest upper bound: the K covered rows with
// u_i <= U_K have exact distances <= U_K, so the exact Kth distance D_K <=
// U_K, and a true top-K row, ties included, has l_i <= d_i <= D_K <= U_K.
// The 4096-row tile feeds the select in two 2048-row halves through the
// same 17 KB buffer k_prefilter uses. MASKED as in k_prefilter: a lane's 16
// rows are 16 bits of one mask word, a wave's 1024 rows 16 words.
//
// L2 (the euclidean tier): the same stream over the same codes; only the
// side loads and the per-row finish differ. pscale holds the scales, peps
// the xx values with the res values sn_pad floats behind them, the query's
// PfL2Q stands behind the query at qg + d (inv_qnorm and qbias are not
// read), and [l_i, u_i] = pf_l2_finish's [lo, up].
template <bool MASKED, bool L2 = false>
__global__ __launch_bounds__(THREADS) void k_prefilter_i8(
    const uint8_t *__restrict__ sh, const float *__restrict__ pscale,
    const float *__restrict__ peps, uint64_t n, uint64_t sn_pad, uint32_t d,
    const float *__restrict__ qg, float inv_qnorm, float qbias, uint32_t k,
    uint64_t rows_per_block, float *__restrict__ scores,
    Cand *__restrict__ block_out, uint32_t *__restrict__ cand_cnt,
    const uint64_t *__restrict__ mask) {
	__shared__ uint64_t buf[PF_TILE + MAX_K];
	__shared__ uint64_t topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth;

	pf_topk_init(cnt, topk_n, kth, cand_cnt);

	uint64_t row_begin = (uint64_t)blockIdx.x * rows_per_block;
	uint64_t row_end = row_begin + rows_per_block;
	if (row_end > n)
		row_end = n;
	const float ninf = __uint_as_float(0xFF800000u);
	const float qnan = __uint_as_float(0x7FC00000u);

	for (uint64_t tile_base = row_begin; tile_base < row_end;
	     tile_base += PF8_TILE) {
		const uint64_t r0 =
		    tile_base + (uint64_t)threadIdx.x * PF8_ROWS_PER_LANE;
		const uint8_t *p = sh + r0;
		float acc[16];
#pragma unroll
		for (int c = 0; c < 16; c++)
			acc[c] = 0.f;
		uint32_t mb = 0xFFFFu; // the lane's 16 mask bits
		bool live = true;
		if constexpr (MASKED) {
			// r0 + 16 <= tile_base + PF8_TILE <= sn_pad
			mb = (uint32_t)(mask[r0 >> 6] >> (r0 & 63)) & 0xFFFFu;
			live = __ballot(mb != 0u) != 0ULL;
		}
#define PF8_ACC4(W, qk, o)                                                     \
	acc[o + 0] = __fmaf_rn((float)((W) & 0xFFu), qk, acc[o + 0]);              \
	acc[o + 1] = __fmaf_rn((float)(((W) >> 8) & 0xFFu), qk, acc[o + 1]);       \
	acc[o + 2] = __fmaf_rn((float)(((W) >> 16) & 0xFFu), qk, acc[o + 2]);      \
	acc[o + 3] = __fmaf_rn((float)((W) >> 24), qk, acc[o + 3]);
#define PF8_ACC(V, qk)                                                         \
	PF8_ACC4((V).x, qk, 0)                                                     \
	PF8_ACC4((V).y, qk, 4)                                                     \
	PF8_ACC4((V).z, qk, 8)                                                     \
	PF8_ACC4((V).w, qk, 12)
		if (live) {
			uint32_t kk = 0;
			for (; kk + 8 <= d; kk += 8) {
				uint4 w[8];
#pragma unroll
				for (uint32_t j = 0; j < 8; j++)
					w[j] = *(const uint4 *)(p + (uint64_t)(kk + j) * sn_pad);
#pragma unroll
				for (uint32_t j = 0; j < 8; j++) {
					const float qk = qg[kk + j]; // uniform: scalar load
					PF8_ACC(w[j], qk)
				}
			}
			for (; kk < d; kk++) {
				const uint4 w1 = *(const uint4 *)(p + (uint64_t)kk * sn_pad);
				const float qk = qg[kk];
				PF8_ACC(w1, qk)
			}
		}
#undef PF8_ACC
#undef PF8_ACC4
		float up[16];
		bool ok[16];
		PfL2Q qc = {};
		if constexpr (L2)
			qc = *(const PfL2Q *)(qg + d); // uniform: scalar loads
#pragma unroll
		for (int g = 0; g < 4; g++) {
			const float4 s4 = *(const float4 *)(pscale + r0 + 4 * g);
			const float4 e4 = *(const float4 *)(peps + r0 + 4 * g);
			const float ps[4] = {s4.x, s4.y, s4.z, s4.w};
			const float pe[4] = {e4.x, e4.y, e4.z, e4.w};
			float pr[4] = {0.f, 0.f, 0.f, 0.f};
			if constexpr (L2) {
				const float4 r4 =
				    *(const float4 *)(peps + sn_pad + r0 + 4 * g);
				pr[0] = r4.x, pr[1] = r4.y, pr[2] = r4.z, pr[3] = r4.w;
			}
			float lo[4];
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const int c = 4 * g + j;
				if constexpr (L2) {
					float lj, uj;
					const float a = pf_l2_finish(acc[c], ps[j], pe[j], pr[j],
					                             qc, &lj, &uj);
					ok[c] = (r0 + c) < row_end &&
					        (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
					up[c] = ok[c] ? uj : ninf;
					lo[j] = ok[c] ? lj : ninf;
				} else {
					const float a =
					    1.0f - (acc[c] - qbias) * inv_qnorm * ps[j];
					ok[c] = (r0 + c) < row_end &&
					        (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
					up[c] = ok[c] ? a + pe[j] : ninf;
					lo[j] = ok[c] ? a - pe[j] : ninf;
				}
				if constexpr (MASKED) {
					const bool allowed = (mb >> c) & 1u;
					ok[c] = ok[c] && allowed;
					lo[j] = allowed ? lo[j] : qnan;
				}
			}
			*(float4 *)(scores + r0 + 4 * g) =
			    make_float4(lo[0], lo[1], lo[2], lo[3]);
		}

		// threshold check + candidate append, one 2048-row half at a time
#pragma unroll
		for (int h = 0; h < 2; h++) {
			const uint64_t kthv = kth;
			const int full = (topk_n >= (int)k);
#pragma unroll
			for (int c8 = 0; c8 < 8; c8++) {
				const int c = 8 * h + c8;
				if (!ok[c])
					continue;
				uint64_t v =
				    ((uint64_t)d_key32(up[c]) << 32) | (uint32_t)(r0 + c);
				if (!full || v < kthv) {
					int idx = atomicAdd(&cnt, 1);
					buf[idx] = v;
				}
			}
			pf_topk_fold(buf, topk, cnt, topk_n, kth, k);
		}
	}

	pf_topk_write(topk, topk_n, k, block_out);
}

// ---------------------------------------------------------------------------
// Int6 tier of the prefilter: 0.75 of the int8 tier's bytes. Row r is stored
// as symmetric codes c_k in [-31, 31] with one f32 scale_r = maxabs_r / 31,
// as bias-32 codes xu_k = c_k + 32 in [1, 63], split into a high nibble
// xu >> 2 and a low pair xu & 3. The query is quantised on the host to
// cq_k in [-2047, 2047], bias 2048, three nibbles per element. The dot
// product runs in integers on v_dot8_u32_u4 (8 four-bit pairs per
// instruction) and is exact; the biases come off once per row.
//
// Layout, lane = row: features in groups of 32, G = ceil(d / 32). Plane H is
// [G][sn_pad rows][4 dwords]: dword m holds the high nibbles of features
// 32 g + 8 m + i in nibble i. Plane L is [G][sn_pad rows][2 dwords]: dword j
// holds the low pairs of features 32 g + 16 j + f, f < 8 in 2-bit field 2 f
// and f >= 8 in field 2 (f - 8) + 1, so that (w & 0x33333333) and
// ((w >> 2) & 0x33333333) are the nibble words of features 8 (2 j) + i and
// 8 (2 j + 1) + i: the same feature order as the H dwords, so one set of
// query digit words serves both planes. Features past d hold xu = 32.
// ---------------------------------------------------------------------------
#define PF6_SWEEPS 8
#define PF6_TILE (THREADS * PF6_SWEEPS) /* 2048 rows per select feed */
#define PF6_QWORDS 12 /* query digit dwords per group: [3 digits][4 dwords] */
#define PF6_UNROLL 6  /* groups in flight per lane: 9 KiB per wave */
#ifndef PF4_UNROLL
#define PF4_UNROLL 8 /* the H-only stream: 8 KiB per wave */
#endif
typedef uint32_t pf6_v4 __attribute__((ext_vector_type(4)));
typedef uint32_t pf6_v2 __attribute__((ext_vector_type(2)));

// Quantise one row for the int6 shadow (elements x[k * xstride], k < d;
// norm = the row's staged f64 norm) and derive its bound. The one routine
// behind both k_shadow_i6 and sdbv_prefilter_i6_row. Writes group g's four H
// dwords to h[g * hstride + 0..3] and its two L dwords to
// l[g * lstride + 0..1], *scale, *pscale = f32(scale / norm), *eps and
// *xsum = sum of the stored codes over the padded row. A row the bound
// cannot cover (as for pf_i8_row) gets neutral codes (xu = 32), scale =
// pscale = NaN and eps = 0: the prefilter always rescores it.
//
// Bound on |exact - approx| for a covered row and a query inside the norm
// window, exact = the restated f32 chain with its f64 finish (k_scan<0, .>),
// approx = 1 - f32(N) * pscale * qscale in f32 (k_prefilter_i6), where
// N = sum c_k cq_k as an exact integer, qscale = f32(sq / |q|) and sq the
// query's scale. In cosine units, i.e. divided by |x||q|, with u = 2^-24,
// x^ = scale c and q^ = sq cq:
//  - quantisation: x.q - x^.q^ = (x - x^).q + x^.(q - q^). By
//    Cauchy-Schwarz the first term is <= rho_x |x||q| with rho_x =
//    |x - x^| / |x|, the row's ACTUAL residual, computed here in f64 and
//    rounded up as in pf_i8_row; the second is <= |x^| |q - q^| <=
//    (1 + rho_x) |x| rho_q |q| with rho_q = |q - q^| / |q| the query's
//    actual residual (pf_q12). Together rho_x + (1 + rho_x) rho_q.
//  - exact chain: within 1.001 (d + 8) u of its exact sum, as for pf_eps.
//  - approx chain: the integer sum adds nothing: every partial result of
//    the digit sums and of the bias removal is below 2^32 at MAX_D
//    (sum xu qu <= 63 * 4095 * 4096 < 2^31) and |N| <= 31 * 2047 * 4096
//    < 2^28 fits int32.
//  - norms: rho_x, rho_q and both chains are taken against the same computed
//    norms, within (d + 8) u of the true ones: the factor 1.01 covers it, as
//    for pf_eps.
//  - finish: each element is within scale / 2 of its product, so rho_x <=
//    sqrt(d) / 62 <= 1.04 and rho_q <= sqrt(d) / 4094 <= 0.016 at MAX_D:
//    |approx cosine| <= (1 + rho_x)(1 + rho_q) <= 2.1. The int -> f32
//    conversion of N, pscale, qscale and the two f32 products round 5 times
//    (<= 10.6 u), the subtraction from 1 rounds a value below 3.1
//    (<= 3.1 u). The kernel's e = peps + (1 + peps) qeps, qeps = 1.01 rho_q
//    rounded up, uses peps >= rho_x for the row's residual and rounds three
//    times on values below 2.2, 0.04 and 1.2 (<= 3.5 u), and a + e / a - e
//    round once more on a value below 4.4 (<= 4.4 u): < 22 u < 2^-19; f64
//    steps and the underflow terms of the exact chain bounded at
//    PF_NORM_MIN are far below the remaining 10 u. Nothing in the approx
//    chain can underflow: pscale >= 1 / (31 sqrt(d)), qscale >=
//    1 / (2047 sqrt(d)).
// eps = 1.01 (rho_x + 1.001 (d + 8) u) + 2^-19, evaluated in f64 and rounded
// UP to f32; the query term (1 + eps) qeps is added by the kernel.
//
// Plane H on its own (the two-stage path, k_prefilter_i6<false, true>): with
// h_k = xu_k >> 2 the approximant of x_k is x^4_k = scale (4 h_k + 1.5 - 32)
// = scale (8 h_k - 61) / 2; the centre 1.5 of the dropped pair halves the
// truncation residual. N4 = sum (8 h_k - 61) cq_k is an exact integer,
// computed as 8 sum h_k qu_k - 8 * 2048 xsum_h - 61 sum cq_k with xsum_h =
// sum h_k over the padded row (padding features hold h = 8 against cq = 0 and
// add nothing to N4) and the last term a per-query constant;
// approx = 1 - f32(N4) * (pscale / 2) * qscale. Ranges: sum h qu <=
// 15 * 4095 * 4096 < 2^28; 8 h - 61 lies in [-61, 59], so |N4| <=
// 61 * 2047 * 4096 < 2^30 fits int32 and every partial result taken mod 2^32
// is harmless; pscale / 2 is exact in f32 (pscale >= 1 / (31 sqrt(d)), far
// from the subnormals). The proof above carries over with x^4 for x^ and
// rho4 = |x - x^4| / |x|, the row's actual residual, for rho_x; only the
// finish differs, since an element is within 2 scale of its approximant and
// rho4 can reach 2 sqrt(d) / 31 = 4.2 at MAX_D. While rho4 <= 1.04 every
// rounded value is below the one the count above used and the 2^-19 holds as
// it stands. Beyond, every rounded value is below 6 (1 + rho4) <= 32 and the
// 14 roundings add up to less than 450 u < 2.7e-5, while the factor 1.01
// needs 1.0005 for the norms and leaves 0.0095 rho4 > 9.8e-3 unused.
// eps4 = 1.01 (rho4 + 1.001 (d + 8) u) + 2^-19, rounded UP to f32; an
// uncovered row gets eps4 = 0 and xsum_h = 8 d_pad with its neutral codes.
// eps4 and xsum_h may be null together: then neither is computed.
__host__ __device__ static inline void pf_i6_row(
    const float *x, uint64_t xstride, uint32_t d, double norm, uint32_t *h,
    uint64_t hstride, uint32_t *l, uint64_t lstride, float *scale,
    float *pscale, float *eps, uint32_t *xsum, float *eps4 = nullptr,
    uint32_t *xsum_h = nullptr) {
	const uint32_t G = (d + 31) / 32;
	float m = 0.f;
	bool bad = false;
	for (uint32_t k = 0; k < d; k++) {
		const float v = x[(uint64_t)k * xstride];
		if ((__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u)
			bad = true;
		m = fmaxf(m, fabsf(v));
	}
	const bool covered =
	    !bad && norm >= PF_NORM_MIN && norm <= PF_NORM_MAX && m > 0.f;
	const float sc = covered ? (float)((double)m / 31.0)
	                         : __builtin_bit_cast(float, 0x7FC00000u);
	const double sd = (double)sc;
	double res2 = 0.0, res4 = 0.0;
	uint32_t xs = 0, xsh = 0;
	for (uint32_t g = 0; g < G; g++) {
		uint32_t hw[4] = {0, 0, 0, 0}, lw[2] = {0, 0};
#pragma unroll
		for (uint32_t i = 0; i < 32; i++) {
			const uint32_t k = 32 * g + i;
			uint32_t xu = 32;
			if (covered && k < d) {
				const double xv = (double)x[(uint64_t)k * xstride];
				double c = rint(xv / sd);
				c = c > 31.0 ? 31.0 : (c < -31.0 ? -31.0 : c);
				const double r = xv - sd * c;
				res2 += r * r;
				xu = (uint32_t)((int)c + 32);
				if (eps4) {
					const double r4 =
					    xv - sd * ((double)(4 * (xu >> 2)) + 1.5 - 32.0);
					res4 += r4 * r4;
				}
			}
			xs += xu;
			xsh += xu >> 2;
			hw[i >> 3] |= (xu >> 2) << (4 * (i & 7));
			const uint32_t f = i & 15;
			lw[i >> 4] |= (xu & 3u) << (2 * (f < 8 ? 2 * f : 2 * (f - 8) + 1));
		}
		for (int j = 0; j < 4; j++)
			h[(uint64_t)g * hstride + j] = hw[j];
		for (int j = 0; j < 2; j++)
			l[(uint64_t)g * lstride + j] = lw[j];
	}
	*xsum = xs;
	*scale = sc;
	if (eps4) {
		*xsum_h = xsh;
		*eps4 = 0.f;
	}
	if (!covered) {
		*pscale = sc;
		*eps = 0.f;
		return;
	}
	const double rho = sqrt(res2) / norm * (1.0 + 0x1p-40);
	const double e =
	    1.01 * (rho + 1.001 * (double)(d + 8) * 0x1p-24) + 0x1p-19;
	*pscale = (float)(sd / norm);
	*eps = pf_round_up_f32(e);
	if (eps4) {
		const double rho4 = sqrt(res4) / norm * (1.0 + 0x1p-40);
		*eps4 = pf_round_up_f32(
		    1.01 * (rho4 + 1.001 * (double)(d + 8) * 0x1p-24) + 0x1p-19);
	}
}

// Quantise a query for the int6 tier (host, once per call; q finite with a
// norm q_norm inside the window, so maxabs > 0): sq = f32(maxabs / 2047),
// cq_k = rint(q_k / sq) clamped to +-2047, qu_k = cq_k + 2048, padded
// features qu = 2048. words (if not null) receives the digit dwords in the
// order the planes need: words[g * 12 + t * 4 + m] holds digit t (0 = bits
// 11..8, 1 = bits 7..4, 2 = bits 3..0) of features 32 g + 8 m + i in nibble
// i. *rho = |q - sq cq| / q_norm in f64, rounded up to f32; *qs = sum qu_k
// over the padded query.
static void pf_q12(const float *q, uint32_t d, double q_norm, uint32_t *words,
                   int16_t *codes, float *sq, float *rho, uint32_t *qs) {
	const uint32_t G = (d + 31) / 32;
	float m = 0.f;
	for (uint32_t k = 0; k < d; k++)
		m = fmaxf(m, fabsf(q[k]));
	const float s = (float)((double)m / 2047.0);
	const double sd = (double)s;
	double res2 = 0.0;
	uint32_t sum = 0;
	for (uint32_t g = 0; g < G; g++) {
		uint32_t w[PF6_QWORDS] = {0};
		for (uint32_t i = 0; i < 32; i++) {
			const uint32_t k = 32 * g + i;
			uint32_t qu = 2048;
			if (k < d) {
				const double qv = (double)q[k];
				double c = rint(qv / sd);
				c = c > 2047.0 ? 2047.0 : (c < -2047.0 ? -2047.0 : c);
				const double r = qv - sd * c;
				res2 += r * r;
				qu = (uint32_t)((int)c + 2048);
				if (codes)
					codes[k] = (int16_t)c;
			}
			sum += qu;
			const uint32_t sh = 4 * (i & 7), mw = i >> 3;
			w[0 + mw] |= (qu >> 8) << sh;
			w[4 + mw] |= ((qu >> 4) & 15u) << sh;
			w[8 + mw] |= (qu & 15u) << sh;
		}
		if (words)
			std::memcpy(words + (uint64_t)g * PF6_QWORDS, w, sizeof(w));
	}
	*sq = s;
	*qs = sum;
	const double r = sqrt(res2) / q_norm * (1.0 + 0x1p-40);
	*rho = r > 0.0 ? pf_round_up_f32(r) : 0.f;
}

// Build the int6 shadow: one lane per row, as k_shadow_i8. peps4 and xsum_h
// are null for a shadow without the H-only side data.
__global__ void k_shadow_i6(const float *__restrict__ cm,
                            const double *__restrict__ norms,
                            uint32_t *__restrict__ hp,
                            uint32_t *__restrict__ lp,
                            float *__restrict__ pscale,
                            float *__restrict__ peps,
                            uint32_t *__restrict__ xsum,
                            float *__restrict__ peps4,
                            uint32_t *__restrict__ xsum_h, uint64_t n,
                            uint64_t n_pad, uint64_t sn_pad, uint32_t d,
                            uint64_t row0,
                            const uint32_t *__restrict__ blist) {
	const uint64_t r = (blist ? (uint64_t)blist[blockIdx.x] * 256
	                          : row0 + (uint64_t)blockIdx.x * blockDim.x) +
	                   threadIdx.x;
	if (r >= sn_pad)
		return;
	const uint32_t G = (d + 31) / 32;
	float sc, ps = __uint_as_float(0x7FC00000u), pe = 0.f, pe4 = 0.f;
	uint32_t xs = 32u * 32u * G, xsh = 8u * 32u * G;
	if (r < n) {
		pf_i6_row(cm + r, n_pad, d, norms[r], hp + r * 4, sn_pad * 4,
		          lp + r * 2, sn_pad * 2, &sc, &ps, &pe, &xs,
		          peps4 ? &pe4 : nullptr, &xsh);
	} else { // padding row: never covered
		for (uint32_t g = 0; g < G; g++) {
			*(uint4 *)(hp + ((uint64_t)g * sn_pad + r) * 4) = make_uint4(
			    0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u);
			*(uint2 *)(lp + ((uint64_t)g * sn_pad + r) * 2) = make_uint2(0, 0);
		}
	}
	pscale[r] = ps;
	peps[r] = pe;
	xsum[r] = xs;
	if (peps4) { // the H-only side data (Shadow::h4)
		peps4[r] = pe4;
		xsum_h[r] = xsh;
	}
}

// k_prefilter over the int6 shadow: one row per lane and sweep, one 16-byte
// H load and one 8-byte L load per group of 32 features (a wave reads 1 KiB
// + 512 B contiguous), PF6_UNROLL groups in flight, loaded non-temporal (the
// shadow is read once per query; worth 0.02-0.05 ms of 1.03 at 10M x 768,
// profiles/prefilter_i6.md). Six exact u32
// accumulators: H and L against the query's three digits (qd, uniform:
// scalar loads, used as the dots' scalar operand). Per row
// S = 4 (256 A_h2 + 16 A_h1 + A_h0) + 256 A_l2 + 16 A_l1 + A_l0 = sum xu qu
// and N = sum c cq = S - 2048 xsum + qbias, qbias = 65536 d_pad - 32 sum qu
// (mod 2^32; N fits int32). a = 1 - f32(N) * pscale * qscale, bounds
// a +- e with e = peps + (1 + peps) qeps (proof above pf_i6_row). Upper
// bounds go to the block top-K, lower bounds to scores[], exactly as in
// k_prefilter_i8. A block collects the rows of PF6_SWEEPS sweeps that beat
// its current Kth upper bound, then runs one select: the same 17 KB buffer.
// MASKED as in k_prefilter: lane = row, so a wave's 64 rows of one sweep are
// exactly one mask word, and the skip is per wave and sweep.
//
// H4 (the two-stage path's stream, unmasked only): plane H alone, one
// non-temporal 16-byte load per group and lane, PF4_UNROLL groups in flight,
// three accumulators. lp is never read (nullptr); peps is the shadow's peps4,
// xsum its xsum_h and qbias = -61 sum cq (mod 2^32). N4 = 8 (256 A_h2 +
// 16 A_h1 + A_h0) - 8 * 2048 xsum_h + qbias and a = 1 - f32(N4) *
// (pscale / 2) * qscale (ranges and bound above pf_i6_row). Block 0 also
// clears the first list's counter, cand_cnt[1], for k_pf4_compact.
#define PF6_DOT3(X, m, a2, a1, a0)                                             \
	a2 = __builtin_amdgcn_udot8((X), qw[0 + (m)], a2, false);                  \
	a1 = __builtin_amdgcn_udot8((X), qw[4 + (m)], a1, false);                  \
	a0 = __builtin_amdgcn_udot8((X), qw[8 + (m)], a0, false);
#define PF6_GROUP_H(HV, gi)                                                    \
	{                                                                          \
		const uint32_t *qw = qd + (uint64_t)(gi) * PF6_QWORDS;                 \
		PF6_DOT3((HV).x, 0, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).y, 1, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).z, 2, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).w, 3, ah2, ah1, ah0)                                     \
	}
#define PF6_GROUP(HV, LV, gi)                                                  \
	{                                                                          \
		const uint32_t *qw = qd + (uint64_t)(gi) * PF6_QWORDS;                 \
		PF6_DOT3((HV).x, 0, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).y, 1, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).z, 2, ah2, ah1, ah0)                                     \
		PF6_DOT3((HV).w, 3, ah2, ah1, ah0)                                     \
		PF6_DOT3((LV).x & 0x33333333u, 0, al2, al1, al0)                       \
		PF6_DOT3(((LV).x >> 2) & 0x33333333u, 1, al2, al1, al0)                \
		PF6_DOT3((LV).y & 0x33333333u, 2, al2, al1, al0)                       \
		PF6_DOT3(((LV).y >> 2) & 0x33333333u, 3, al2, al1, al0)                \
	}

// The int6 tier's finish, shared by the stream and by k_pf4_refine: N from
// the six digit sums, then a and e.
#define PF6_N(xs, qb)                                                          \
	((int32_t)(4u * (256u * ah2 + 16u * ah1 + ah0) + 256u * al2 + 16u * al1 +  \
	           al0 - 2048u * (xs) + (qb)))
#define PF6_A(N, ps, qscale)                                                   \
	__fsub_rn(1.0f, __fmul_rn(__fmul_rn((float)(N), (ps)), (qscale)))
#define PF6_E(pe, qeps)                                                        \
	__fadd_rn((pe), __fmul_rn(__fadd_rn(1.0f, (pe)), (qeps)))

template <bool MASKED, bool H4 = false>
__global__ __launch_bounds__(THREADS) void k_prefilter_i6(
    const uint4 *__restrict__ hp, const uint2 *__restrict__ lp,
    const float *__restrict__ pscale, const float *__restrict__ peps,
    const uint32_t *__restrict__ xsum, uint64_t n, uint64_t sn_pad,
    uint32_t ngroups, const uint32_t *__restrict__ qd, float qscale,
    float qeps, uint32_t qbias, uint32_t k, uint64_t rows_per_block,
    float *__restrict__ scores, Cand *__restrict__ block_out,
    uint32_t *__restrict__ cand_cnt, const uint64_t *__restrict__ mask) {
	__shared__ uint64_t buf[PF_TILE + MAX_K];
	__shared__ uint64_t topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth;

	static_assert(!(MASKED && H4), "the H-only stream has no masked variant");
	pf_topk_init(cnt, topk_n, kth, cand_cnt);
	if constexpr (H4)
		if (blockIdx.x == 0 && threadIdx.x == 0)
			cand_cnt[1] = 0;

	uint64_t row_begin = (uint64_t)blockIdx.x * rows_per_block;
	uint64_t row_end = row_begin + rows_per_block;
	if (row_end > n)
		row_end = n;
	const float ninf = __uint_as_float(0xFF800000u);

	for (uint64_t tile_base = row_begin; tile_base < row_end;
	     tile_base += PF6_TILE) {
		const uint64_t kthv = kth;
		const int full = (topk_n >= (int)k);
		for (int s = 0; s < PF6_SWEEPS; s++) {
			const uint64_t sbase = tile_base + (uint64_t)s * THREADS;
			if (sbase >= row_end)
				break; // uniform
			const uint64_t r = sbase + threadIdx.x; // < sn_pad
			const uint4 *ph = hp + r;
			const uint2 *pl = lp + r;
			uint32_t ah2 = 0, ah1 = 0, ah0 = 0, al2 = 0, al1 = 0, al0 = 0;
			bool allowed = true, live = true;
			if constexpr (MASKED) {
				// sbase is a multiple of 256: r >> 6 is the wave's own word
				const uint64_t mw = mask[r >> 6];
				allowed = (mw >> (r & 63)) & 1ULL;
				live = __ballot(mw != 0ULL) != 0ULL;
			}
			if constexpr (H4) {
				uint32_t g = 0;
				for (; g + PF4_UNROLL <= ngroups; g += PF4_UNROLL) {
					pf6_v4 hv[PF4_UNROLL];
#pragma unroll
					for (uint32_t j = 0; j < PF4_UNROLL; j++)
						hv[j] = __builtin_nontemporal_load(
						    (const pf6_v4 *)(ph + (uint64_t)(g + j) * sn_pad));
#pragma unroll
					for (uint32_t j = 0; j < PF4_UNROLL; j++)
						PF6_GROUP_H(hv[j], g + j)
				}
				for (; g < ngroups; g++) {
					const uint4 hv1 = ph[(uint64_t)g * sn_pad];
					PF6_GROUP_H(hv1, g)
				}
			} else if (live) {
				uint32_t g = 0;
				for (; g + PF6_UNROLL <= ngroups; g += PF6_UNROLL) {
					pf6_v4 hv[PF6_UNROLL];
					pf6_v2 lv[PF6_UNROLL];
#pragma unroll
					for (uint32_t j = 0; j < PF6_UNROLL; j++) {
						hv[j] = __builtin_nontemporal_load(
						    (const pf6_v4 *)(ph + (uint64_t)(g + j) * sn_pad));
						lv[j] = __builtin_nontemporal_load(
						    (const pf6_v2 *)(pl + (uint64_t)(g + j) * sn_pad));
					}
#pragma unroll
					for (uint32_t j = 0; j < PF6_UNROLL; j++)
						PF6_GROUP(hv[j], lv[j], g + j)
				}
				for (; g < ngroups; g++) {
					const uint4 hv1 = ph[(uint64_t)g * sn_pad];
					const uint2 lv1 = pl[(uint64_t)g * sn_pad];
					PF6_GROUP(hv1, lv1, g)
				}
			}
			const int32_t N =
			    H4 ? (int32_t)(8u * (256u * ah2 + 16u * ah1 + ah0) -
			                   16384u * xsum[r] + qbias)
			       : PF6_N(xsum[r], qbias);
			const float pe = peps[r];
			const float a = PF6_A(
			    N, H4 ? __fmul_rn(pscale[r], 0.5f) : pscale[r], qscale);
			const float e = PF6_E(pe, qeps);
			const bool ok = allowed && r < row_end &&
			                (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
			if constexpr (MASKED)
				scores[r] = ok        ? __fsub_rn(a, e)
				            : allowed ? ninf
				                      : __uint_as_float(0x7FC00000u);
			else
				scores[r] = ok ? __fsub_rn(a, e) : ninf;
			if (ok) {
				const uint64_t v =
				    ((uint64_t)d_key32(__fadd_rn(a, e)) << 32) | (uint32_t)r;
				if (!full || v < kthv) {
					int idx = atomicAdd(&cnt, 1);
					buf[idx] = v;
				}
			}
		}
		pf_topk_fold(buf, topk, cnt, topk_n, kth, k);
	}

	pf_topk_write(topk, topk_n, k, block_out);
}

// One pass over scores[]: append every row with score <= T_K + 2 eps to the
// candidate list. bf16 tier: scores are a_i, approx_top[k-1].dist is A_K and
// eps = pf_eps(d). int8 and int6 tiers: scores are the lower bounds l_i,
// approx_top[k-1].dist is U_K and eps = 0. T_K is +inf when fewer than K
// rows carry a bound: then every row passes. The counter keeps counting past
// PF_CAND_CAP; the list is never written past it.
__global__ void k_pf_compact(const float *__restrict__ scores, uint64_t n,
                             const Cand *__restrict__ approx_top, uint32_t k,
                             float eps, uint32_t *__restrict__ cand_cnt,
                             uint32_t *__restrict__ cand_rows) {
	const double thr = approx_top[k - 1].dist + 2.0 * (double)eps;
	const uint64_t ngrp = (n + 3) / 4;
	for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	     g < ngrp; g += (uint64_t)gridDim.x * blockDim.x) {
		const float4 s = *(const float4 *)(scores + g * 4);
		const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
		for (int c = 0; c < 4; c++) {
			uint64_t r = g * 4 + c;
			if (r < n && (double)v[c] <= thr) {
				uint32_t idx = atomicAdd(cand_cnt, 1u);
				if (idx < PF_CAND_CAP)
					cand_rows[idx] = (uint32_t)r;
			}
		}
	}
}

// The exact chain on listed rows, one 64-lane workgroup per row (grid-stride
// over cnt rows), out[c] = Cand{dist, ids[rows[c]]}: the body of k_pf_rescore
// and k_rows_exact. All lanes fetch the row's d strided f32 elements into
// LDS. Cosine then runs the op sequence of k_scan<0, .> / k_gather_dist<0>: 8
// partial sums, the same combine, the same tail, the f64 finish with
// norms[r]. Euclidean runs the sequential chain of k_scan<1, .> /
// k_gather_dist<1> on lane 0. qs, xs ([MAX_D]) and ps ([8]) are the calling
// kernel's LDS. rows_exact_one is one row of it, *out = Cand{dist, ids[r]},
// with the query already in qs (the barrier it opens with orders that).
template <int METRIC>
__device__ __forceinline__ static void rows_exact_one(
    const float *__restrict__ cm, const double *__restrict__ norms,
    const uint64_t *__restrict__ ids, uint64_t n_pad, uint32_t d,
    double q_norm, uint32_t r, Cand *__restrict__ out, float *qs, float *xs,
    float *ps) {
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < d; i += 64)
		xs[i] = cm[(uint64_t)i * n_pad + r];
	__syncthreads();
	if (METRIC == 0) {
		// the chain's 8 partial sums are independent of each other: lane
		// j runs partial j's own sequence, lane 0 then combines them in
		// the chain's order — the same operations on the same values
		const uint32_t d8 = d & ~7u;
		if (threadIdx.x < 8) {
			float pj = 0.f;
			for (uint32_t i = threadIdx.x; i < d8; i += 8)
				pj = __fadd_rn(pj, __fmul_rn(xs[i], qs[i]));
			ps[threadIdx.x] = pj;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			float p[8];
#pragma unroll
			for (int j = 0; j < 8; j++)
				p[j] = ps[j];
			uint32_t k8 = d8;
			float sum = 0.f;
			sum = __fadd_rn(sum, __fadd_rn(p[0], p[4]));
			sum = __fadd_rn(sum, __fadd_rn(p[1], p[5]));
			sum = __fadd_rn(sum, __fadd_rn(p[2], p[6]));
			sum = __fadd_rn(sum, __fadd_rn(p[3], p[7]));
			for (; k8 < d; k8++)
				sum = __fadd_rn(sum, __fmul_rn(xs[k8], qs[k8]));
			double den = q_norm * norms[r];
			Cand o;
			o.dist = 1.0 - (double)sum / den;
			o.id = ids[r];
			*out = o;
		}
	} else {
		if (threadIdx.x == 0) {
			float acc = 0.f;
			for (uint32_t kk = 0; kk < d; kk++) {
				float diff = xs[kk] - qs[kk];
				acc = __fadd_rn(acc, __fmul_rn(diff, diff));
			}
			Cand o;
			o.dist = sqrt((double)acc);
			o.id = ids[r];
			*out = o;
		}
	}
}

template <int METRIC>
__device__ __forceinline__ static void rows_exact(
    const float *__restrict__ cm, const double *__restrict__ norms,
    const uint64_t *__restrict__ ids, uint64_t n_pad, uint32_t d,
    const float *__restrict__ qg, double q_norm,
    const uint32_t *__restrict__ rows, uint32_t cnt, Cand *__restrict__ out,
    float *qs, float *xs, float *ps) {
	for (uint32_t i = threadIdx.x; i < d; i += 64)
		qs[i] = qg[i];
	for (uint32_t c = blockIdx.x; c < cnt; c += gridDim.x)
		rows_exact_one<METRIC>(cm, norms, ids, n_pad, d, q_norm, rows[c],
		                       out + c, qs, xs, ps);
}

// Exact rescore of the prefilter's candidates: rows_exact<METRIC> over the
// count k_pf_compact left on the device.
template <int METRIC>
__global__ __launch_bounds__(64) void k_pf_rescore(
    const float *__restrict__ cm, const double *__restrict__ norms,
    const uint64_t *__restrict__ ids, uint64_t n_pad, uint32_t d,
    const float *__restrict__ qg, double q_norm,
    const uint32_t *__restrict__ cand_cnt,
    const uint32_t *__restrict__ cand_rows, Cand *__restrict__ out) {
	__shared__ float qs[MAX_D];
	__shared__ float xs[MAX_D];
	__shared__ float ps[8];
	const uint32_t cnt = *cand_cnt;
	if (cnt > PF_CAND_CAP || blockIdx.x >= cnt)
		return; // overflow: the host reruns the exact scan
	rows_exact<METRIC>(cm, norms, ids, n_pad, d, qg, q_norm, cand_rows, cnt,
	                   out, qs, xs, ps);
}

// Row-list path of the filtered call: rows_exact on the
// cnt <= PF_CAND_CAP allowed rows the host listed. A single-block k_merge
// over out[0..cnt) selects the top-k.
template <int METRIC>
__global__ __launch_bounds__(64) void k_rows_exact(
    const float *__restrict__ cm, const double *__restrict__ norms,
    const uint64_t *__restrict__ ids, uint64_t n_pad, uint32_t d,
    const float *__restrict__ qg, double q_norm,
    const uint32_t *__restrict__ rows, uint32_t cnt, Cand *__restrict__ out) {
	__shared__ float qs[MAX_D];
	__shared__ float xs[MAX_D];
	__shared__ float ps[8];
	rows_exact<METRIC>(cm, norms, ids, n_pad, d, qg, q_norm, rows, cnt, out,
	                   qs, xs, ps);
}

// Final select over the rescored candidates: k_merge's (total_cmp dist, id)
// order with the candidate count read on the device. The raw count lands
// right behind the k results so one D2H copy carries both; an overflowed
// count selects nothing (the host reruns the exact scan).
__global__ __launch_bounds__(THREADS) void k_pf_final(
    Cand *__restrict__ cands, const uint32_t *__restrict__ cand_cnt,
    uint32_t k, Cand *__restrict__ out) {
	const uint32_t raw = *cand_cnt;
	const uint64_t total = raw > PF_CAND_CAP ? 0 : raw;
	if (threadIdx.x == 0) {
		out[k].dist = 0.0;
		out[k].id = raw;
	}
	merge_slice(cands, total, k, total, out);
}

// ---------------------------------------------------------------------------
// Two-stage int6 path: k_prefilter_i6<false, true> streams
// plane H alone; the kernels here turn its scores into the candidate list
// that k_pf_rescore and k_pf_final take as from k_pf_compact.
// ---------------------------------------------------------------------------
#define PF4_LIST_CAP 262144u /* first list: 1 MB of rows */
#define PF4_BLOCK_LIST 8192  /* rows a block collects before it reserves */
#define PF4_PASSES 4         /* score loads a lane has in flight */
#ifndef PF4_REFINE_LANES
#define PF4_REFINE_LANES 32 /* lanes that share one listed row */
#endif

// Exact distances of the K rows with the smallest H-only upper bounds
// (approx_top of launch_merge_tree: id = row position), one 64-lane
// workgroup each: out[c] = rows_exact<0> of row approx_top[c].id, or +inf
// for an entry without a row (fewer than K rows carry a bound). With
// fold_total > 0, approx_top is the merge tree's level 1 instead
// (fold_total <= 32 * MAX_K winners): every workgroup selects the K smallest
// of them itself, which is the tree's level 2 without its launch, and takes
// its own entry.
__global__ __launch_bounds__(64) void k_pf4_threshold(
    const float *__restrict__ cm, const double *__restrict__ norms,
    const uint64_t *__restrict__ ids, uint64_t n_pad, uint32_t d,
    const float *__restrict__ qg, double q_norm,
    const Cand *__restrict__ approx_top, uint32_t fold_total, uint32_t k,
    Cand *__restrict__ out) {
	__shared__ float qs[MAX_D];
	__shared__ float xs[MAX_D];
	__shared__ float ps[8];
	__shared__ SliceSel sel;
	__shared__ Cand top[MAX_K];
	uint64_t r;
	if (fold_total > 0) { // uniform
		block_select_slice<64, 16>(approx_top, fold_total, k, top, &sel);
		r = top[blockIdx.x].id;
	} else {
		r = approx_top[blockIdx.x].id;
	}
	if (r == ~0ULL) { // uniform
		if (threadIdx.x == 0) {
			Cand o;
			o.dist = __longlong_as_double(0x7FF0000000000000LL);
			o.id = ~0ULL;
			out[blockIdx.x] = o;
		}
		return;
	}
	for (uint32_t i = threadIdx.x; i < d; i += 64)
		qs[i] = qg[i];
	rows_exact_one<0>(cm, norms, ids, n_pad, d, q_norm, (uint32_t)r,
	                  out + blockIdx.x, qs, xs, ps);
}

// T = the largest of the k threshold distances in total_cmp order, for every
// thread of the block (k <= MAX_K <= blockDim.x; key is the caller's LDS).
// The exact distances of K distinct rows bound the true Kth distance from
// above, so a row whose lower bound exceeds T is in no top-K, ties included.
__device__ __forceinline__ static double pf4_threshold(
    const Cand *__restrict__ thr, uint32_t k, unsigned long long *key) {
	if (threadIdx.x == 0)
		*key = 0;
	__syncthreads();
	if (threadIdx.x < k)
		atomicMax(key, (unsigned long long)d_total_key(thr[threadIdx.x].dist));
	__syncthreads();
	const uint64_t kb = *key;
	return __longlong_as_double(
	    (long long)((kb >> 63) ? (kb & 0x7FFFFFFFFFFFFFFFULL) : ~kb));
}

// k_pf_compact against T, for a list of thousands of rows: a block collects
// the rows of its whole grid-stride loop in LDS and reserves list space with
// one global atomic per PF4_BLOCK_LIST rows at most (the list's order is
// arbitrary as before); a lane loads PF4_PASSES score quads before the block
// meets at a barrier, so the loads of a round overlap. A row passes unless
// its score is above T: -inf, the rows without a bound, always does. The
// counter keeps counting past list_cap <= PF4_LIST_CAP; the list is never
// written past it.
__global__ __launch_bounds__(THREADS) void k_pf4_compact(
    const float *__restrict__ scores, uint64_t n,
    const Cand *__restrict__ thr, uint32_t k, uint32_t list_cap,
    uint32_t *__restrict__ list_cnt, uint32_t *__restrict__ list_rows) {
	__shared__ uint32_t rows[PF4_BLOCK_LIST];
	__shared__ uint32_t cnt, base;
	__shared__ unsigned long long tkey;
	if (threadIdx.x == 0)
		cnt = 0;
	const double T = pf4_threshold(thr, k, &tkey);
	const uint64_t ngrp = (n + 3) / 4;
	const uint64_t round = (uint64_t)THREADS * PF4_PASSES;
	// g0 is uniform, so every thread of the block meets every barrier
	for (uint64_t g0 = (uint64_t)blockIdx.x * round;;
	     g0 += (uint64_t)gridDim.x * round) {
		const bool last = g0 >= ngrp;
		float4 s[PF4_PASSES];
#pragma unroll
		for (int p = 0; p < PF4_PASSES; p++) {
			const uint64_t g = g0 + (uint64_t)p * THREADS + threadIdx.x;
			if (g < ngrp)
				s[p] = *(const float4 *)(scores + g * 4);
		}
#pragma unroll
		for (int p = 0; p < PF4_PASSES; p++) {
			const uint64_t g = g0 + (uint64_t)p * THREADS + threadIdx.x;
			if (g >= ngrp)
				continue;
			const float v[4] = {s[p].x, s[p].y, s[p].z, s[p].w};
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const uint64_t r = g * 4 + c;
				if (r < n && !((double)v[c] > T))
					rows[atomicAdd(&cnt, 1u)] = (uint32_t)r;
			}
		}
		__syncthreads();
		const uint32_t m = cnt;
		__syncthreads();
		// one round adds at most 4 * round rows: flush while that still fits
		if (m > PF4_BLOCK_LIST - 4 * THREADS * PF4_PASSES || (last && m > 0)) {
			if (threadIdx.x == 0) {
				base = atomicAdd(list_cnt, m);
				cnt = 0;
			}
			__syncthreads();
			for (uint32_t i = threadIdx.x; i < m; i += THREADS)
				if (base + i < list_cap)
					list_rows[base + i] = rows[i];
			__syncthreads();
		}
		if (last)
			break;
	}
}

// The second test: PF4_REFINE_LANES lanes gather one listed row's H and L
// words, group by group, and add up the six digit sums (exact integers, any
// order); the row goes on to cand_rows (cap PF_CAND_CAP, as k_pf_compact
// fills it) unless its int6 lower bound, k_prefilter_i6's own a - e, is
// above T, and always if it carries no bound. An overflowed first list is
// left alone: the host then runs the plain int6 path.
__global__ __launch_bounds__(THREADS) void k_pf4_refine(
    const uint4 *__restrict__ hp, const uint2 *__restrict__ lp,
    const float *__restrict__ pscale, const float *__restrict__ peps,
    const uint32_t *__restrict__ xsum, uint64_t sn_pad, uint32_t ngroups,
    const uint32_t *__restrict__ qd, float qscale, float qeps, uint32_t qbias,
    const Cand *__restrict__ thr, uint32_t k, uint32_t list_cap,
    const uint32_t *__restrict__ list_cnt,
    const uint32_t *__restrict__ list_rows, uint32_t *__restrict__ cand_cnt,
    uint32_t *__restrict__ cand_rows) {
	__shared__ unsigned long long tkey;
	const double T = pf4_threshold(thr, k, &tkey);
	const uint32_t m = *list_cnt;
	if (m > list_cap)
		return;
	const uint32_t sub = threadIdx.x % PF4_REFINE_LANES;
	const uint32_t per_grid = gridDim.x * (THREADS / PF4_REFINE_LANES);
	for (uint32_t c = (blockIdx.x * THREADS + threadIdx.x) / PF4_REFINE_LANES;
	     c < m; c += per_grid) { // uniform over the lanes of one row
		const uint32_t r = list_rows[c];
		uint32_t ah2 = 0, ah1 = 0, ah0 = 0, al2 = 0, al1 = 0, al0 = 0;
		for (uint32_t g = sub; g < ngroups; g += PF4_REFINE_LANES) {
			const uint4 hv = hp[(uint64_t)g * sn_pad + r];
			const uint2 lv = lp[(uint64_t)g * sn_pad + r];
			PF6_GROUP(hv, lv, g)
		}
#pragma unroll
		for (int off = PF4_REFINE_LANES / 2; off > 0; off >>= 1) {
			ah2 += __shfl_xor(ah2, off);
			ah1 += __shfl_xor(ah1, off);
			ah0 += __shfl_xor(ah0, off);
			al2 += __shfl_xor(al2, off);
			al1 += __shfl_xor(al1, off);
			al0 += __shfl_xor(al0, off);
		}
		if (sub == 0) {
			const int32_t N = PF6_N(xsum[r], qbias);
			const float pe = peps[r];
			const float a = PF6_A(N, pscale[r], qscale);
			const float e = PF6_E(pe, qeps);
			const bool covered =
			    (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u;
			if (!covered || !((double)__fsub_rn(a, e) > T)) {
				const uint32_t idx = atomicAdd(cand_cnt, 1u);
				if (idx < PF_CAND_CAP)
					cand_rows[idx] = r;
			}
		}
	}
}
#undef PF6_E
#undef PF6_A
#undef PF6_N
#undef PF6_GROUP
#undef PF6_GROUP_H
#undef PF6_DOT3

// All-distance kernel: one lane per row, feature-major coalesced reads.
// Used for parity dumps, k > MAX_K, and (as the product path proper) the
// six non-headline metrics — each restating the reference's F32 chain
// (vector.rs:206-451) operation-for-operation. `order` = minkowski order;
// `q_mean` = the query's ndarray-mean (pearson, host-precomputed with the
// same unrolled-8 chain).
template <int METRIC>
__global__ void k_all_dists(const float *__restrict__ cm,
                            const double *__restrict__ norms, uint64_t n,
                            uint64_t n_pad, uint32_t d,
                            const float *__restrict__ qg, double q_norm,
                            double order, double q_mean,
                            double *__restrict__ out) {
	uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n)
		return;
	if (METRIC == 0) {
		float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t k = 0;
		for (; k + 8 <= d; k += 8) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				float x = cm[(uint64_t)(k + j) * n_pad + r];
				p[j] = __fadd_rn(p[j], __fmul_rn(x, qg[k + j]));
			}
		}
		float sum = 0.f;
		sum = __fadd_rn(sum, __fadd_rn(p[0], p[4]));
		sum = __fadd_rn(sum, __fadd_rn(p[1], p[5]));
		sum = __fadd_rn(sum, __fadd_rn(p[2], p[6]));
		sum = __fadd_rn(sum, __fadd_rn(p[3], p[7]));
		for (; k < d; k++)
			sum = __fadd_rn(sum, __fmul_rn(cm[(uint64_t)k * n_pad + r], qg[k]));
		out[r] = 1.0 - (double)sum / (q_norm * norms[r]);
	} else if (METRIC == 1) {
		float acc = 0.f;
		for (uint32_t k = 0; k < d; k++) {
			float diff = cm[(uint64_t)k * n_pad + r] - qg[k];
			acc = __fadd_rn(acc, __fmul_rn(diff, diff));
		}
		out[r] = sqrt((double)acc);
	} else if (METRIC == 2) {
		// manhattan via l1_dist: sequential f32 |a-b| sum (vector.rs:379)
		float acc = 0.f;
		for (uint32_t k = 0; k < d; k++)
			acc = __fadd_rn(acc, fabsf(qg[k] - cm[(uint64_t)k * n_pad + r]));
		out[r] = (double)acc;
	} else if (METRIC == 3) {
		// chebyshev via linf_dist: f32 fmax chain (vector.rs:220-229)
		float m = 0.f;
		for (uint32_t k = 0; k < d; k++)
			m = fmaxf(m, fabsf(qg[k] - cm[(uint64_t)k * n_pad + r]));
		out[r] = (double)m;
	} else if (METRIC == 4) {
		// hamming: count of element-wise != (vector.rs:292-303)
		uint64_t acc = 0;
		for (uint32_t k = 0; k < d; k++)
			if (qg[k] != cm[(uint64_t)k * n_pad + r])
				acc++;
		out[r] = (double)acc;
	} else if (METRIC == 6) {
		// minkowski: f64 |diff|^order sequential sum, final ^(1/order)
		// (vector.rs:389-399)
		double acc = 0.0;
		for (uint32_t k = 0; k < d; k++)
			acc += pow(fabs((double)qg[k] -
			                (double)cm[(uint64_t)k * n_pad + r]),
			           order);
		out[r] = pow(acc, 1.0 / order);
	} else if (METRIC == 7) {
		// pearson similarity used directly as the metric value
		// (vector.rs:413-440): row mean via the unrolled-8 f32 chain
		// (ndarray .mean() = .sum()/len), then sequential f64 moments
		float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t k = 0;
		for (; k + 8 <= d; k += 8) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++)
				p[j] = __fadd_rn(p[j], cm[(uint64_t)(k + j) * n_pad + r]);
		}
		float sb = 0.f;
		sb = __fadd_rn(sb, __fadd_rn(__fadd_rn(p[0], p[4]),
		                             __fadd_rn(p[1], p[5])));
		sb = __fadd_rn(sb, __fadd_rn(__fadd_rn(p[2], p[6]),
		                             __fadd_rn(p[3], p[7])));
		for (; k < d; k++)
			sb = __fadd_rn(sb, cm[(uint64_t)k * n_pad + r]);
		double my = (double)(sb / (float)d);
		double sum_xy = 0, sum_x2 = 0, sum_y2 = 0;
		for (uint32_t i = 0; i < d; i++) {
			double dx = (double)qg[i] - q_mean;
			double dy = (double)cm[(uint64_t)i * n_pad + r] - my;
			sum_xy += dx * dy;
			sum_x2 += dx * dx;
			sum_y2 += dy * dy;
		}
		double den = sqrt(sum_x2 * sum_y2);
		out[r] = den == 0.0 ? 0.0 : sum_xy / den;
	}
}

// Jaccard (vector.rs:317-340): bit-pattern sets — |I|/|U| with the
// reference's F32 asymmetry restated as-is. One block per row; two LDS
// open-addressing sets (query uniques, row uniques). The counted
// quantities are order-independent restatements of the reference's
// progressive-insert loop: inter = per row element [bits in unique(q)] or
// [non-first duplicate within the row]; |U| = |unique(q)| + |unique(row)
// \ unique(q)|. d <= 1024 (LDS capacity; the guard is in the caller).
#define JACC_SLOTS 2048
#define JACC_EMPTY 0xFFFFFFFFu
__global__ __launch_bounds__(256) void k_jaccard_dists(
    const float *__restrict__ cm, uint64_t n, uint64_t n_pad, uint32_t d,
    const float *__restrict__ qg, double *__restrict__ out) {
	__shared__ uint32_t setA[JACC_SLOTS];
	__shared__ uint32_t setB[JACC_SLOTS];
	__shared__ uint32_t suA, interS, bNotA;
	__shared__ int sentA, sentB; // the 0xFFFFFFFF bit pattern, if present
	uint64_t r = blockIdx.x;
	if (r >= n)
		return;
	for (uint32_t i = threadIdx.x; i < JACC_SLOTS; i += 256) {
		setA[i] = JACC_EMPTY;
		setB[i] = JACC_EMPTY;
	}
	if (threadIdx.x == 0) {
		suA = 0;
		interS = 0;
		bNotA = 0;
		sentA = 0;
		sentB = 0;
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < d; i += 256) {
		uint32_t bits = __float_as_uint(qg[i]);
		if (bits == JACC_EMPTY) {
			if (atomicOr(&sentA, 1) == 0)
				atomicAdd(&suA, 1);
			continue;
		}
		uint32_t h = (bits * 2654435761u) & (JACC_SLOTS - 1);
		for (;;) {
			uint32_t prev = atomicCAS(&setA[h], JACC_EMPTY, bits);
			if (prev == JACC_EMPTY) {
				atomicAdd(&suA, 1);
				break;
			}
			if (prev == bits)
				break;
			h = (h + 1) & (JACC_SLOTS - 1);
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < d; i += 256) {
		uint32_t bits = __float_as_uint(cm[(uint64_t)i * n_pad + r]);
		bool inA;
		if (bits == JACC_EMPTY) {
			inA = sentA != 0;
		} else {
			inA = false;
			uint32_t h = (bits * 2654435761u) & (JACC_SLOTS - 1);
			for (;;) {
				uint32_t v = setA[h];
				if (v == bits) {
					inA = true;
					break;
				}
				if (v == JACC_EMPTY)
					break;
				h = (h + 1) & (JACC_SLOTS - 1);
			}
		}
		if (inA) {
			atomicAdd(&interS, 1);
			continue;
		}
		if (bits == JACC_EMPTY) {
			if (atomicOr(&sentB, 1) == 0)
				atomicAdd(&bNotA, 1);
			else
				atomicAdd(&interS, 1);
			continue;
		}
		uint32_t h = (bits * 2654435761u) & (JACC_SLOTS - 1);
		for (;;) {
			uint32_t prev = atomicCAS(&setB[h], JACC_EMPTY, bits);
			if (prev == JACC_EMPTY) {
				atomicAdd(&bNotA, 1);
				break;
			}
			if (prev == bits) {
				atomicAdd(&interS, 1);
				break;
			}
			h = (h + 1) & (JACC_SLOTS - 1);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0)
		out[r] = (double)interS / (double)(suA + bNotA);
}

// Gather + distance for HNSW frontier expansion: one block per frontier row,
// coalesced row read (rows gathered from the feature-major store).
template <int METRIC>
__global__ void k_gather_dist(const float *__restrict__ cm,
                              const double *__restrict__ norms, uint64_t n_pad,
                              uint32_t d, const uint32_t *__restrict__ rows,
                              uint32_t nrows, const float *__restrict__ qg,
                              double q_norm, double *__restrict__ out) {
	uint32_t i = blockIdx.x;
	if (i >= nrows)
		return;
	uint32_t r = rows[i];
	// single lane computes the exact per-row chain; other lanes prefetch via L2
	if (threadIdx.x == 0) {
		if (METRIC == 0) {
			float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			uint32_t k = 0;
			for (; k + 8 <= d; k += 8)
#pragma unroll
				for (uint32_t j = 0; j < 8; j++)
					p[j] = __fadd_rn(
					    p[j], __fmul_rn(cm[(uint64_t)(k + j) * n_pad + r], qg[k + j]));
			float sum = 0.f;
			sum = __fadd_rn(sum, __fadd_rn(p[0], p[4]));
			sum = __fadd_rn(sum, __fadd_rn(p[1], p[5]));
			sum = __fadd_rn(sum, __fadd_rn(p[2], p[6]));
			sum = __fadd_rn(sum, __fadd_rn(p[3], p[7]));
			for (; k < d; k++)
				sum = __fadd_rn(sum, __fmul_rn(cm[(uint64_t)k * n_pad + r], qg[k]));
			out[i] = 1.0 - (double)sum / (q_norm * norms[r]);
		} else {
			float acc = 0.f;
			for (uint32_t k = 0; k < d; k++) {
				float diff = cm[(uint64_t)k * n_pad + r] - qg[k];
				acc = __fadd_rn(acc, __fmul_rn(diff, diff));
			}
			out[i] = sqrt((double)acc);
		}
	}
}

// ---------------------------------------------------------------------------
// Batched-query path (BASELINE configs[3]) — the genuinely-dense case.
// scores = corpus x Q^T runs as a plain f32 GEMM on MFMA (rocBLAS; the
// feature-major store [d][n_pad] IS the column-major corpus matrix with
// lda = n_pad, so no transform is needed). Selection per query uses a
// monotone f32 approximation of the distance as the key; the survivors
// (k + SLACK per query) are then recomputed with the exact restated chain so
// the final scores are bitwise identical to the single-query path, and
// re-ranked by the exact (total_cmp dist, id) order.
// ---------------------------------------------------------------------------
#define BATCH_SLACK 16

__device__ static inline uint64_t d_total_key32(float x) {
	uint32_t bits = __float_as_uint(x);
	uint32_t k = (bits >> 31) ? ~bits : (bits | 0x80000000u);
	return (uint64_t)k;
}

struct BCand {
	float key; // monotone f32 selection key (smaller = better)
	uint32_t row;
};

__global__ void k_binit(BCand *state, uint64_t total) {
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < total) {
		state[i].key = __uint_as_float(0x7F800000u); // +inf
		state[i].row = ~0u;
	}
}

// What staging learns about a table for the batch path besides aux.
struct BatchAuxHdr {
	unsigned long long max_norm_bits; // largest norm of a row with a key (f64
	                                  // bits: non-negative doubles order as u64)
	uint32_t n_unc;                   // rows without a usable key
	uint32_t pad;
};
// Rows without a usable key the batch call lists and recomputes exactly for
// every query; a table with more of them is answered by the exact scan.
#define BATCH_UNC_CAP 1024u

// f32 aux for the selection key: cosine -> 1/norm, euclidean -> restated f32
// sum-of-squares per row. A row the key bound (batch_key_bound) cannot cover
// -- norm non-finite or above PF_NORM_MAX, for cosine also below PF_NORM_MIN,
// zero included -- gets aux = NaN, which makes its key NaN for every query, and
// is appended to unc_rows (in no particular order).
__global__ void k_aux(const float *__restrict__ cm,
                      const double *__restrict__ norms,
                      float *__restrict__ aux, uint64_t n, uint64_t n_pad,
                      uint32_t d, int metric, uint32_t *__restrict__ unc_rows,
                      BatchAuxHdr *__restrict__ hdr) {
	uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n)
		return;
	float a;
	double norm;
	if (metric == 0) {
		norm = norms[r];
		a = (float)(1.0 / norm);
	} else {
		float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t k = 0;
		for (; k + 8 <= d; k += 8) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				float x = cm[(uint64_t)(k + j) * n_pad + r];
				p[j] = __fadd_rn(p[j], __fmul_rn(x, x));
			}
		}
		float acc = 0.0f;
		acc = __fadd_rn(acc,
		                __fadd_rn(__fadd_rn(p[0], p[4]), __fadd_rn(p[1], p[5])));
		acc = __fadd_rn(acc,
		                __fadd_rn(__fadd_rn(p[2], p[6]), __fadd_rn(p[3], p[7])));
		for (; k < d; k++) {
			float x = cm[(uint64_t)k * n_pad + r];
			acc = __fadd_rn(acc, __fmul_rn(x, x));
		}
		a = acc;
		norm = sqrt((double)acc);
	}
	const bool covered =
	    norm <= PF_NORM_MAX && (metric != 0 || norm >= PF_NORM_MIN);
	if (covered) {
		aux[r] = a;
		atomicMax(&hdr->max_norm_bits,
		          (unsigned long long)__double_as_longlong(norm));
	} else {
		aux[r] = __uint_as_float(0x7FC00000u);
		uint32_t idx = atomicAdd(&hdr->n_unc, 1u);
		if (idx < BATCH_UNC_CAP)
			unc_rows[idx] = (uint32_t)r;
	}
}

// ---------------------------------------------------------------------------
// In-place append (sdbv_append_rows): rows [n, n + m) of a
// table with spare capacity, in one launch what k_transpose, k_fill_ids,
// k_norms and k_aux do for a whole table.
// One wave per 64 absolute-aligned rows (block = one wave), lane = row; lanes
// whose row lies outside [n, n + m) write nothing. The wave walks the
// features in blocks of APP_FB: it loads the row-major block coalesced
// (256 B per row) into an LDS tile of odd row length, reads it back
// transposed and writes cm[k * n_pad + r], 64 consecutive floats per
// feature. APP_FB is a multiple of 8, so k % 8 is the position in the block
// and each lane carries the sum-of-squares chain of k_norms / k_aux in
// registers: eight partials by k % 8 over the whole groups of 8, combined as
// ((p0+p4)+(p1+p5)) + ((p2+p6)+(p3+p7)), then the d % 8 tail in sequence.
// rm holds the m new rows row-major; ids their ids, or null for id_next +
// (r - n). norms is null off cosine tables, aux / unc_rows / hdr are null
// off cosine and euclidean ones. hdr is the table's own and is not reset:
// its maximum and its count continue.
// ---------------------------------------------------------------------------
#define APP_FB 64
__global__ __launch_bounds__(64) void k_append_rows(
    const float *__restrict__ rm, const uint64_t *__restrict__ ids,
    uint64_t id_next, float *__restrict__ cm, double *__restrict__ norms,
    float *__restrict__ aux, uint64_t *__restrict__ ids_dev, uint64_t n,
    uint64_t m, uint64_t n_pad, uint32_t d, int metric,
    uint32_t *__restrict__ unc_rows, BatchAuxHdr *__restrict__ hdr) {
	__shared__ float tile[64][APP_FB + 1];
	const uint32_t lane = threadIdx.x;
	const uint64_t base = (n / 64 + blockIdx.x) * 64; // first row of the wave
	const uint64_t r = base + lane;
	const bool mine = r >= n && r < n + m; // r < n_pad: the host checked
	const uint32_t d8 = d & ~7u;
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	float tail[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // x * x of the d % 8 tail
	for (uint32_t kb = 0; kb < d; kb += APP_FB) {
		const uint32_t k = kb + lane;
		// eight rows' loads in flight before their LDS stores
#pragma unroll 1
		for (uint32_t i0 = 0; i0 < 64; i0 += 8) {
			float v[8];
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				const uint64_t ri = base + i0 + j;
				v[j] = 0.0f;
				if (ri >= n && ri < n + m && k < d)
					v[j] = rm[(ri - n) * d + k];
			}
#pragma unroll
			for (uint32_t j = 0; j < 8; j++)
				tile[i0 + j][lane] = v[j];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t g = 0; g < APP_FB; g += 8) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				const uint32_t kk = kb + g + j;
				const float x = tile[lane][g + j];
				if (kk < d) {
					if (mine)
						cm[(uint64_t)kk * n_pad + r] = x;
					const float xx = __fmul_rn(x, x);
					if (kk < d8)
						p[j] = __fadd_rn(p[j], xx);
					else
						tail[j] = xx;
				}
			}
		}
		__syncthreads();
	}
	if (!mine)
		return;
	ids_dev[r] = ids ? ids[r - n] : id_next + (r - n);
	if (!norms && !aux)
		return;
	float acc = 0.0f;
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[0], p[4]), __fadd_rn(p[1], p[5])));
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[2], p[6]), __fadd_rn(p[3], p[7])));
#pragma unroll
	for (uint32_t j = 0; j < 8; j++)
		if (d8 + j < d)
			acc = __fadd_rn(acc, tail[j]);
	const double norm = sqrt((double)acc);
	if (norms)
		norms[r] = norm;
	if (!aux)
		return;
	// as k_aux: cosine 1 / norm, euclidean the sum of squares
	const float a = metric == 0 ? (float)(1.0 / norm) : acc;
	const bool covered =
	    norm <= PF_NORM_MAX && (metric != 0 || norm >= PF_NORM_MIN);
	if (covered) {
		aux[r] = a;
		atomicMax(&hdr->max_norm_bits,
		          (unsigned long long)__double_as_longlong(norm));
	} else {
		aux[r] = __uint_as_float(0x7FC00000u);
		uint32_t idx = atomicAdd(&hdr->n_unc, 1u);
		if (idx < BATCH_UNC_CAP)
			unc_rows[idx] = (uint32_t)r;
	}
}

// ---------------------------------------------------------------------------
// In-place update (sdbv_update_rows): the scatter sibling of
// k_append_rows. One wave per 64 consecutive entries of the row list, lane =
// entry i, target row idx[i] (strictly increasing, all < n: the host
// checked, so no two lanes write the same row). rm holds the m new rows
// row-major. The loads are those of the append; the stores of a feature go
// to cm[k * n_pad + idx[i]], scattered unless the listed rows are adjacent.
// norms[row] and aux[row] are written as k_norms / k_aux would (aux NaN for
// a row without a usable key); the batch header, the list of such rows and
// the ids are not touched: k_aux_refold recomputes the first two.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_update_rows(
    const float *__restrict__ rm, const uint32_t *__restrict__ idx,
    float *__restrict__ cm, double *__restrict__ norms,
    float *__restrict__ aux, uint64_t m, uint64_t n_pad, uint32_t d,
    int metric) {
	__shared__ float tile[64][APP_FB + 1];
	const uint32_t lane = threadIdx.x;
	const uint64_t base = (uint64_t)blockIdx.x * 64; // first entry of the wave
	const bool mine = base + lane < m;
	const uint64_t r = mine ? idx[base + lane] : 0;
	const uint32_t d8 = d & ~7u;
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	float tail[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // x * x of the d % 8 tail
	for (uint32_t kb = 0; kb < d; kb += APP_FB) {
		const uint32_t k = kb + lane;
		// eight rows' loads in flight before their LDS stores
#pragma unroll 1
		for (uint32_t i0 = 0; i0 < 64; i0 += 8) {
			float v[8];
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				const uint64_t si = base + i0 + j;
				v[j] = 0.0f;
				if (si < m && k < d)
					v[j] = rm[si * d + k];
			}
#pragma unroll
			for (uint32_t j = 0; j < 8; j++)
				tile[i0 + j][lane] = v[j];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t g = 0; g < APP_FB; g += 8) {
#pragma unroll
			for (uint32_t j = 0; j < 8; j++) {
				const uint32_t kk = kb + g + j;
				const float x = tile[lane][g + j];
				if (kk < d) {
					if (mine)
						cm[(uint64_t)kk * n_pad + r] = x;
					const float xx = __fmul_rn(x, x);
					if (kk < d8)
						p[j] = __fadd_rn(p[j], xx);
					else
						tail[j] = xx;
				}
			}
		}
		__syncthreads();
	}
	if (!mine || (!norms && !aux))
		return;
	float acc = 0.0f;
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[0], p[4]), __fadd_rn(p[1], p[5])));
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[2], p[6]), __fadd_rn(p[3], p[7])));
#pragma unroll
	for (uint32_t j = 0; j < 8; j++)
		if (d8 + j < d)
			acc = __fadd_rn(acc, tail[j]);
	const double norm = sqrt((double)acc);
	if (norms)
		norms[r] = norm;
	if (!aux)
		return;
	// as k_aux: cosine 1 / norm, euclidean the sum of squares
	const float a = metric == 0 ? (float)(1.0 / norm) : acc;
	const bool covered =
	    norm <= PF_NORM_MAX && (metric != 0 || norm >= PF_NORM_MIN);
	aux[r] = covered ? a : __uint_as_float(0x7FC00000u);
}

// The batch header from the arrays (sdbv_update_rows): over aux[0..n), a row
// with NaN aux is counted and listed in unc_rows while the count is below
// BATCH_UNC_CAP, every other row gives its norm to the maximum -- norms[r] on
// a cosine table, sqrt((double)aux[r]) on a euclidean one, the value k_aux
// had. hdr is zero on entry. A wave reduces first: one atomicAdd for its
// rows without a key, whose lanes take consecutive slots; the maximum goes
// wave, then workgroup, then one atomicMax per workgroup when it leaves.
// Grid-stride: at most this many workgroups, four per compute unit of a
// 256-unit device, so a table whose rows all have a key issues at most 1024
// atomics to the one address.
#define REFOLD_MAX_BLOCKS 1024u
__global__ __launch_bounds__(THREADS) void k_aux_refold(
    const float *__restrict__ aux, const double *__restrict__ norms,
    uint64_t n, uint32_t *__restrict__ unc_rows,
    BatchAuxHdr *__restrict__ hdr) {
	__shared__ unsigned long long wave_best[THREADS / 64];
	const uint32_t lane = threadIdx.x & 63;
	unsigned long long best = 0;
	// the loop bound is the wave's first row: all 64 lanes stay together
	for (uint64_t r0 = (uint64_t)blockIdx.x * THREADS + (threadIdx.x & ~63u);
	     r0 < n; r0 += (uint64_t)gridDim.x * THREADS) {
		const uint64_t r = r0 + lane;
		bool unc = false;
		if (r < n) {
			const float a = aux[r];
			unc = a != a;
			if (!unc) {
				const double norm = norms ? norms[r] : sqrt((double)a);
				const unsigned long long b =
				    (unsigned long long)__double_as_longlong(norm);
				best = b > best ? b : best;
			}
		}
		const unsigned long long vote = __ballot(unc);
		if (vote) {
			const int leader = __ffsll((long long)vote) - 1;
			uint32_t slot = 0;
			if ((int)lane == leader)
				slot = atomicAdd(&hdr->n_unc, (uint32_t)__popcll(vote));
			slot = __shfl(slot, leader);
			slot += (uint32_t)__popcll(vote & ((1ull << lane) - 1));
			if (unc && slot < BATCH_UNC_CAP)
				unc_rows[slot] = (uint32_t)r;
		}
	}
	for (int off = 32; off > 0; off >>= 1) {
		const unsigned long long o = __shfl_down(best, off);
		best = o > best ? o : best;
	}
	if (lane == 0)
		wave_best[threadIdx.x >> 6] = best;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (uint32_t w = 1; w < THREADS / 64; w++)
			best = wave_best[w] > best ? wave_best[w] : best;
		if (best)
			atomicMax(&hdr->max_norm_bits, best);
	}
}

// Growth of a table's store: dst [d][new_pad] receives src [d][old_pad]
// column by column and zeros in every cell at or past old_pad. Both strides
// are multiples of 4, so a float4 never straddles a column or the old edge.
__global__ void k_grow_cm(const float *__restrict__ src,
                          float *__restrict__ dst, uint64_t old_pad,
                          uint64_t new_pad, uint32_t d) {
	const uint64_t q_new = new_pad / 4;
	const uint64_t total = (uint64_t)d * q_new;
	for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	     idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t k = idx / q_new;
		const uint64_t r = (idx % q_new) * 4;
		float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
		if (r < old_pad)
			v = *(const float4 *)(src + k * old_pad + r);
		*(float4 *)(dst + k * new_pad + r) = v;
	}
}

// Per-query f64 norms of a row-major Q (restated sumsq chain + f64 sqrt).
__global__ void k_qnorms(const float *__restrict__ Q, uint32_t b, uint32_t d,
                         double *__restrict__ out) {
	uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= b)
		return;
	const float *a = Q + (uint64_t)j * d;
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t i = 0;
	for (; i + 8 <= d; i += 8)
#pragma unroll
		for (uint32_t t = 0; t < 8; t++)
			p[t] = __fadd_rn(p[t], __fmul_rn(a[i + t], a[i + t]));
	float acc = 0.0f;
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[0], p[4]), __fadd_rn(p[1], p[5])));
	acc = __fadd_rn(acc, __fadd_rn(__fadd_rn(p[2], p[6]), __fadd_rn(p[3], p[7])));
	for (; i < d; i++)
		acc = __fadd_rn(acc, __fmul_rn(a[i], a[i]));
	out[j] = sqrt((double)acc);
}

// Per-query running top-(kk) update over one GEMM chunk.
// S is [n_chunk x b] column-major (column j = scores of query j, contiguous).
// metric 0 (cosine): key = -(s * inv_norm)   (maximise normalised dot)
// metric 1 (euclid): key = sumsq_row - 2*s   (minimise ||q-r||^2 - qn2)
__global__ __launch_bounds__(THREADS) void k_batch_topk(
    const float *__restrict__ S, const float *__restrict__ aux,
    uint64_t row0, uint32_t n_chunk, uint64_t n, int metric,
    BCand *__restrict__ state, int kk) {
	__shared__ LCand buf[TILE + MAX_K];
	__shared__ LCand topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth_key;
	__shared__ uint32_t kth_row;

	uint32_t j = blockIdx.x;
	const float *col = S + (uint64_t)j * n_chunk;
	BCand *st = state + (uint64_t)j * kk;

	// load current state into LDS topk (keys already total-ordered u64)
	if (threadIdx.x == 0) {
		cnt = 0;
		topk_n = 0;
		kth_key = ~0ULL;
		kth_row = ~0u;
	}
	__syncthreads();
	if (threadIdx.x < (uint32_t)kk) {
		BCand c = st[threadIdx.x];
		if (c.row != ~0u) {
			topk[threadIdx.x].key = d_total_key32(c.key);
			topk[threadIdx.x].dist = (double)c.key;
			topk[threadIdx.x].row = c.row;
			atomicAdd(&topk_n, 1);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0 && topk_n >= kk) {
		kth_key = topk[kk - 1].key;
		kth_row = topk[kk - 1].row;
	}
	__syncthreads();

	for (uint32_t tile = 0; tile < n_chunk; tile += TILE) {
		uint32_t i0 = tile + threadIdx.x * 4;
		uint64_t kk_key = kth_key;
		uint32_t kk_row = kth_row;
		int full = (topk_n >= kk);
		if (i0 + 3 < n_chunk) {
			const float4 s4 = *(const float4 *)(col + i0);
			float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
			for (int c = 0; c < 4; c++) {
				uint64_t r = row0 + i0 + c;
				if (r >= n)
					continue;
				float key = (metric == 0) ? -(sv[c] * aux[r])
				                          : (aux[r] - 2.0f * sv[c]);
				if (key != key)
					continue; // a row without a usable key (aux = NaN)
				uint64_t tk = d_total_key32(key);
				uint32_t row32 = (uint32_t)r;
				bool take =
				    !full || tk < kk_key || (tk == kk_key && row32 < kk_row);
				if (take) {
					int idx = atomicAdd(&cnt, 1);
					buf[idx].key = tk;
					buf[idx].dist = (double)key;
					buf[idx].row = row32;
				}
			}
		}
		__syncthreads();
		if (cnt > 0) {
			int m = cnt;
			for (int i = threadIdx.x; i < topk_n; i += THREADS)
				buf[m + i] = topk[i];
			int total = m + topk_n;
			__syncthreads();
			int new_n;
			block_select_topk(buf, total, topk, kk, &new_n);
			if (threadIdx.x == 0) {
				topk_n = new_n;
				if (new_n >= kk) {
					kth_key = topk[kk - 1].key;
					kth_row = topk[kk - 1].row;
				}
				cnt = 0;
			}
		}
		__syncthreads();
	}

	// write back
	if (threadIdx.x < (uint32_t)kk) {
		BCand c;
		if ((int)threadIdx.x < topk_n) {
			c.key = (float)topk[threadIdx.x].dist;
			c.row = topk[threadIdx.x].row;
		} else {
			c.key = __uint_as_float(0x7F800000u);
			c.row = ~0u;
		}
		st[threadIdx.x] = c;
	}
}

// ---------------------------------------------------------------------------
// Fused MFMA scan (the hand-written batch kernel): scores = corpus x Q^T on
// v_mfma_f32_32x32x2_f32 (exact f32 at the 157 TF vector rate), with the
// top-K filter fused into the epilogue — survivors (score key <= the
// query's bootstrapped kth-best threshold) append to a per-query candidate
// buffer; the b x n score matrix NEVER touches HBM (the round-1 rocBLAS +
// k_batch_topk path re-read ~41 GB/step of it). Thresholds bootstrap on the
// first n0 rows via the legacy path and stay put during the launch, so a
// query appends about kk*(n/n0 - 1) candidates (~1200 at 3M rows).
// Selection semantics are identical to k_batch_topk (exact running top-kk
// by (monotone f32 key, row)): the filter can only drop entries strictly
// worse than the current kk-th, and k_cand_fold recomputes the exact
// running top-kk from the survivors.
// Block tile 128x128 x K=32 LDS stages; 4 waves, each 2x2 subtiles of
// 32x32. A = cm (feature-major = column-major corpus, lda n_pad), B = Q
// row-major [b][d].
// ---------------------------------------------------------------------------
#define FMM_BM 128
#define FMM_BN 128
#define FMM_BK 32
#define FMM_LDS_PAD 4
#define FMM_CAND_CAP 4096u

typedef __attribute__((ext_vector_type(16))) float f32x16;

__global__ __launch_bounds__(256) void k_mfma_scan_topk(
    const float *__restrict__ cm, uint64_t n_pad, uint32_t d,
    const float *__restrict__ Q, uint32_t b, uint64_t row0, uint64_t row1,
    const float *__restrict__ aux, int metric,
    const uint32_t *__restrict__ theta, // per-query kth-best u32 key
    BCand *__restrict__ cand,           // [b][FMM_CAND_CAP]
    uint32_t *__restrict__ cand_cnt) {  // [b]
	__shared__ float As[FMM_BK][FMM_BM + FMM_LDS_PAD];
	__shared__ float Bs[FMM_BK][FMM_BN + FMM_LDS_PAD];
	const uint32_t wave = threadIdx.x >> 6;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wm = wave & 1;  // wave row (2x2 wave grid)
	const uint32_t wn = wave >> 1; // wave col
	const uint64_t brow = row0 + (uint64_t)blockIdx.x * FMM_BM;
	const uint32_t bcol = blockIdx.y * FMM_BN;
	f32x16 acc[2][2] = {};

	const uint32_t tid = threadIdx.x;
	// software pipeline: prefetch K-stage t+1 into registers while MFMA
	// consumes stage t from LDS (the naive load->sync->compute cycle
	// measured 73 TF; the guide's untuned same-shape reference is 122)
	// each thread stages 4 float4 of A (k = a_kq + 8r, fixed m4) and 4 of
	// B (j = b_jq + 32r, fixed k4): A has FMM_BK*FMM_BM/4 = 1024 float4
	// per stage over 256 threads, B likewise
	const uint32_t a_m4 = (tid % (FMM_BM / 4)) * 4; // 0..124
	const uint32_t b_k4 = (tid % (FMM_BK / 4)) * 4; // 0..28
	const uint32_t a_kq = tid / (FMM_BM / 4); // 0..7 (k quarter index)
	const uint32_t b_jq = tid / (FMM_BK / 4); // 0..31 (j quarter index)
	float4 pa[4], pb[4];
	auto prefetch = [&](uint32_t k0) {
#pragma unroll
		for (uint32_t r = 0; r < 4; r++) {
			uint32_t k = a_kq + 8 * r;
			pa[r] = *(const float4 *)(cm + (uint64_t)(k0 + k) * n_pad +
			                          brow + a_m4);
			uint32_t j = b_jq + 32 * r;
			pb[r] = *(const float4 *)(Q + (uint64_t)(bcol + j) * d + k0 +
			                          b_k4);
		}
	};
	auto stage_lds = [&]() {
#pragma unroll
		for (uint32_t r = 0; r < 4; r++) {
			uint32_t k = a_kq + 8 * r;
			As[k][a_m4 + 0] = pa[r].x;
			As[k][a_m4 + 1] = pa[r].y;
			As[k][a_m4 + 2] = pa[r].z;
			As[k][a_m4 + 3] = pa[r].w;
			uint32_t j = b_jq + 32 * r;
			Bs[b_k4 + 0][j] = pb[r].x;
			Bs[b_k4 + 1][j] = pb[r].y;
			Bs[b_k4 + 2][j] = pb[r].z;
			Bs[b_k4 + 3][j] = pb[r].w;
		}
	};
	prefetch(0);
	stage_lds();
	__syncthreads();
	for (uint32_t k0 = 0; k0 < d; k0 += FMM_BK) {
		if (k0 + FMM_BK < d)
			prefetch(k0 + FMM_BK); // in flight during the MFMA block
#pragma unroll
		for (uint32_t kk = 0; kk < FMM_BK; kk += 2) {
			// operand map (32x32x2): lane l holds A[i=l&31][k=l>>5],
			// B[k=l>>5][j=l&31]
			const uint32_t ai = lane & 31, ak = lane >> 5;
			float a0 = As[kk + ak][wm * 64 + ai];
			float a1 = As[kk + ak][wm * 64 + 32 + ai];
			float b0 = Bs[kk + ak][wn * 64 + ai];
			float b1 = Bs[kk + ak][wn * 64 + 32 + ai];
			acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0,
			                                                 acc[0][0], 0, 0, 0);
			acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0,
			                                                 acc[1][0], 0, 0, 0);
			acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1,
			                                                 acc[0][1], 0, 0, 0);
			acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1,
			                                                 acc[1][1], 0, 0, 0);
		}
		__syncthreads();
		if (k0 + FMM_BK < d) {
			stage_lds();
			__syncthreads();
		}
	}

	// epilogue: C/D map for 32x32 shapes — col = lane&31,
	// row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
	const uint32_t ccol = lane & 31;
	const uint32_t crow_base = 4 * (lane >> 5);
#pragma unroll
	for (uint32_t sn = 0; sn < 2; sn++) {
		uint32_t j = bcol + wn * 64 + sn * 32 + ccol;
		if (j >= b)
			continue;
		uint32_t th = theta[j];
#pragma unroll
		for (uint32_t sm = 0; sm < 2; sm++) {
#pragma unroll
			for (uint32_t rg = 0; rg < 16; rg++) {
				uint32_t rsub =
				    (rg & 3) + 8 * (rg >> 2) + crow_base;
				uint64_t row =
				    brow + wm * 64 + sm * 32 + rsub;
				if (row >= row1)
					continue;
				float s = acc[sm][sn][rg];
				float key = (metric == 0) ? -(s * aux[row])
				                          : (aux[row] - 2.0f * s);
				uint32_t tk = (uint32_t)d_total_key32(key);
				// key != key: a row without a usable key (aux = NaN)
				if (tk <= th && key == key) {
					uint32_t idx = atomicAdd(&cand_cnt[j], 1u);
					if (idx < FMM_CAND_CAP) {
						cand[(uint64_t)j * FMM_CAND_CAP + idx] =
						    BCand{key, (uint32_t)row};
					}
				}
			}
		}
	}
}

// Per-query thresholds from the bootstrapped running top-kk state.
__global__ void k_theta_init(const BCand *__restrict__ state, int kk,
                             uint32_t b, uint32_t *__restrict__ theta) {
	uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= b)
		return;
	BCand kth = state[(uint64_t)j * kk + (kk - 1)];
	theta[j] = kth.row == ~0u ? 0xFFFFFFFFu
	                          : (uint32_t)d_total_key32(kth.key);
}

// Fold each query's candidate buffer into its running top-kk state —
// identical comparator and tile loop as k_batch_topk, reading precomputed
// (key, row) pairs instead of a score matrix.
__global__ __launch_bounds__(THREADS) void k_cand_fold(
    const BCand *__restrict__ cand, const uint32_t *__restrict__ cand_cnt,
    BCand *__restrict__ state, int kk) {
	__shared__ LCand buf[TILE + MAX_K];
	__shared__ LCand topk[MAX_K];
	__shared__ int cnt;
	__shared__ int topk_n;
	__shared__ uint64_t kth_key;
	__shared__ uint32_t kth_row;
	uint32_t j = blockIdx.x;
	uint32_t m_in = cand_cnt[j];
	if (m_in > FMM_CAND_CAP)
		m_in = FMM_CAND_CAP; // overflow: host reruns via the legacy path
	const BCand *cj = cand + (uint64_t)j * FMM_CAND_CAP;
	BCand *st = state + (uint64_t)j * kk;
	if (threadIdx.x == 0) {
		cnt = 0;
		topk_n = 0;
		kth_key = ~0ULL;
		kth_row = ~0u;
	}
	__syncthreads();
	if (threadIdx.x < (uint32_t)kk) {
		BCand c = st[threadIdx.x];
		if (c.row != ~0u) {
			topk[threadIdx.x].key = d_total_key32(c.key);
			topk[threadIdx.x].dist = (double)c.key;
			topk[threadIdx.x].row = c.row;
			atomicAdd(&topk_n, 1);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0 && topk_n >= kk) {
		kth_key = topk[kk - 1].key;
		kth_row = topk[kk - 1].row;
	}
	__syncthreads();
	// a tile is TILE candidates, ROWS_PER_LANE per thread (one per thread
	// left three quarters of every tile unread: wrong results from 257
	// candidates on)
	for (uint32_t tile = 0; tile < m_in; tile += TILE) {
		uint64_t kk_key = kth_key;
		uint32_t kk_row = kth_row;
		int full = (topk_n >= kk);
#pragma unroll
		for (uint32_t l = 0; l < ROWS_PER_LANE; l++) {
			uint32_t i = tile + l * THREADS + threadIdx.x;
			if (i >= m_in)
				break;
			BCand c = cj[i];
			uint64_t tk = d_total_key32(c.key);
			bool take = !full || tk < kk_key ||
			            (tk == kk_key && c.row < kk_row);
			if (take) {
				int idx = atomicAdd(&cnt, 1);
				buf[idx].key = tk;
				buf[idx].dist = (double)c.key;
				buf[idx].row = c.row;
			}
		}
		__syncthreads();
		if (cnt > 0) {
			int m = cnt;
			for (int i2 = threadIdx.x; i2 < topk_n; i2 += THREADS)
				buf[m + i2] = topk[i2];
			int total = m + topk_n;
			__syncthreads();
			int new_n;
			block_select_topk(buf, total, topk, kk, &new_n);
			if (threadIdx.x == 0) {
				topk_n = new_n;
				if (new_n >= kk) {
					kth_key = topk[kk - 1].key;
					kth_row = topk[kk - 1].row;
				}
				cnt = 0;
			}
		}
		__syncthreads();
	}
	if (threadIdx.x < (uint32_t)kk) {
		BCand c;
		if ((int)threadIdx.x < topk_n) {
			c.key = (float)topk[threadIdx.x].dist;
			c.row = topk[threadIdx.x].row;
		} else {
			c.key = __uint_as_float(0x7F800000u);
			c.row = ~0u;
		}
		st[threadIdx.x] = c;
	}
}

// Exact recompute of each surviving candidate with the restated per-row
// chain (bitwise identical to the single-query scan path).
__global__ void k_batch_exact(const float *__restrict__ cm,
                              const double *__restrict__ norms,
                              uint64_t n_pad, uint32_t d,
                              const float *__restrict__ Q,
                              const double *__restrict__ qnorms, int metric,
                              const BCand *__restrict__ state,
                              const uint32_t *__restrict__ shared_rows, int kk,
                              double *__restrict__ out) {
	uint32_t j = blockIdx.x;  // query
	uint32_t c = blockIdx.y;  // candidate slot
	if (threadIdx.x != 0)
		return;
	// shared_rows: the same kk rows for every query (the rows without a
	// usable key) in place of the query's own window
	BCand cand = shared_rows ? BCand{0.f, shared_rows[c]}
	                         : state[(uint64_t)j * kk + c];
	double *o = out + (uint64_t)j * kk + c;
	if (cand.row == ~0u) {
		*o = __longlong_as_double(0x7FF0000000000000LL);
		return;
	}
	const float *q = Q + (uint64_t)j * d;
	uint64_t r = cand.row;
	if (metric == 0) {
		float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t k = 0;
		for (; k + 8 <= d; k += 8)
#pragma unroll
			for (uint32_t t = 0; t < 8; t++)
				p[t] = __fadd_rn(
				    p[t], __fmul_rn(cm[(uint64_t)(k + t) * n_pad + r], q[k + t]));
		float sum = 0.f;
		sum = __fadd_rn(sum, __fadd_rn(p[0], p[4]));
		sum = __fadd_rn(sum, __fadd_rn(p[1], p[5]));
		sum = __fadd_rn(sum, __fadd_rn(p[2], p[6]));
		sum = __fadd_rn(sum, __fadd_rn(p[3], p[7]));
		for (; k < d; k++)
			sum = __fadd_rn(sum, __fmul_rn(cm[(uint64_t)k * n_pad + r], q[k]));
		*o = 1.0 - (double)sum / (qnorms[j] * norms[r]);
	} else {
		float acc = 0.f;
		for (uint32_t k = 0; k < d; k++) {
			float diff = cm[(uint64_t)k * n_pad + r] - q[k];
			acc = __fadd_rn(acc, __fmul_rn(diff, diff));
		}
		*o = sqrt((double)acc);
	}
}

// ---------------------------------------------------------------------------
// Persistent HNSW ef-search kernel: ONE query per 64-thread workgroup, the
// entire best-first loop (layer.rs:184-223) inside one launch. Queues live in
// LDS as append-only arrays with wave-parallel (key,seq) min/max scans —
// exactly the DoublePriorityQueue semantics (knn.rs:15-123: total_cmp order,
// FIFO within equal distance, pop_last = latest of the max key). Neighbour
// distances: one LANE per row over the ROW-MAJOR vector copy with the
// restated per-row chain (bit-identical to the oracle / single-query path).
// Visited set: per-query global bitset.
// ---------------------------------------------------------------------------
#define HQ_CAND_CAP 2048
#define HQ_EF_CAP 512
#define HQ_FLAG_OVERFLOW 1u

// PADDED=0: offsets/edges are the scrubbed layer-0 CSR (search path after
// finalize). PADDED=1: `offsets` is a per-node degree array and `edges` a
// padded [n][stride] adjacency — the GPU snapshot build's delta-updatable
// graph (sdbv_hnsw_insert_batch_snapshot_gpu), where per-chunk edge
// changes scatter into rows instead of re-laying-out a CSR.
// `ep_off` selects the seeding mode: NULL = one entry point per query
// (ep_rows[qid]); non-NULL = the insert path's multi-ep seeding — query
// qid seeds from ep_rows/ep_dists[ep_off[qid] .. ep_off[qid+1]), already
// in (dist total_cmp, seq) order (the previous layer's w, layer.rs:342).
template <int PADDED>
__global__ __launch_bounds__(64) void k_hnsw_search(
    const float *__restrict__ rm, const double *__restrict__ norms,
    uint32_t d, int metric, const uint32_t *__restrict__ offsets,
    const uint32_t *__restrict__ edges, uint32_t stride,
    const float *__restrict__ Q,
    const double *__restrict__ qnorms, const uint32_t *__restrict__ ep_rows,
    const double *__restrict__ ep_dists, const uint32_t *__restrict__ ep_off,
    uint32_t *__restrict__ visited,
    uint64_t vwords_per_q, uint32_t k, uint32_t ef,
    uint32_t *__restrict__ out_rows, double *__restrict__ out_dists,
    uint32_t *__restrict__ out_cnt, uint32_t *__restrict__ out_flags) {
	__shared__ uint64_t c_key[HQ_CAND_CAP];
	__shared__ uint32_t c_seq[HQ_CAND_CAP];
	__shared__ uint32_t c_row[HQ_CAND_CAP];
	__shared__ uint64_t w_key[HQ_EF_CAP];
	__shared__ uint32_t w_seq[HQ_EF_CAP];
	__shared__ uint32_t w_row[HQ_EF_CAP];

	const uint32_t qid = blockIdx.x;
	const int lane = threadIdx.x;
	const float *q = Q + (uint64_t)qid * d;
	const double qn = qnorms[qid];
	uint32_t *vis = visited + (uint64_t)qid * vwords_per_q;

	// state kept wave-uniform in registers (updated by every lane alike)
	uint32_t c_cnt = 0;   // append cursor of candidates
	uint32_t w_cnt = 0;
	uint32_t seq = 0;
	uint32_t flags = 0;
	uint64_t fq_key = ~0ULL; // max key in w (or +max when w not full)
	uint32_t fq_idx = 0;

	// seed with the entry point(s) (search_single layer.rs:76-90; insert's
	// search_multi seeds the whole previous-layer w, layer.rs:342-358)
	{
		uint32_t e0 = ep_off ? ep_off[qid] : qid;
		uint32_t e1 = ep_off ? ep_off[qid + 1] : qid + 1;
		uint32_t ne = e1 - e0;
		for (uint32_t i = lane; i < ne; i += 64) {
			uint64_t ek = d_total_key(ep_dists[e0 + i]);
			uint32_t er = ep_rows[e0 + i];
			c_key[i] = ek;
			c_seq[i] = i;
			c_row[i] = er;
			w_key[i] = ek;
			w_seq[i] = i;
			w_row[i] = er;
			atomicOr(&vis[er >> 5], 1u << (er & 31));
		}
		c_cnt = ne;
		w_cnt = ne;
		seq = ne;
		// eps arrive sorted ascending (key, seq): the max is the last
		fq_key = d_total_key(ep_dists[e1 - 1]);
		fq_idx = ne - 1;
	}
	__syncthreads();

	auto wave_min_cand = [&](uint64_t *bk, uint32_t *bs, int *bi) {
		uint64_t mk = ~0ULL;
		uint32_t ms = ~0u;
		int mi = -1;
		for (uint32_t i = lane; i < c_cnt; i += 64) {
			uint64_t kk = c_key[i];
			uint32_t ss = c_seq[i];
			if (kk < mk || (kk == mk && ss < ms)) {
				mk = kk;
				ms = ss;
				mi = (int)i;
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			uint64_t ok = __shfl_down(mk, off);
			uint32_t os = __shfl_down(ms, off);
			int oi = __shfl_down(mi, off);
			if (ok < mk || (ok == mk && os < ms)) {
				mk = ok;
				ms = os;
				mi = oi;
			}
		}
		*bk = __shfl(mk, 0);
		*bs = __shfl(ms, 0);
		*bi = __shfl(mi, 0);
	};
	auto wave_max_w = [&](uint64_t *bk, uint32_t *bi) {
		// max by (key, seq): latest seq among the max key
		uint64_t mk = 0;
		uint32_t ms = 0;
		int mi = 0;
		for (uint32_t i = lane; i < w_cnt; i += 64) {
			uint64_t kk = w_key[i];
			uint32_t ss = w_seq[i];
			if (kk > mk || (kk == mk && ss > ms)) {
				mk = kk;
				ms = ss;
				mi = (int)i;
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			uint64_t ok = __shfl_down(mk, off);
			uint32_t os = __shfl_down(ms, off);
			int oi = __shfl_down(mi, off);
			if (ok > mk || (ok == mk && os > ms)) {
				mk = ok;
				ms = os;
				mi = oi;
			}
		}
		*bk = __shfl(mk, 0);
		*bi = __shfl(mi, 0);
	};

	// main best-first loop
	for (;;) {
		uint64_t ck;
		uint32_t cs;
		int ci;
		wave_min_cand(&ck, &cs, &ci);
		if (ci < 0)
			break;
		// cq_dist > fq_dist -> stop (strict, distance only; fq = max of w
		// from the very first element, layer.rs:184)
		if (ck > fq_key)
			break;
		uint32_t doc = c_row[ci];
		if (lane == 0)
			c_key[ci] = ~0ULL; // tombstone
		__syncthreads();

		uint32_t e0, e1;
		if (PADDED) {
			e0 = doc * stride;
			e1 = e0 + offsets[doc]; // offsets = per-node degree
		} else {
			e0 = offsets[doc];
			e1 = offsets[doc + 1];
		}
		for (uint32_t base = e0; base < e1; base += 64) {
			uint32_t my_e = ~0u;
			double my_d = 0.0;
			bool mine = false;
			uint32_t idx = base + lane;
			if (idx < e1) {
				uint32_t e = edges[idx];
				uint32_t old = atomicOr(&vis[e >> 5], 1u << (e & 31));
				if (!(old & (1u << (e & 31)))) {
					mine = true;
					my_e = e;
					// restated per-row chain from the row-major copy
					const float *row = rm + (uint64_t)e * d;
					if (metric == 0) {
						float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
						uint32_t kk = 0;
						for (; kk + 8 <= d; kk += 8)
#pragma unroll
							for (uint32_t t = 0; t < 8; t++)
								p[t] = __fadd_rn(
								    p[t], __fmul_rn(row[kk + t], q[kk + t]));
						float sum = 0.f;
						sum = __fadd_rn(sum, __fadd_rn(p[0], p[4]));
						sum = __fadd_rn(sum, __fadd_rn(p[1], p[5]));
						sum = __fadd_rn(sum, __fadd_rn(p[2], p[6]));
						sum = __fadd_rn(sum, __fadd_rn(p[3], p[7]));
						for (; kk < d; kk++)
							sum = __fadd_rn(sum,
							                __fmul_rn(row[kk], q[kk]));
						my_d = 1.0 - (double)sum / (qn * norms[e]);
					} else {
						float acc = 0.f;
						for (uint32_t kk = 0; kk < d; kk++) {
							float diff = row[kk] - q[kk];
							acc = __fadd_rn(acc, __fmul_rn(diff, diff));
						}
						my_d = sqrt((double)acc);
					}
				}
			}
			// serial accept/update in edge order (layer.rs:195-218)
			uint32_t nlanes = (e1 - base) < 64 ? (e1 - base) : 64;
			for (uint32_t i = 0; i < nlanes; i++) {
				int src = (int)i;
				bool m = __shfl(mine ? 1 : 0, src) != 0;
				if (!m)
					continue;
				uint32_t erow = __shfl(my_e, src);
				double ed = __shfl(my_d, src);
				uint64_t ekey = d_total_key(ed);
				// e_dist < fq_dist || w.len < ef  (strict distance compare)
				if (!(w_cnt < ef || ekey < fq_key))
					continue;
				// candidates.push
				if (c_cnt < HQ_CAND_CAP) {
					if (lane == 0) {
						c_key[c_cnt] = ekey;
						c_seq[c_cnt] = seq;
						c_row[c_cnt] = erow;
					}
					c_cnt++;
				} else {
					flags |= HQ_FLAG_OVERFLOW;
				}
				__syncthreads();
				// w.push + (w.len > ef ? pop_last) as a conditional replace
				bool replaced = false;
				if (w_cnt < ef) {
					if (lane == 0) {
						w_key[w_cnt] = ekey;
						w_seq[w_cnt] = seq;
						w_row[w_cnt] = erow;
					}
					// incremental max: the new entry has the largest seq, so
					// ekey >= fq_key makes it the (key,seq) max
					if (ekey >= fq_key) {
						fq_key = ekey;
						fq_idx = w_cnt;
					}
					w_cnt++;
				} else {
					// new entry has the LARGEST seq: if its key >= max key it
					// would be popped right back (pop_last = latest of the
					// max) -> net no-op; else it replaces the current max
					if (ekey < fq_key) {
						if (lane == 0) {
							w_key[fq_idx] = ekey;
							w_seq[fq_idx] = seq;
							w_row[fq_idx] = erow;
						}
						replaced = true;
					}
				}
				seq++;
				__syncthreads();
				if (replaced)
					wave_max_w(&fq_key, &fq_idx);
			}
		}
	}

	// emit to_vec_limit(k): ascending (key, seq) = (dist, FIFO) (knn.rs:92-104)
	uint32_t out_m = w_cnt < k ? w_cnt : k;
	for (uint32_t slot = 0; slot < out_m; slot++) {
		uint64_t mk = ~0ULL;
		uint32_t ms = ~0u;
		int mi = -1;
		for (uint32_t i = lane; i < w_cnt; i += 64) {
			uint64_t kk = w_key[i];
			uint32_t ss = w_seq[i];
			if (kk < mk || (kk == mk && ss < ms)) {
				mk = kk;
				ms = ss;
				mi = (int)i;
			}
		}
		for (int off = 32; off > 0; off >>= 1) {
			uint64_t ok = __shfl_down(mk, off);
			uint32_t os = __shfl_down(ms, off);
			int oi = __shfl_down(mi, off);
			if (ok < mk || (ok == mk && os < ms)) {
				mk = ok;
				ms = os;
				mi = oi;
			}
		}
		mk = __shfl(mk, 0);
		mi = __shfl(mi, 0);
		if (lane == 0) {
			out_rows[(uint64_t)qid * k + slot] = w_row[mi];
			// decode distance from the total_cmp key (invertible)
			uint64_t bits =
			    (mk >> 63) ? (mk & ~0x8000000000000000ULL) : ~mk;
			out_dists[(uint64_t)qid * k + slot] =
			    __longlong_as_double(bits);
			w_key[mi] = ~0ULL;
			w_seq[mi] = ~0u;
		}
		__syncthreads();
	}
	if (lane == 0) {
		out_cnt[qid] = out_m;
		out_flags[qid] = flags;
	}
}

// Scatter per-chunk adjacency deltas into the padded device graph: upd_ids
// names the dirty nodes, upd_deg their new degrees, upd_edges their new
// edge rows (cnt x stride, host-packed). One thread per slot.
__global__ void k_adj_scatter(const uint32_t *__restrict__ upd_ids,
                              const uint32_t *__restrict__ upd_deg,
                              const uint32_t *__restrict__ upd_edges,
                              uint32_t cnt, uint32_t stride,
                              uint32_t *__restrict__ adj,
                              uint32_t *__restrict__ deg) {
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= (uint64_t)cnt * stride)
		return;
	uint32_t i = (uint32_t)(t / stride);
	uint32_t s = (uint32_t)(t % stride);
	uint32_t node = upd_ids[i];
	if (s == 0)
		deg[node] = upd_deg[i];
	if (s < upd_deg[i])
		adj[(uint64_t)node * stride + s] = upd_edges[t];
}

// ---------------------------------------------------------------------------
// Batched-apply kernels for the GPU snapshot build: the host apply phase is
// RAM-bound on pair distances (select's is_closer + backlink prunes read
// ~100 MB of random rows per insert), so the pair matrices and the
// heuristic select itself run on the device; the host keeps only the
// (cheap, exact) edge bookkeeping. Distances use the restated chain, so a
// host twin with the same batched schedule is bit-identical.
// ---------------------------------------------------------------------------

// One block per list. lists = concatenated [focus, c_0, c_1, ...] row ids
// (loff[i]..loff[i+1]); mats = per-list len^2 f64 distance matrix at
// moff[i] (row-major, M[a][b] = dist(list[a], list[b])).
__global__ __launch_bounds__(256) void k_pair_mats(
    const float *__restrict__ rm, const double *__restrict__ norms,
    uint32_t d, int metric, const uint32_t *__restrict__ lists,
    const uint32_t *__restrict__ loff, const uint64_t *__restrict__ moff,
    double *__restrict__ mats) {
	uint32_t li = blockIdx.x;
	uint32_t o0 = loff[li], o1 = loff[li + 1];
	uint32_t len = o1 - o0;
	double *M = mats + moff[li];
	for (uint32_t p = threadIdx.x; p < len * len; p += 256) {
		uint32_t a = p / len, bb = p % len;
		if (bb < a)
			continue; // symmetric: fill upper, mirror below
		uint32_t ra = lists[o0 + a], rb = lists[o0 + bb];
		const float *va = rm + (uint64_t)ra * d;
		const float *vb = rm + (uint64_t)rb * d;
		double dist;
		if (metric == 0) {
			float pp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			uint32_t k = 0;
			for (; k + 8 <= d; k += 8)
#pragma unroll
				for (uint32_t t = 0; t < 8; t++)
					pp[t] = __fadd_rn(pp[t],
					                  __fmul_rn(va[k + t], vb[k + t]));
			float sum = 0.f;
			sum = __fadd_rn(sum, __fadd_rn(pp[0], pp[4]));
			sum = __fadd_rn(sum, __fadd_rn(pp[1], pp[5]));
			sum = __fadd_rn(sum, __fadd_rn(pp[2], pp[6]));
			sum = __fadd_rn(sum, __fadd_rn(pp[3], pp[7]));
			for (; k < d; k++)
				sum = __fadd_rn(sum, __fmul_rn(va[k], vb[k]));
			dist = 1.0 - (double)sum / (norms[ra] * norms[rb]);
		} else {
			float acc = 0.f;
			for (uint32_t k = 0; k < d; k++) {
				float diff = va[k] - vb[k];
				acc = __fadd_rn(acc, __fmul_rn(diff, diff));
			}
			dist = sqrt((double)acc);
		}
		M[(uint64_t)a * len + bb] = dist;
		if (a != bb)
			M[(uint64_t)bb * len + a] = dist;
	}
}

// Heuristic neighbour select on the device (heuristic.rs:35-116 without
// extend, + keep :92-112; is_closer :193-216): one 64-lane block per list.
// Candidates = list[1..len), keys = M[0][i], popped in (total_cmp key,
// insertion seq) order — reproduced by a stable sort on (key, index).
// out_sel[i][m_max] gets the selected ROW ids, out_cnt[i] the count.
#define HSEL_CAP 640 // 1 + HQ_EF_CAP + headroom; m_max <= 64
__global__ __launch_bounds__(64) void k_heur_select(
    const uint32_t *__restrict__ lists, const uint32_t *__restrict__ loff,
    const uint64_t *__restrict__ moff, const double *__restrict__ mats,
    uint32_t m_max, int keep, uint32_t *__restrict__ out_sel,
    uint32_t *__restrict__ out_cnt) {
	__shared__ uint64_t skey[HSEL_CAP];
	__shared__ uint32_t sidx[HSEL_CAP];
	__shared__ uint32_t res[64];
	__shared__ uint32_t pruned[HSEL_CAP];
	uint32_t li = blockIdx.x;
	uint32_t o0 = loff[li], o1 = loff[li + 1];
	uint32_t len = o1 - o0;
	uint32_t n = len - 1; // candidates
	const double *M = mats + moff[li];
	const int lane = threadIdx.x;
	uint32_t *out = out_sel + (uint64_t)li * m_max;
	for (uint32_t i = lane; i < n; i += 64) {
		skey[i] = d_total_key(M[1 + i]);
		sidx[i] = i;
	}
	__syncthreads();
	// odd-even transposition sort on (key, idx) — stable order == the
	// host PQ's (total_cmp, push seq)
	for (uint32_t phase = 0; phase < n; phase++) {
		uint32_t start = phase & 1;
		for (uint32_t i = start + 2 * lane; i + 1 < n; i += 128) {
			uint64_t k0 = skey[i], k1 = skey[i + 1];
			uint32_t i0 = sidx[i], i1 = sidx[i + 1];
			if (k1 < k0 || (k1 == k0 && i1 < i0)) {
				skey[i] = k1;
				skey[i + 1] = k0;
				sidx[i] = i1;
				sidx[i + 1] = i0;
			}
		}
		__syncthreads();
	}
	if (n <= m_max) {
		for (uint32_t i = lane; i < n; i += 64)
			out[i] = lists[o0 + 1 + sidx[i]];
		if (lane == 0)
			out_cnt[li] = n;
		return;
	}
	// serial heuristic loop; is_closer's res scan is lane-parallel
	__shared__ int res_n, pruned_n, done;
	if (lane == 0) {
		res_n = 0;
		pruned_n = 0;
		done = 0;
	}
	__syncthreads();
	for (uint32_t i = 0; i < n; i++) {
		if (done)
			break;
		uint32_t ci = sidx[i];          // list index - 1
		double ed = M[1 + ci];          // dist(focus, cand)
		// is_closer: fails if ed > dist(cand, res_r) for ANY r
		int bad = 0;
		if (lane < res_n) {
			double dr = M[(uint64_t)(1 + ci) * len + (1 + res[lane])];
			bad = ed > dr;
		}
		uint64_t anybad = __ballot(bad);
		if (lane == 0) {
			if (!anybad) {
				res[res_n++] = ci;
				if ((uint32_t)res_n == m_max)
					done = 1;
			} else if (keep) {
				pruned[pruned_n++] = ci;
			}
		}
		__syncthreads();
	}
	if (keep) {
		__syncthreads();
		if (lane == 0) {
			int nmore = (int)m_max - res_n;
			for (int i = 0; i < nmore && i < pruned_n; i++)
				res[res_n++] = pruned[i];
		}
		__syncthreads();
	}
	for (int i = lane; i < res_n; i += 64)
		out[i] = lists[o0 + 1 + res[i]];
	if (lane == 0)
		out_cnt[li] = (uint32_t)res_n;
}

// ---------------------------------------------------------------------------
// Host-side helpers (restated reference arithmetic for the query's own norm —
// must be bit-identical to oracle orc_sumsq_f32; covered by tests/)
// ---------------------------------------------------------------------------
static float h_sumsq_f32(const float *a, uint32_t d) {
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t i = 0;
	for (; i + 8 <= d; i += 8)
		for (uint32_t j = 0; j < 8; j++)
			p[j] += a[i + j] * a[i + j];
	float acc = 0;
	acc += ((p[0] + p[4]) + (p[1] + p[5]));
	acc += ((p[2] + p[6]) + (p[3] + p[7]));
	for (; i < d; i++)
		acc += a[i] * a[i];
	return acc;
}

// ndarray .mean() = unrolled-8 .sum() / len in f32, then widened (the
// pearson query mean, vector.rs:418-421 via ndarray; same chain as the
// oracle's restatement).
static double h_mean_f32(const float *a, uint32_t d) {
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t i = 0;
	for (; i + 8 <= d; i += 8)
		for (uint32_t j = 0; j < 8; j++)
			p[j] += a[i + j];
	float s = 0;
	s += ((p[0] + p[4]) + (p[1] + p[5]));
	s += ((p[2] + p[6]) + (p[3] + p[7]));
	for (; i < d; i++)
		s += a[i];
	return (double)(s / (float)d);
}

static void free_table(Table &t) {
	if (t.cm)
		(void)hipFree(t.cm);
	if (t.norms)
		(void)hipFree(t.norms);
	if (t.aux)
		(void)hipFree(t.aux);
	if (t.bunc)
		(void)hipFree(t.bunc);
	if (t.ids_dev)
		(void)hipFree(t.ids_dev);
	if (t.sh.codes)
		(void)hipFree(t.sh.codes);
	if (t.sh.side)
		(void)hipFree(t.sh.side);
	t = Table{};
}

// ---------------------------------------------------------------------------
// Device select of the all-distances route
// ---------------------------------------------------------------------------
// The k_eff smallest rows of the all-distances buffer under knn_large_k's own
// order, ascending (total_key(dist), row), found on the device: an MSB-first
// radix select over the 96-bit composite (64-bit total-order key, 32-bit
// row), 8 bits per pass. Composites are distinct, so the walk ends on one
// threshold and the selected set is unique. The kernel boundary is the only
// synchronisation: pass p reads what launches before it wrote, never what a
// block of its own launch writes.

#define SEL_MAX_K 65536u /* larger k keeps the host selection */
#define SEL_PASSES 12    /* 8 key digits, then 4 row digits */
#define SEL_CHUNKS 4     /* 256-row chunks a block loads before counting */
#define SEL_MAX_BLOCKS 2048
// Smallest table the device select serves by default
// (SDBV_SELECT_DEVICE_MIN_ROWS). Measured at 16384, 65536, 262144 and
// 1048576 rows x 768 on manhattan K=10 and cosine K=100: the smallest of them
// at which the device route's p50 last_total_ms beats the host route's by
// more than 10 times the host route's p50-to-p95 gap on both, in both runs
// (profiles/select_device.md; at 16384 the device route is ahead as well,
// but one cosine run missed that margin). Never below 16384.
#define SEL_DEFAULT_MIN_ROWS 65536ull

// The walk's state on entering a pass: the digits chosen so far in the high
// bits of (key, row), zeros below; need = how many of the rows under this
// prefix belong to the result. done: every row under the prefix belongs to
// it; the bits below the prefix are then all ones, (key, row) is the final
// threshold and later passes have nothing to count.
struct SelState {
	uint64_t key;
	uint32_t row;
	uint32_t need;
	uint32_t done;
	uint32_t pad;
};

struct SelHead {
	uint32_t count; // slots the emit handed out
	uint32_t pad;
};

// Device scratch of one select, zeroed by one memset before the first pass;
// the k_eff result slots follow it, so head and results come back in one copy.
struct SelDev {
	uint32_t hist[SEL_PASSES][256];
	SelState st[SEL_PASSES]; // st[p]: state on entering pass p
	SelHead head;
};
static_assert(offsetof(SelDev, head) + sizeof(SelHead) == sizeof(SelDev) &&
                  sizeof(SelDev) % alignof(Cand) == 0,
              "result slots follow the head directly");

// d_total_key for host and device.
__host__ __device__ static inline uint64_t sel_total_key(double x) {
	uint64_t bits;
	__builtin_memcpy(&bits, &x, 8);
	return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
}

// The digit of pass p: passes 0..7 walk the key from its top byte, 8..11 the
// row from its top byte.
__host__ __device__ static inline uint32_t sel_digit(uint64_t key, uint32_t row,
                                                     int pass) {
	return pass < 8 ? (uint32_t)(key >> (56 - 8 * pass)) & 255u
	                : (row >> (24 - 8 * (pass - 8))) & 255u;
}

// Whether the digits above pass p's equal the prefix in s.
__host__ __device__ static inline bool sel_match(uint64_t key, uint32_t row,
                                                 const SelState &s, int pass) {
	if (pass == 0)
		return true;
	if (pass < 8)
		return (key >> (64 - 8 * pass)) == (s.key >> (64 - 8 * pass));
	if (key != s.key)
		return false;
	if (pass == 8)
		return true;
	const int sh = 32 - 8 * (pass - 8);
	return (row >> sh) == (s.row >> sh);
}

// Set the digits of passes from..11 to all ones.
__host__ __device__ static inline void sel_fill(SelState *s, int from) {
	if (from < 8) {
		const int bits = 64 - 8 * from;
		s->key |= bits == 64 ? ~0ULL : (1ULL << bits) - 1;
		s->row = ~0u;
	} else if (from < SEL_PASSES) {
		const int bits = 32 - 8 * (from - 8);
		s->row |= bits == 32 ? ~0u : (1u << bits) - 1;
	}
}

// One step of the walk, shared by the kernels and sdbv_select_topk: hist is
// pass p's histogram over the rows under s's prefix. The digit chosen is the
// first whose running count reaches need; the rows of smaller digits all
// belong to the result and leave need. When the chosen bin holds exactly the
// rows still needed the walk is done. A histogram that cannot reach need (the
// caller's k_eff exceeds the rows it counted) selects everything under the
// prefix; the caller's slot count then shows the mismatch. No early exit from
// the loop: the loads batch.
__host__ __device__ static inline void sel_step(const uint32_t *hist, int pass,
                                                SelState *s) {
	if (s->done)
		return;
	uint32_t digit = 256, before = 0, acc = 0;
	for (uint32_t b = 0; b < 256; b++) {
		const uint32_t c = hist[b];
		const bool hit = digit == 256 && c != 0 && acc + c >= s->need;
		digit = hit ? b : digit;
		before = hit ? acc : before;
		acc += c;
	}
	if (digit == 256) {
		sel_fill(s, pass);
		s->done = 1;
		return;
	}
	s->need -= before;
	if (pass < 8)
		s->key |= (uint64_t)digit << (56 - 8 * pass);
	else
		s->row |= digit << (24 - 8 * (pass - 8));
	if (hist[digit] == s->need) {
		sel_fill(s, pass + 1);
		s->done = 1;
	}
}

// (key, row) at or below the final threshold.
__host__ __device__ static inline bool sel_below(uint64_t key, uint32_t row,
                                                 const SelState &s) {
	return key < s.key || (key == s.key && row <= s.row);
}

// Head of every select kernel: the state on entering `pass` (SEL_PASSES = the
// emit), stepped by one thread from the previous pass's finished histogram
// and state; every block computes the same, block 0 records it for the next
// launch. h is the block's 256-bin LDS histogram, left zeroed.
__device__ static inline SelState sel_enter(SelDev *dev, int pass,
                                            uint32_t k_eff, uint32_t *h,
                                            SelState *st) {
	const uint32_t tid = threadIdx.x;
	if (pass == 0) {
		if (tid == 0)
			*st = SelState{0, 0, k_eff, 0, 0};
	} else {
		h[tid] = dev->hist[pass - 1][tid];
		__syncthreads();
		if (tid == 0) {
			SelState s = dev->st[pass - 1];
			sel_step(h, pass - 1, &s);
			*st = s;
		}
	}
	__syncthreads();
	if (tid == 0 && blockIdx.x == 0 && pass < SEL_PASSES)
		dev->st[pass] = *st;
	h[tid] = 0;
	__syncthreads();
	return *st;
}

// One histogram pass: count pass's digit over the rows below n that the
// bitmap allows and whose higher digits equal the prefix. Per-block LDS
// histogram, flushed once. On a hamming or jaccard table nearly all rows
// share their upper digits, so a wave first tests whether its active lanes
// carry one digit and then adds their number with one LDS atomic.
template <bool MASKED>
__global__ void __launch_bounds__(THREADS)
k_sel_hist(const double *__restrict__ dists, uint64_t n,
           const uint64_t *__restrict__ mask, SelDev *dev, int pass,
           uint32_t k_eff) {
	__shared__ uint32_t h[256];
	__shared__ SelState st;
	const SelState s = sel_enter(dev, pass, k_eff, h, &st);
	if (s.done)
		return;
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint64_t span = (uint64_t)THREADS * SEL_CHUNKS;
	for (uint64_t base = (uint64_t)blockIdx.x * span; base < n;
	     base += (uint64_t)gridDim.x * span) {
		double v[SEL_CHUNKS];
#pragma unroll
		for (int u = 0; u < SEL_CHUNKS; u++) {
			const uint64_t r = base + (uint64_t)u * THREADS + tid;
			v[u] = r < n ? dists[r] : 0.0;
		}
#pragma unroll
		for (int u = 0; u < SEL_CHUNKS; u++) {
			const uint64_t r = base + (uint64_t)u * THREADS + tid;
			bool act = r < n;
			if (MASKED && act)
				act = (mask[r >> 6] >> (r & 63)) & 1ULL;
			const uint64_t key = sel_total_key(v[u]);
			act = act && sel_match(key, (uint32_t)r, s, pass);
			const uint32_t dg = sel_digit(key, (uint32_t)r, pass);
			const unsigned long long m = __ballot(act);
			if (m) {
				const int first = __ffsll(m) - 1;
				const uint32_t d0 = (uint32_t)__shfl((int)dg, first);
				if (__ballot(act && dg == d0) == m) {
					if ((int)lane == first)
						atomicAdd(&h[d0], (uint32_t)__popcll(m));
				} else if (act) {
					atomicAdd(&h[dg], 1u);
				}
			}
		}
	}
	__syncthreads();
	if (h[tid])
		atomicAdd(&dev->hist[pass][tid], h[tid]);
}

// Emit: every considered row at or below the threshold goes to a result slot,
// one counter add per wave. A slot at or past k_eff is counted, never
// written; the host compares the count with k_eff.
template <bool MASKED>
__global__ void __launch_bounds__(THREADS)
k_sel_emit(const double *__restrict__ dists, uint64_t n,
           const uint64_t *__restrict__ mask,
           const uint64_t *__restrict__ ids, SelDev *dev, Cand *out,
           uint32_t k_eff) {
	__shared__ uint32_t h[256];
	__shared__ SelState st;
	const SelState s = sel_enter(dev, SEL_PASSES, k_eff, h, &st);
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	for (uint64_t base = (uint64_t)blockIdx.x * THREADS; base < n;
	     base += (uint64_t)gridDim.x * THREADS) {
		const uint64_t r = base + tid;
		bool sel = r < n;
		if (MASKED && sel)
			sel = (mask[r >> 6] >> (r & 63)) & 1ULL;
		const double v = r < n ? dists[r] : 0.0;
		sel = sel && sel_below(sel_total_key(v), (uint32_t)r, s);
		const unsigned long long m = __ballot(sel);
		if (m) {
			const int first = __ffsll(m) - 1;
			uint32_t slot0 = 0;
			if ((int)lane == first)
				slot0 = atomicAdd(&dev->head.count, (uint32_t)__popcll(m));
			slot0 = (uint32_t)__shfl((int)slot0, first);
			const uint32_t slot =
			    slot0 + (uint32_t)__popcll(m & ((1ULL << lane) - 1));
			if (sel && slot < k_eff)
				out[slot] = Cand{v, ids[r]};
		}
	}
}

// ---------------------------------------------------------------------------
// C-ABI implementation
// ---------------------------------------------------------------------------
extern "C" {

int sdbv_init(int device, sdbv_ctx **out) {
	auto *ctx = new sdbv_ctx();
	if (device >= 0) {
		if (hipSetDevice(device) != hipSuccess) {
			delete ctx;
			return SDBV_ERR_HIP;
		}
		ctx->device = device;
	} else {
		(void)hipGetDevice(&ctx->device);
	}
	if (hipStreamCreate(&ctx->stream) != hipSuccess) {
		delete ctx;
		return SDBV_ERR_HIP;
	}
	(void)hipEventCreate(&ctx->ev0);
	(void)hipEventCreate(&ctx->ev1);
	(void)hipEventCreate(&ctx->ev2);
	(void)hipEventCreate(&ctx->ev3);
	(void)hipEventCreate(&ctx->ev4);
	*out = ctx;
	return SDBV_OK;
}

void sdbv_shutdown(sdbv_ctx *ctx) {
	if (!ctx)
		return;
	for (auto &kv : ctx->tables)
		free_table(kv.second);
	if (ctx->block_out)
		(void)hipFree(ctx->block_out);
	if (ctx->final_out)
		(void)hipFree(ctx->final_out);
	if (ctx->merge_tmp)
		(void)hipFree(ctx->merge_tmp);
	if (ctx->q_dev)
		(void)hipFree(ctx->q_dev);
	for (void *p : {(void *)ctx->pf_scores, (void *)ctx->pf_rows,
	                ctx->pf_cands, ctx->pf_res, (void *)ctx->pf4_list,
	                ctx->pf4_thr})
		if (p)
			(void)hipFree(p);
	for (void *p : {(void *)ctx->S, ctx->bstate, (void *)ctx->Q_dev,
	                (void *)ctx->qnorms, (void *)ctx->bdists,
	                (void *)ctx->btheta, (void *)ctx->bcand,
	                (void *)ctx->bcand_cnt})
		if (p)
			(void)hipFree(p);
	for (void *p : {(void *)ctx->flt_mask, (void *)ctx->flt_rows,
	                ctx->flt_cands})
		if (p)
			(void)hipFree(p);
	if (ctx->flt_mask_pin)
		(void)hipHostFree(ctx->flt_mask_pin);
	if (ctx->flt_rows_pin)
		(void)hipHostFree(ctx->flt_rows_pin);
	if (ctx->sel_dists)
		(void)hipFree(ctx->sel_dists);
	if (ctx->sel_dev)
		(void)hipFree(ctx->sel_dev);
	if (ctx->sel_pin)
		(void)hipHostFree(ctx->sel_pin);
	if (ctx->app_buf)
		(void)hipFree(ctx->app_buf);
	if (ctx->blas)
		(void)rocblas_destroy_handle(ctx->blas);
	(void)hipEventDestroy(ctx->ev0);
	(void)hipEventDestroy(ctx->ev1);
	(void)hipEventDestroy(ctx->ev2);
	(void)hipEventDestroy(ctx->ev3);
	(void)hipEventDestroy(ctx->ev4);
	(void)hipStreamDestroy(ctx->stream);
	delete ctx;
}

const char *sdbv_last_error(sdbv_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int sdbv_get_stats(sdbv_ctx *ctx, sdbv_stats *out) {
	if (!ctx || !out)
		return SDBV_ERR_BAD_ARG;
	*out = ctx->stats;
	return SDBV_OK;
}

static int stage_common(sdbv_ctx *ctx, uint64_t table, uint64_t n, uint32_t d,
                        uint8_t metric, Table **out) {
	if (d == 0 || d > MAX_D || (d % 4) != 0)
		return SDBV_ERR_BAD_ARG; // float4 path needs d%4==0 in this revision
	if (metric > SDBV_METRIC_PEARSON)
		return SDBV_ERR_UNSUPPORTED;
	if (metric == SDBV_METRIC_JACCARD && d > 1024)
		return SDBV_ERR_UNSUPPORTED; // LDS set capacity (JACC_SLOTS)
	auto it = ctx->tables.find(table);
	if (it != ctx->tables.end()) {
		free_table(it->second);
		ctx->tables.erase(it);
	}
	Table t;
	t.n = n;
	t.n_pad = ((n + TILE - 1) / TILE) * TILE;
	t.d = d;
	t.metric = metric;
	uint64_t cm_bytes = (uint64_t)d * t.n_pad * sizeof(float);
	HIP_CHECK(ctx, hipMalloc(&t.cm, cm_bytes));
	t.bytes = cm_bytes;
	if (metric == SDBV_METRIC_COSINE) {
		HIP_CHECK(ctx, hipMalloc(&t.norms, t.n_pad * sizeof(double)));
		t.bytes += t.n_pad * sizeof(double);
	}
	HIP_CHECK(ctx, hipMalloc(&t.ids_dev, t.n_pad * sizeof(uint64_t)));
	t.bytes += t.n_pad * sizeof(uint64_t);
	ctx->tables[table] = t;
	*out = &ctx->tables[table];
	return SDBV_OK;
}

static void refresh_bytes_staged(sdbv_ctx *ctx) {
	uint64_t total = 0;
	for (auto &kv : ctx->tables)
		total += kv.second.bytes;
	ctx->stats.bytes_staged = total;
}

static void free_shadow(sdbv_ctx *ctx, Table *t) {
	if (t->sh.codes)
		(void)hipFree(t->sh.codes);
	if (t->sh.side)
		(void)hipFree(t->sh.side);
	t->bytes -= t->sh.bytes;
	t->sh = Shadow{};
	refresh_bytes_staged(ctx);
}

// What the three shadow tiers differ in, by Shadow::kind: the rows of one
// block-sweep of the tier's prefilter kernel (sn_pad is a multiple of it),
// the f32-sized side values per row, and (below) the code bytes. Entry 4 is
// the int6 tier's H-only stream, for prefilter_grid alone: its spans are
// whole sweeps of THREADS rows, not whole tiles, which left a fifth of the
// device's 8 blocks per CU empty at 10M rows (profiles/prefilter_h4.md).
// Entry 5 is the euclidean int8 tier.
struct ShadowTier {
	uint64_t tile;
	uint64_t side_per_row;
};
static const ShadowTier SHADOW_TIERS[6] = {
    {0, 0},        {PF_TILE, 1}, {PF8_TILE, 2},
    {PF6_TILE, 3}, {THREADS, 0}, {PF8_TILE, 3}};

// bf16: 2 d bytes per row (+50 % of the f32 store); int8 and l2: d (+25 %);
// int6: 0.75 d_pad, d_pad = d rounded up to a multiple of 32 (planes H and
// L).
static uint64_t shadow_code_bytes(int kind, uint32_t d, uint64_t sn_pad) {
	switch (kind) {
	case 1: return 2ull * d * sn_pad;
	case 2:
	case 5: return (uint64_t)d * sn_pad;
	default: return 24ull * ((d + 31) / 32) * sn_pad;
	}
}

// Build the kind shadow of a staged table (cosine: kinds 1..3, norms already
// computed, in stream order; euclidean: kind 5), instead of any other kind
// the table holds. A failed allocation leaves the table without a shadow and
// returns SDBV_ERR_OOM.
// h4 (int6 only): with the H-only side data, 8 B per row more. Staging asks
// for it when h4_policy holds; the explicit entries build the plain shadow,
// also in place of a staged one that carries the side data.
// The builder of t->sh over nb 256-row blocks in one launch: those from row0
// on (blist null), or the blocks blist[0..nb) on the device, ascending and
// distinct (sdbv_update_rows).
static void launch_shadow_blocks(sdbv_ctx *ctx, Table *t, uint64_t n,
                                 uint64_t row0, uint64_t nb,
                                 const uint32_t *blist) {
	const Shadow &sh = t->sh;
	const uint64_t sn_pad = sh.sn_pad;
	if (nb == 0)
		return;
	switch (sh.kind) {
	case 1: { // one lane per PF_ROWS_PER_LANE rows
		uint64_t groups = nb * (256 / PF_ROWS_PER_LANE);
		hipLaunchKernelGGL(k_shadow, dim3((uint32_t)((groups + 255) / 256)),
		                   dim3(256), 0, ctx->stream, t->cm, t->norms,
		                   (uint16_t *)sh.codes, sh.pinv(), n, t->n_pad,
		                   sn_pad, t->d, row0, blist, (uint32_t)nb);
		break;
	}
	case 2: // one lane per row
		hipLaunchKernelGGL(k_shadow_i8, dim3((uint32_t)nb), dim3(256), 0,
		                   ctx->stream, t->cm, t->norms, (uint8_t *)sh.codes,
		                   sh.pscale(), sh.peps(), n, t->n_pad, sn_pad, t->d,
		                   row0, blist);
		break;
	case 3:
		hipLaunchKernelGGL(k_shadow_i6, dim3((uint32_t)nb), dim3(256), 0,
		                   ctx->stream, t->cm, t->norms, sh.plane_h(),
		                   sh.plane_l(t->d), sh.pscale(), sh.peps(), sh.xsum(),
		                   sh.peps4(), sh.xsum_h(), n, t->n_pad, sn_pad, t->d,
		                   row0, blist);
		break;
	case 5: // one lane per row
		hipLaunchKernelGGL(k_shadow_l2, dim3((uint32_t)nb), dim3(256), 0,
		                   ctx->stream, t->cm, (uint8_t *)sh.codes,
		                   sh.pscale(), sh.l2_xx(), sh.l2_res(), n, t->n_pad,
		                   sn_pad, t->d, row0, blist);
		break;
	}
}

// Launch the shadow builder of t->sh over rows [row0, row_end), both
// multiples of 256 with row_end <= sn_pad (the bf16 builder's last block may
// run on to sn_pad, its own guard): the whole shadow when staging or growth
// builds it, the 256-row blocks around the new rows after an in-place append.
// A builder writes row r from cm alone, so writing a row again is idempotent.
// n = the table's row count as the builders shall see it: an append passes
// the count it is about to commit.
static void launch_shadow_rows(sdbv_ctx *ctx, Table *t, uint64_t n,
                               uint64_t row0, uint64_t row_end) {
	launch_shadow_blocks(ctx, t, n, row0, (row_end - row0) / 256, nullptr);
}

static int build_shadow(sdbv_ctx *ctx, Table *t, int kind, bool h4 = false) {
	if (t->metric !=
	    (kind == 5 ? SDBV_METRIC_EUCLIDEAN : SDBV_METRIC_COSINE))
		return SDBV_ERR_UNSUPPORTED;
	h4 = h4 && kind == 3;
	if (t->sh.kind == kind && t->sh.h4 == h4)
		return SDBV_OK;
	if (t->sh.kind)
		free_shadow(ctx, t);
	const ShadowTier &tier = SHADOW_TIERS[kind];
	Shadow sh;
	sh.h4 = h4;
	// from the capacity, not from n: appended rows need their shadow cells.
	// For a table as staged, n_pad = roundup(n, TILE) and every tier's tile is
	// a multiple of TILE, so this is roundup(n, tile) as before; a grown
	// capacity is a multiple of every tile, so sn_pad == n_pad.
	sh.sn_pad = ((t->n_pad + tier.tile - 1) / tier.tile) * tier.tile;
	if (sh.sn_pad == 0)
		sh.sn_pad = tier.tile;
	const uint64_t code_bytes = shadow_code_bytes(kind, t->d, sh.sn_pad);
	const uint64_t side_bytes =
	    (tier.side_per_row + (sh.h4 ? 2 : 0)) * sh.sn_pad * sizeof(float);
	if (hipMalloc(&sh.codes, code_bytes) != hipSuccess ||
	    hipMalloc(&sh.side, side_bytes) != hipSuccess) {
		(void)hipGetLastError(); // allocation failure is not sticky
		if (sh.codes)
			(void)hipFree(sh.codes);
		return SDBV_ERR_OOM;
	}
	sh.kind = kind;
	sh.bytes = code_bytes + side_bytes;
	t->sh = sh;
	t->bytes += sh.bytes;
	launch_shadow_rows(ctx, t, t->n, 0, sh.sn_pad);
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	refresh_bytes_staged(ctx);
	return SDBV_OK;
}

// Default minimum row counts of the staging policy, one measured crossover
// per tier: a shadow at all, below which the extra launches of the prefilter
// path cost more than the halved stream saves (profiles/prefilter_scan.md);
// int8 rather than bf16 (profiles/prefilter_i8.md); int6 rather than int8
// (profiles/prefilter_i6.md). The last two are never below the first.
#define PF_DEFAULT_MIN_ROWS 500000ull
#define PF8_DEFAULT_MIN_ROWS 500000ull
#define PF6_DEFAULT_MIN_ROWS 500000ull
// The two-stage int6 path rather than the plain one: a tie at 500 000 rows,
// ahead from 1 000 000 (profiles/prefilter_h4.md); never below
// PF6_DEFAULT_MIN_ROWS.
#define PF4_DEFAULT_MIN_ROWS 1000000ull
// The euclidean tier's shadow at all: measured against the exact scan at
// 200 000 (a tie), 500 000, 1 000 000 and 2 000 000 rows; 500 000 is the
// smallest of them at which the shadow path wins by more than 10 times the
// spread (profiles/prefilter_l2.md).
#define PFL2_DEFAULT_MIN_ROWS 500000ull

// One staging policy question: env_flag=0 answers no; otherwise the table
// needs env_min_rows rows (default default_min). The three row counts are
// independent of each other.
static bool shadow_policy(const Table *t, const char *env_flag,
                          const char *env_min_rows, uint64_t default_min) {
	const char *e = getenv(env_flag);
	if (e && e[0] == '0' && e[1] == 0)
		return false;
	uint64_t min_rows = default_min;
	const char *m = getenv(env_min_rows);
	if (m && *m)
		min_rows = strtoull(m, nullptr, 10);
	return t->n >= min_rows;
}

// The two-stage path's question, asked when staging builds an int6 shadow
// (for its side data) and again at every call: SDBV_SCAN_PREFILTER_H4 and
// SDBV_SCAN_PREFILTER_H4_MIN_ROWS.
static bool h4_policy(const Table *t) {
	return shadow_policy(t, "SDBV_SCAN_PREFILTER_H4",
	                     "SDBV_SCAN_PREFILTER_H4_MIN_ROWS",
	                     PF4_DEFAULT_MIN_ROWS);
}

// The shadow that scan staging builds. Euclidean: the l2 tier when
// SDBV_SCAN_PREFILTER_L2 / SDBV_SCAN_PREFILTER_L2_MIN_ROWS say yes, a pair of
// its own (the cosine variables give a euclidean table nothing). Cosine: none
// when SDBV_SCAN_PREFILTER says no; else bf16 when SDBV_SCAN_PREFILTER_I8
// says no; else int8 when SDBV_SCAN_PREFILTER_I6 says no; else int6. Any
// other metric: none.
static int staged_shadow_kind(const Table *t) {
	if (t->metric == SDBV_METRIC_EUCLIDEAN)
		return shadow_policy(t, "SDBV_SCAN_PREFILTER_L2",
		                     "SDBV_SCAN_PREFILTER_L2_MIN_ROWS",
		                     PFL2_DEFAULT_MIN_ROWS)
		           ? 5
		           : 0;
	if (t->metric != SDBV_METRIC_COSINE ||
	    !shadow_policy(t, "SDBV_SCAN_PREFILTER", "SDBV_SCAN_PREFILTER_MIN_ROWS",
	                   PF_DEFAULT_MIN_ROWS))
		return 0;
	if (!shadow_policy(t, "SDBV_SCAN_PREFILTER_I8",
	                   "SDBV_SCAN_PREFILTER_I8_MIN_ROWS", PF8_DEFAULT_MIN_ROWS))
		return 1;
	if (!shadow_policy(t, "SDBV_SCAN_PREFILTER_I6",
	                   "SDBV_SCAN_PREFILTER_I6_MIN_ROWS", PF6_DEFAULT_MIN_ROWS))
		return 2;
	return 3;
}

static int finish_stage(sdbv_ctx *ctx, Table *t, bool scan_table) {
	uint64_t nb = (t->n + THREADS - 1) / THREADS;
	BatchAuxHdr *hdr = nullptr;
	if (t->metric == SDBV_METRIC_COSINE) {
		hipLaunchKernelGGL(k_norms, dim3((uint32_t)nb), dim3(THREADS), 0,
		                   ctx->stream, t->cm, t->norms, t->n, t->n_pad, t->d);
	}
	if (t->metric <= SDBV_METRIC_EUCLIDEAN) {
		// batch-path selection aux (cosine 1/norm, euclidean sumsq), the rows
		// without a usable key and the largest norm of the others; the
		// other metrics take the all-distances route and need none
		HIP_CHECK(ctx, hipMalloc(&t->aux, t->n_pad * sizeof(float)));
		t->bytes += t->n_pad * sizeof(float);
		const uint64_t unc_bytes =
		    BATCH_UNC_CAP * sizeof(uint32_t) + sizeof(BatchAuxHdr);
		// (a fixed 4 KiB, left out of the per-row byte count)
		HIP_CHECK(ctx, hipMalloc(&t->bunc, unc_bytes));
		hdr = (BatchAuxHdr *)(t->bunc + BATCH_UNC_CAP);
		HIP_CHECK(ctx, hipMemsetAsync(hdr, 0, sizeof(BatchAuxHdr), ctx->stream));
		hipLaunchKernelGGL(k_aux, dim3((uint32_t)nb), dim3(THREADS), 0,
		                   ctx->stream, t->cm, t->norms, t->aux, t->n,
		                   t->n_pad, t->d, (int)t->metric, t->bunc, hdr);
	}
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	if (hdr) {
		BatchAuxHdr h;
		HIP_CHECK(ctx, hipMemcpy(&h, hdr, sizeof(h), hipMemcpyDeviceToHost));
		t->bunc_n = h.n_unc;
		std::memcpy(&t->bmax_norm, &h.max_norm_bits, sizeof(double));
	}
	refresh_bytes_staged(ctx);
	// a table staged for scanning gets the prefilter shadow when the policy
	// asks for one; without the memory for it the table simply has none
	const int kind = scan_table ? staged_shadow_kind(t) : 0;
	if (kind) {
		int rc = build_shadow(ctx, t, kind, kind == 3 && h4_policy(t));
		if (rc != SDBV_OK && rc != SDBV_ERR_OOM)
			return rc;
	}
	return SDBV_OK;
}

// Internal staging entry. scan_table = false stages for graph search
// (sdbv_hnsw_finalize): such a table is never scanned per query, so it never
// pays the shadow's +50 % HBM.
static int stage_corpus_impl(sdbv_ctx *ctx, uint64_t table, const float *rows,
                             const uint64_t *ids, uint64_t n, uint32_t d,
                             uint8_t metric, bool scan_table) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	// tie-break contract: ids must be strictly increasing (see include/sdbv.h)
	if (ids)
		for (uint64_t i = 1; i < n; i++)
			if (ids[i] <= ids[i - 1])
				return SDBV_ERR_IDS_UNSORTED;
	Table *t = nullptr;
	int rc = stage_common(ctx, table, n, d, metric, &t);
	if (rc != SDBV_OK)
		return rc;
	t->scan_table = scan_table;
	t->last_id = n ? (ids ? ids[n - 1] : n - 1) : 0;
	// upload row-major then transpose on device
	float *rm = nullptr;
	HIP_CHECK(ctx, hipMalloc(&rm, n * (uint64_t)d * sizeof(float)));
	HIP_CHECK(ctx, hipMemcpyAsync(rm, rows, n * (uint64_t)d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	dim3 grid((uint32_t)((t->n_pad + 31) / 32), (d + 31) / 32);
	hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, ctx->stream, rm, t->cm,
	                   n, t->n_pad, d);
	if (ids) {
		HIP_CHECK(ctx, hipMemcpyAsync(t->ids_dev, ids, n * sizeof(uint64_t),
		                              hipMemcpyHostToDevice, ctx->stream));
	} else {
		uint64_t nb = (t->n_pad + THREADS - 1) / THREADS;
		hipLaunchKernelGGL(k_fill_ids, dim3((uint32_t)nb), dim3(THREADS), 0,
		                   ctx->stream, t->ids_dev, t->n_pad, 0);
	}
	int rc2 = finish_stage(ctx, t, scan_table);
	(void)hipFree(rm);
	return rc2;
}

int sdbv_stage_corpus(sdbv_ctx *ctx, uint64_t table, const float *rows,
                      const uint64_t *ids, uint64_t n, uint32_t d,
                      uint8_t metric) {
	return stage_corpus_impl(ctx, table, rows, ids, n, d, metric, true);
}

int sdbv_table_set_prefilter(sdbv_ctx *ctx, uint64_t table, int on) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table *t = &it->second;
	if (t->metric != SDBV_METRIC_COSINE)
		return SDBV_ERR_UNSUPPORTED;
	if (on)
		return build_shadow(ctx, t, 1);
	if (t->sh.kind)
		free_shadow(ctx, t);
	return SDBV_OK;
}

// sdbv_table_set_prefilter_kind(.., 2) and sdbv_table_set_prefilter_i6.
static int set_shadow_kind(sdbv_ctx *ctx, uint64_t table, int kind) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	return build_shadow(ctx, &it->second, kind);
}

int sdbv_table_set_prefilter_kind(sdbv_ctx *ctx, uint64_t table, int kind) {
	if (kind < 0 || kind > 2)
		return SDBV_ERR_BAD_ARG;
	if (kind < 2)
		return sdbv_table_set_prefilter(ctx, table, kind);
	return set_shadow_kind(ctx, table, 2);
}

// The int6 shadow has an entry of its own: sdbv_table_set_prefilter_kind
// keeps rejecting every kind above 2, as its callers rely on.
int sdbv_table_set_prefilter_i6(sdbv_ctx *ctx, uint64_t table) {
	return set_shadow_kind(ctx, table, 3);
}

// The euclidean tier's entry: the three above keep refusing a euclidean
// table, this one refuses every other metric.
int sdbv_table_set_prefilter_l2(sdbv_ctx *ctx, uint64_t table, int on) {
	if (on)
		return set_shadow_kind(ctx, table, 5);
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table *t = &it->second;
	if (t->metric != SDBV_METRIC_EUCLIDEAN)
		return SDBV_ERR_UNSUPPORTED;
	if (t->sh.kind)
		free_shadow(ctx, t);
	return SDBV_OK;
}

float sdbv_prefilter_eps(uint32_t d) { return pf_eps(d); }

// Proven bound on |key - E| of the batch path: key is the
// f32 selection key of a row under ANY summation order of the two f32 dot
// products, E the row's exact distance mapped into the key's domain in f64,
//   cosine:    key = -(s * f32(1 / norm)),  E = -(1 - dist) * q_norm
//   euclidean: key = sumsq - 2 s,           E = dist^2 - q_norm^2
// with gamma(m) = m u / (1 - m u), u = 2^-24. Holds for rows and queries with
// norms in [PF_NORM_MIN, PF_NORM_MAX] (euclidean: at most PF_NORM_MAX);
// max_row_norm is the largest such row norm of the table (euclidean only).
double sdbv_batch_key_bound(uint8_t metric, uint32_t d, double q_norm,
                            double max_row_norm) {
	const double u = 0x1p-24;
	auto gamma = [u](double m) { return m * u / (1.0 - m * u); };
	if (metric == SDBV_METRIC_COSINE)
		return 1.01 * (2.0 * gamma(d + 1.0) + 3.0 * u) * q_norm;
	const double w = (max_row_norm + q_norm) * (max_row_norm + q_norm);
	return 1.01 * (3.0 * gamma(d + 2.0) + 2.0 * u) * w + 4.0 * d * 0x1p-149;
}

int sdbv_prefilter_i8_row(const float *x, uint32_t d, double norm,
                          int8_t *codes, float *scale, float *eps) {
	if (!x || !codes || !scale || !eps || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	uint8_t stored[MAX_D];
	float pscale;
	pf_i8_row(x, 1, d, norm, stored, 1, scale, &pscale, eps);
	for (uint32_t k = 0; k < d; k++)
		codes[k] = (int8_t)((int)stored[k] - 128);
	return SDBV_OK;
}

int sdbv_prefilter_l2_row(const float *x, uint32_t d, int8_t *codes,
                          float *scale, float *xx, float *res) {
	if (!x || !codes || !scale || !xx || !res || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	uint8_t stored[MAX_D];
	pf_l2_row(x, 1, d, stored, 1, scale, xx, res);
	for (uint32_t k = 0; k < d; k++)
		codes[k] = (int8_t)((int)stored[k] - 128);
	return SDBV_OK;
}

// One row of k_prefilter_i8<., true>: the same FMA chain over the stored
// bytes, the same pf_l2_finish. *lo = -inf and *up = +inf for a row without
// a bound (scale NaN); SDBV_ERR_UNSUPPORTED for a query outside the window.
int sdbv_prefilter_l2_interval(const float *q, uint32_t d, const int8_t *codes,
                               float scale, float xx, float res, float *lo,
                               float *up) {
	if (!q || !codes || !lo || !up || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	PfL2Q qc;
	if (!pf_l2_query(q, d, &qc))
		return SDBV_ERR_UNSUPPORTED;
	float t = 0.f;
	for (uint32_t k = 0; k < d; k++)
		t = fmaf((float)((int)codes[k] + 128), q[k], t);
	const float a2 = pf_l2_finish(t, scale, xx, res, qc, lo, up);
	if ((__builtin_bit_cast(uint32_t, a2) & 0x7F800000u) == 0x7F800000u) {
		*lo = -__builtin_inff();
		*up = __builtin_inff();
	}
	return SDBV_OK;
}

int sdbv_prefilter_i6_row(const float *x, uint32_t d, double norm,
                          int8_t *codes, float *scale, float *eps,
                          uint32_t *xsum) {
	if (!x || !codes || !scale || !eps || !xsum || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	uint32_t h[MAX_D / 32 * 4], l[MAX_D / 32 * 2];
	float pscale;
	pf_i6_row(x, 1, d, norm, h, 4, l, 2, scale, &pscale, eps, xsum);
	for (uint32_t k = 0; k < d; k++) {
		const uint32_t g = k / 32, i = k % 32, f = i & 15;
		const uint32_t hi = (h[g * 4 + (i >> 3)] >> (4 * (i & 7))) & 15u;
		const uint32_t lo =
		    (l[g * 2 + (i >> 4)] >> (2 * (f < 8 ? 2 * f : 2 * (f - 8) + 1))) &
		    3u;
		codes[k] = (int8_t)((int)(hi * 4 + lo) - 32);
	}
	return SDBV_OK;
}

int sdbv_prefilter_h4_row(const float *x, uint32_t d, double norm,
                          uint8_t *codes_h, float *scale, float *eps4,
                          uint32_t *xsum_h) {
	if (!x || !codes_h || !scale || !eps4 || !xsum_h || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	uint32_t h[MAX_D / 32 * 4], l[MAX_D / 32 * 2], xsum;
	float pscale, eps;
	pf_i6_row(x, 1, d, norm, h, 4, l, 2, scale, &pscale, &eps, &xsum, eps4,
	          xsum_h);
	for (uint32_t k = 0; k < d; k++) {
		const uint32_t g = k / 32, i = k % 32;
		codes_h[k] = (uint8_t)((h[g * 4 + (i >> 3)] >> (4 * (i & 7))) & 15u);
	}
	return SDBV_OK;
}

int sdbv_prefilter_q12(const float *q, uint32_t d, int16_t *codes, float *sq,
                       float *rho_q, uint32_t *qs) {
	if (!q || !codes || !sq || !rho_q || !qs || d == 0 || d > MAX_D)
		return SDBV_ERR_BAD_ARG;
	const double q_norm = sqrt((double)h_sumsq_f32(q, d));
	if (!(q_norm >= PF_NORM_MIN && q_norm <= PF_NORM_MAX)) {
		// the prefilter never runs for such a query
		for (uint32_t k = 0; k < d; k++)
			codes[k] = 0;
		*sq = __builtin_bit_cast(float, 0x7FC00000u);
		*rho_q = 0.f;
		*qs = 2048u * 32u * ((d + 31) / 32);
		return SDBV_OK;
	}
	pf_q12(q, d, q_norm, nullptr, codes, sq, rho_q, qs);
	return SDBV_OK;
}

float sdbv_bf16_rne(float x) {
	uint32_t u;
	std::memcpy(&u, &x, 4);
	if ((u & 0x7F800000u) == 0x7F800000u)
		return x; // inf and NaN pass through
	u = pf_bf16_bits(u) << 16;
	std::memcpy(&x, &u, 4);
	return x;
}

int sdbv_stage_synthetic(sdbv_ctx *ctx, uint64_t table, uint64_t n, uint32_t d,
                         uint8_t metric, uint64_t seed, uint64_t row_offset,
                         uint64_t id_base) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	Table *t = nullptr;
	int rc = stage_common(ctx, table, n, d, metric, &t);
	if (rc != SDBV_OK)
		return rc;
	t->last_id = n ? id_base + n - 1 : 0;
	hipLaunchKernelGGL(k_gen_cm, dim3(8192), dim3(256), 0, ctx->stream, t->cm,
	                   t->n, t->n_pad, t->d, seed, row_offset);
	uint64_t nb = (t->n_pad + THREADS - 1) / THREADS;
	hipLaunchKernelGGL(k_fill_ids, dim3((uint32_t)nb), dim3(THREADS), 0,
	                   ctx->stream, t->ids_dev, t->n_pad, id_base);
	return finish_stage(ctx, t, true);
}

uint64_t sdbv_table_rows(sdbv_ctx *ctx, uint64_t table) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	return it == ctx->tables.end() ? 0 : it->second.n;
}

int sdbv_drop_table(sdbv_ctx *ctx, uint64_t table) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	free_table(it->second);
	ctx->tables.erase(it);
	refresh_bytes_staged(ctx);
	return SDBV_OK;
}

int sdbv_table_set_order(sdbv_ctx *ctx, uint64_t table, double order) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	it->second.order = order;
	return SDBV_OK;
}

static int ensure_query_scratch(sdbv_ctx *ctx, uint32_t d, uint64_t nblocks,
                                uint32_t k) {
	if (ctx->q_cap < d) {
		if (ctx->q_dev)
			(void)hipFree(ctx->q_dev);
		// the query, then the int6 tier's digit words (one H2D copy)
		const size_t qb = d * sizeof(float) +
		                  (size_t)((d + 31) / 32) * PF6_QWORDS * sizeof(uint32_t);
		HIP_CHECK(ctx, hipMalloc(&ctx->q_dev, qb));
		if (ctx->q_pin)
			(void)hipHostFree(ctx->q_pin);
		HIP_CHECK(ctx, hipHostMalloc(&ctx->q_pin, qb));
		ctx->q_cap = d;
	}
	uint64_t need = nblocks * k * sizeof(Cand);
	if (ctx->block_out_cap < need) {
		if (ctx->block_out)
			(void)hipFree(ctx->block_out);
		HIP_CHECK(ctx, hipMalloc(&ctx->block_out, need));
		ctx->block_out_cap = need;
	}
	if (!ctx->final_out)
		HIP_CHECK(ctx, hipMalloc(&ctx->final_out, MAX_K * sizeof(Cand)));
	if (!ctx->merge_tmp)
		HIP_CHECK(ctx,
		          hipMalloc(&ctx->merge_tmp, 32 * MAX_K * sizeof(Cand)));
	return SDBV_OK;
}

// Upload the query: q into the pinned staging buffer, then q_bytes of it
// (the d floats, and whatever the caller put behind them) to ctx->q_dev.
static int stage_query(sdbv_ctx *ctx, const float *q, uint32_t d,
                       size_t q_bytes) {
	std::memcpy(ctx->q_pin, q, d * sizeof(float));
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->q_dev, ctx->q_pin, q_bytes,
	                              hipMemcpyHostToDevice, ctx->stream));
	return SDBV_OK;
}

// Hand the first m selected candidates to the caller.
static void copy_results(const Cand *host_out, uint32_t m, uint64_t *out_ids,
                         double *out_dists, uint32_t *out_n) {
	*out_n = m;
	for (uint32_t i = 0; i < m; i++) {
		out_ids[i] = host_out[i].id;
		out_dists[i] = host_out[i].dist;
	}
}

// Grid of k_scan: contiguous spans of whole tiles per block, at most 2048
// blocks (enough to fill 256 CUs).
static uint64_t scan_grid(uint64_t n, uint64_t *rows_per_block) {
	uint64_t tiles = (n + TILE - 1) / TILE;
	uint64_t nblocks = tiles < 2048 ? tiles : 2048;
	if (nblocks == 0)
		nblocks = 1;
	uint64_t tiles_per_block = (tiles + nblocks - 1) / nblocks;
	*rows_per_block = tiles_per_block * TILE;
	return (n + *rows_per_block - 1) / *rows_per_block;
}

// Launch k_scan over scan_grid (mask = nullptr: every row below n).
static void launch_scan(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                        uint64_t nblocks, uint64_t rows_per_block,
                        const uint64_t *mask) {
#define LAUNCH_SCAN(M, MASKED)                                                 \
	hipLaunchKernelGGL((k_scan<M, MASKED>), dim3((uint32_t)nblocks),           \
	                   dim3(THREADS), 0, ctx->stream, t.cm, t.norms, t.n,      \
	                   t.n_pad, t.d, ctx->q_dev, q_norm, k, rows_per_block,    \
	                   (Cand *)ctx->block_out, t.ids_dev, mask)
	const bool cosine = t.metric == SDBV_METRIC_COSINE;
	if (mask) {
		if (cosine)
			LAUNCH_SCAN(0, true);
		else
			LAUNCH_SCAN(1, true);
	} else {
		if (cosine)
			LAUNCH_SCAN(0, false);
		else
			LAUNCH_SCAN(1, false);
	}
#undef LAUNCH_SCAN
}

// The k_merge tree over the nblocks * k block winners in ctx->block_out:
// the top-k lands in ctx->final_out. Top-k of per-slice top-ks is the global
// top-k, exactly. A caller whose next kernel folds level 2 into itself
// passes fold: of a two-level tree only level 1 then runs, *fold receives
// the G * k winners it left in ctx->merge_tmp, and ctx->final_out is not
// written; a single-level tree runs whole and leaves *fold 0.
static void launch_merge_tree(sdbv_ctx *ctx, uint64_t nblocks, uint32_t k,
                              uint32_t *fold = nullptr) {
	uint64_t total = nblocks * k;
	const uint64_t G = 32; // level-1 fan-in
	if (fold)
		*fold = 0;
	if (total > 4096 && nblocks > G) {
		// two levels: G slices in parallel, then one block over G * k
		uint64_t per = ((nblocks + G - 1) / G) * k;
		hipLaunchKernelGGL(k_merge, dim3((uint32_t)G), dim3(THREADS), 0,
		                   ctx->stream, (Cand *)ctx->block_out, total, k, per,
		                   (Cand *)ctx->merge_tmp);
		if (fold) {
			*fold = (uint32_t)(G * k);
			return;
		}
		hipLaunchKernelGGL(k_merge, dim3(1), dim3(THREADS), 0, ctx->stream,
		                   (Cand *)ctx->merge_tmp, G * k, k, G * k,
		                   (Cand *)ctx->final_out);
	} else {
		hipLaunchKernelGGL(k_merge, dim3(1), dim3(THREADS), 0, ctx->stream,
		                   (Cand *)ctx->block_out, total, k, total,
		                   (Cand *)ctx->final_out);
	}
}

// Launch the all-distances computation for any metric (q already staged in
// ctx->q_dev). Jaccard runs its block-per-row LDS-set kernel; the rest run
// the per-lane k_all_dists chain.
static void launch_all_dists(sdbv_ctx *ctx, Table &t, const float *q,
                             double *dout) {
	uint64_t nb = (t.n + THREADS - 1) / THREADS;
	double q_norm = t.metric == SDBV_METRIC_COSINE
	                    ? sqrt((double)h_sumsq_f32(q, t.d))
	                    : 0;
	double q_mean = t.metric == SDBV_METRIC_PEARSON ? h_mean_f32(q, t.d) : 0;
#define LAUNCH_AD(M)                                                       \
	hipLaunchKernelGGL(k_all_dists<M>, dim3((uint32_t)nb), dim3(THREADS), \
	                   0, ctx->stream, t.cm, t.norms, t.n, t.n_pad, t.d,  \
	                   ctx->q_dev, q_norm, t.order, q_mean, dout)
	switch (t.metric) {
	case SDBV_METRIC_COSINE: LAUNCH_AD(0); break;
	case SDBV_METRIC_EUCLIDEAN: LAUNCH_AD(1); break;
	case SDBV_METRIC_MANHATTAN: LAUNCH_AD(2); break;
	case SDBV_METRIC_CHEBYSHEV: LAUNCH_AD(3); break;
	case SDBV_METRIC_HAMMING: LAUNCH_AD(4); break;
	case SDBV_METRIC_JACCARD:
		hipLaunchKernelGGL(k_jaccard_dists, dim3((uint32_t)t.n), dim3(256),
		                   0, ctx->stream, t.cm, t.n, t.n_pad, t.d,
		                   ctx->q_dev, dout);
		break;
	case SDBV_METRIC_MINKOWSKI: LAUNCH_AD(6); break;
	case SDBV_METRIC_PEARSON: LAUNCH_AD(7); break;
	}
#undef LAUNCH_AD
}

// All-distances launch + exact host selection: the route for k beyond the
// scan kernel's LDS top-K window (MAX_K) and for the six non-headline
// metrics (SURVEY §8 a2 closure) whenever knn_all_dists_route does not take
// the device select. ids are strictly
// increasing, so (dist, row) order equals the contract's (dist, id)
// order. Costs one n-f64 D2H per query. Under a filter (allow not null:
// ceil(n / 64) validated words) the host selection skips the rows the bitmap
// does not allow, and last_rows_scanned is the caller's. Caller holds
// ctx->mu.
static int knn_large_k(sdbv_ctx *ctx, Table &t, const float *q, uint32_t d,
                       uint32_t k, const uint64_t *allow, uint64_t *out_ids,
                       double *out_dists, uint32_t *out_n) {
	int rc = ensure_query_scratch(ctx, d, 1, 1);
	if (rc != SDBV_OK)
		return rc;
	rc = stage_query(ctx, q, d, d * sizeof(float));
	if (rc != SDBV_OK)
		return rc;
	double *dout = nullptr;
	HIP_CHECK(ctx, hipMalloc(&dout, t.n * sizeof(double)));
	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	launch_all_dists(ctx, t, q, dout);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	std::vector<double> hd(t.n);
	std::vector<uint64_t> hids(t.n);
	if (hipMemcpyAsync(hd.data(), dout, t.n * sizeof(double),
	                   hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
	    hipMemcpyAsync(hids.data(), t.ids_dev, t.n * sizeof(uint64_t),
	                   hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
	    hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipGetLastError() != hipSuccess) {
		(void)hipFree(dout);
		ctx->err = "knn_large_k: device error";
		return SDBV_ERR_HIP;
	}
	(void)hipFree(dout);
	float ms = 0;
	(void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
	ctx->stats.last_scan_kernel_ms = ms;
	ctx->stats.last_merge_kernel_ms = 0;
	if (!allow)
		ctx->stats.last_rows_scanned = t.n;
	// bounded max-heap of (total_key(dist), row): keep the k smallest
	auto tkey = [](double x) {
		uint64_t bits;
		std::memcpy(&bits, &x, 8);
		return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
	};
	std::priority_queue<std::pair<uint64_t, uint64_t>> heap;
	for (uint64_t r = 0; r < t.n; r++) {
		if (allow && !((allow[r >> 6] >> (r & 63)) & 1ULL))
			continue;
		std::pair<uint64_t, uint64_t> e{tkey(hd[r]), r};
		if (heap.size() < k) {
			heap.push(e);
		} else if (e < heap.top()) {
			heap.pop();
			heap.push(e);
		}
	}
	uint32_t m = (uint32_t)heap.size();
	*out_n = m;
	for (uint32_t i = m; i-- > 0;) {
		auto e = heap.top();
		heap.pop();
		out_ids[i] = hids[e.second];
		out_dists[i] = hd[e.second];
	}
	return SDBV_OK;
}

// Host side of the device select (kernels: "Device select of the
// all-distances route", above the C-ABI block).
static int ensure_cap(sdbv_ctx *ctx, void **buf, uint64_t *cap, uint64_t need);
static int upload_filter_mask(sdbv_ctx *ctx, const Table &t,
                              const uint64_t *allow, uint64_t allow_words);
// All-distances launch + device select (last_scan_path 21, 22 under a
// bitmap). count = the rows considered: t.n, or the allowed rows of the
// filtered call (at least 1, its bitmap validated). The bitmap only reaches
// the select; the distance kernel computes every row. Caller holds ctx->mu.
static int knn_device_select(sdbv_ctx *ctx, Table &t, const float *q,
                             uint32_t d, uint32_t k, const uint64_t *allow,
                             uint64_t count, uint64_t *out_ids,
                             double *out_dists, uint32_t *out_n) {
	const uint32_t k_eff = (uint32_t)(k < count ? k : count);
	int rc = ensure_query_scratch(ctx, d, 1, 1);
	if (rc != SDBV_OK)
		return rc;
	rc = stage_query(ctx, q, d, d * sizeof(float));
	if (rc != SDBV_OK)
		return rc;
	const uint64_t res_bytes = sizeof(SelHead) + (uint64_t)k_eff * sizeof(Cand);
	if ((rc = ensure_cap(ctx, (void **)&ctx->sel_dists, &ctx->sel_dists_cap,
	                     t.n * sizeof(double))) ||
	    (rc = ensure_cap(ctx, &ctx->sel_dev, &ctx->sel_dev_cap,
	                     sizeof(SelDev) + (uint64_t)k_eff * sizeof(Cand))))
		return rc;
	if (ctx->sel_pin_cap < res_bytes) {
		if (ctx->sel_pin)
			(void)hipHostFree(ctx->sel_pin);
		ctx->sel_pin = nullptr;
		ctx->sel_pin_cap = 0;
		HIP_CHECK(ctx, hipHostMalloc(&ctx->sel_pin, res_bytes));
		ctx->sel_pin_cap = res_bytes;
	}
	if (allow) {
		rc = upload_filter_mask(ctx, t, allow, (t.n + 63) / 64);
		if (rc != SDBV_OK)
			return rc;
	}
	SelDev *dev = (SelDev *)ctx->sel_dev;
	Cand *res_dev = (Cand *)((char *)ctx->sel_dev + sizeof(SelDev));
	const uint64_t span = (uint64_t)THREADS * SEL_CHUNKS;
	uint64_t nb = (t.n + span - 1) / span;
	nb = nb < 1 ? 1 : nb > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : nb;

	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	launch_all_dists(ctx, t, q, ctx->sel_dists);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	HIP_CHECK(ctx, hipMemsetAsync(dev, 0, sizeof(SelDev), ctx->stream));
	for (int pass = 0; pass < SEL_PASSES; pass++) {
		if (allow)
			hipLaunchKernelGGL(k_sel_hist<true>, dim3((uint32_t)nb),
			                   dim3(THREADS), 0, ctx->stream, ctx->sel_dists,
			                   t.n, ctx->flt_mask, dev, pass, k_eff);
		else
			hipLaunchKernelGGL(k_sel_hist<false>, dim3((uint32_t)nb),
			                   dim3(THREADS), 0, ctx->stream, ctx->sel_dists,
			                   t.n, (const uint64_t *)nullptr, dev, pass, k_eff);
	}
	if (allow)
		hipLaunchKernelGGL(k_sel_emit<true>, dim3((uint32_t)nb), dim3(THREADS),
		                   0, ctx->stream, ctx->sel_dists, t.n, ctx->flt_mask,
		                   t.ids_dev, dev, res_dev, k_eff);
	else
		hipLaunchKernelGGL(k_sel_emit<false>, dim3((uint32_t)nb), dim3(THREADS),
		                   0, ctx->stream, ctx->sel_dists, t.n,
		                   (const uint64_t *)nullptr, t.ids_dev, dev, res_dev,
		                   k_eff);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->sel_pin, &dev->head, res_bytes,
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());

	float ms_dist = 0, ms_sel = 0;
	(void)hipEventElapsedTime(&ms_dist, ctx->ev0, ctx->ev1);
	(void)hipEventElapsedTime(&ms_sel, ctx->ev1, ctx->ev2);
	ctx->stats.last_scan_kernel_ms = ms_dist;
	ctx->stats.last_merge_kernel_ms = ms_sel;
	ctx->stats.last_scan_path = allow ? 22u : 21u;
	if (!allow)
		ctx->stats.last_rows_scanned = t.n;

	const SelHead *head = (const SelHead *)ctx->sel_pin;
	if (head->count != k_eff) {
		ctx->err = "device select: emitted " + std::to_string(head->count) +
		           " rows, expected " + std::to_string(k_eff);
		return SDBV_ERR_HIP;
	}
	Cand *res = (Cand *)((char *)ctx->sel_pin + sizeof(SelHead));
	std::sort(res, res + k_eff, [](const Cand &a, const Cand &b) {
		const uint64_t ka = sel_total_key(a.dist), kb = sel_total_key(b.dist);
		return ka != kb ? ka < kb : a.id < b.id;
	});
	copy_results(res, k_eff, out_ids, out_dists, out_n);
	return SDBV_OK;
}

// SDBV_SELECT_DEVICE / SDBV_SELECT_DEVICE_MIN_ROWS, read at each call.
static bool select_device_policy(const Table &t) {
	return shadow_policy(&t, "SDBV_SELECT_DEVICE", "SDBV_SELECT_DEVICE_MIN_ROWS",
	                     SEL_DEFAULT_MIN_ROWS);
}

// The all-distances route of sdbv_knn_bruteforce, _filtered and the non-GEMM
// sdbv_knn_batch: the device select when k <= SEL_MAX_K, the rows fit 32-bit
// indices and the policy admits the table; otherwise knn_large_k, unchanged.
// count as for knn_device_select. last_total_ms is the wall time of either.
static int knn_all_dists_route(sdbv_ctx *ctx, Table &t, const float *q,
                               uint32_t d, uint32_t k, const uint64_t *allow,
                               uint64_t count, uint64_t *out_ids,
                               double *out_dists, uint32_t *out_n) {
	auto t_start = std::chrono::steady_clock::now();
	int rc;
	if (k <= SEL_MAX_K && count > 0 && t.n < (1ULL << 32) &&
	    select_device_policy(t))
		rc = knn_device_select(ctx, t, q, d, k, allow, count, out_ids,
		                       out_dists, out_n);
	else
		rc = knn_large_k(ctx, t, q, d, k, allow, out_ids, out_dists, out_n);
	ctx->stats.last_total_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t_start)
	        .count();
	return rc;
}

// Row-span grid of the prefilter sweep of shadow tier kind (1..3 and 5; 4 =
// the int6 tier's H-only stream, unmasked only): contiguous
// spans of the tier's tiles, sized so that the whole grid is resident at once
// (one round, every block the same span). A grid of a few more blocks than
// the chip holds runs a second, mostly empty round with too few bytes in
// flight per CU — 3.5 % of the kernel at 10M rows
// (profiles/prefilter_scan.md).
static uint64_t prefilter_grid(sdbv_ctx *ctx, uint64_t n, int kind,
                               bool masked, uint64_t *rows_per_block) {
	uint64_t &slots = ctx->pf_slots[masked][kind];
	if (slots == 0) {
		int per_cu = 0, cus = 0;
		const void *kernel = nullptr;
		switch (kind) {
		case 1:
			kernel = masked ? (const void *)k_prefilter<true>
			                : (const void *)k_prefilter<false>;
			break;
		case 2:
			kernel = masked ? (const void *)k_prefilter_i8<true>
			                : (const void *)k_prefilter_i8<false>;
			break;
		case 3:
			kernel = masked ? (const void *)k_prefilter_i6<true>
			                : (const void *)k_prefilter_i6<false>;
			break;
		case 4:
			kernel = (const void *)k_prefilter_i6<false, true>;
			break;
		case 5:
			kernel = masked ? (const void *)k_prefilter_i8<true, true>
			                : (const void *)k_prefilter_i8<false, true>;
			break;
		}
		hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
		    &per_cu, kernel, THREADS, 0);
		if (e != hipSuccess ||
		    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
		                          ctx->device) != hipSuccess ||
		    per_cu <= 0 || cus <= 0) {
			(void)hipGetLastError();
			slots = 2048;
		} else {
			slots = (uint64_t)per_cu * (uint64_t)cus;
		}
	}
	const uint64_t tile = SHADOW_TIERS[kind].tile;
	uint64_t tiles = (n + tile - 1) / tile;
	uint64_t nblocks = tiles < slots ? tiles : slots;
	if (nblocks == 0)
		nblocks = 1;
	uint64_t tiles_per_block = (tiles + nblocks - 1) / nblocks;
	*rows_per_block = tiles_per_block * tile;
	return (n + *rows_per_block - 1) / *rows_per_block;
}

struct PfQ6 { // int6 tier: the quantised query's kernel operands
	float qscale = 0.f; // f32(sq / |q|)
	float qeps = 0.f;   // 1.01 rho_q, rounded up
	uint32_t bias = 0;  // 65536 d_pad - 32 sum qu (mod 2^32)
	uint32_t bias4 = 0; // the H-only stream's: -61 sum cq (mod 2^32)
};

static inline int shadow_kind(const Table &t) { return t.sh.kind; }

// Upload the query for a call that may take the prefilter of tier kind (0:
// none, the plain query): the int6 tier's digit words ride behind the query
// in the same copy and *q6 receives its kernel operands; *qbias receives the
// int8 tier's bias term 128 * sum q_k, one f64 sum rounded once. The l2
// tier's PfL2Q (the caller's, from pf_l2_query) rides behind the query too.
static int stage_query_pf(sdbv_ctx *ctx, const float *q, uint32_t d,
                          double q_norm, int kind, PfQ6 *q6, float *qbias,
                          const PfL2Q *l2 = nullptr) {
	size_t q_bytes = d * sizeof(float);
	*qbias = 0.f;
	if (kind == 5) {
		// fits: the buffers hold at least PF6_QWORDS dwords behind the query
		static_assert(sizeof(PfL2Q) <= PF6_QWORDS * sizeof(uint32_t), "");
		std::memcpy(ctx->q_pin + d, l2, sizeof(PfL2Q));
		q_bytes += sizeof(PfL2Q);
	} else if (kind == 3) {
		const uint32_t G = (d + 31) / 32;
		float sq, rho;
		uint32_t qs;
		pf_q12(q, d, q_norm, (uint32_t *)(ctx->q_pin + d), nullptr, &sq, &rho,
		       &qs);
		q_bytes += (size_t)G * PF6_QWORDS * sizeof(uint32_t);
		q6->qscale = (float)((double)sq / q_norm);
		q6->qeps = rho > 0.f ? pf_round_up_f32(1.01 * (double)rho) : 0.f;
		q6->bias = 65536u * (32u * G) - 32u * qs;
		q6->bias4 = 61u * (2048u * (32u * G) - qs);
	} else if (kind == 2) {
		double qsum = 0.0;
		for (uint32_t i = 0; i < d; i++)
			qsum += (double)q[i];
		*qbias = (float)(128.0 * qsum);
	}
	return stage_query(ctx, q, d, q_bytes);
}

// Device scratch of both prefilter paths: scores for sn_pad rows, the
// candidate list, its rescored Cands and the result block with the counters.
static int ensure_prefilter_scratch(sdbv_ctx *ctx, uint64_t sn_pad) {
	if (ctx->pf_scores_cap < sn_pad) {
		if (ctx->pf_scores)
			(void)hipFree(ctx->pf_scores);
		ctx->pf_scores = nullptr;
		ctx->pf_scores_cap = 0;
		HIP_CHECK(ctx, hipMalloc(&ctx->pf_scores, sn_pad * sizeof(float)));
		ctx->pf_scores_cap = sn_pad;
	}
	if (!ctx->pf_rows)
		HIP_CHECK(ctx, hipMalloc(&ctx->pf_rows,
		                         PF_CAND_CAP * sizeof(uint32_t)));
	if (!ctx->pf_cands)
		HIP_CHECK(ctx, hipMalloc(&ctx->pf_cands, PF_CAND_CAP * sizeof(Cand)));
	if (!ctx->pf_res)
		HIP_CHECK(ctx, hipMalloc(&ctx->pf_res, (MAX_K + 2) * sizeof(Cand)));
	return SDBV_OK;
}

// The prefilter path of sdbv_knn_bruteforce (k <= MAX_K, table with a
// shadow, query inside the tier's window; q already in ctx->q_dev and the
// query scratch sized for prefilter_grid). host_out[0..k) receives the
// exact top-k, *ncand the candidate count; *ncand > PF_CAND_CAP means the
// list overflowed and host_out is void: the caller runs the exact scan.
// One D2H copy and one sync, like the exact path. Caller holds ctx->mu.
// mask = nullptr for the unfiltered call; the filtered call passes the
// device bitmap of upload_filter_mask (sn_pad / 64 words) and gets the
// top-k of the allowed rows: the stream runs masked, everything behind it
// is the same.
static int knn_prefilter(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                         float qbias, const PfQ6 &q6, const uint64_t *mask,
                         Cand *host_out, uint32_t *ncand) {
	const Shadow &sh = t.sh;
	const int kind = sh.kind;
	int rc = ensure_prefilter_scratch(ctx, sh.sn_pad);
	if (rc != SDBV_OK)
		return rc;

	uint64_t rows_per_block = 0;
	uint64_t nblocks =
	    prefilter_grid(ctx, t.n, kind, mask != nullptr, &rows_per_block);
	Cand *res = (Cand *)ctx->pf_res;
	// device counter: behind the k results and the copy of the count that
	// k_pf_final appends to them
	uint32_t *cand_cnt = (uint32_t *)&res[MAX_K + 1];
	const float inv_q = (float)(1.0 / q_norm);

	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
// KT / KF: the kernel's MASKED and unmasked instantiations
#define LAUNCH_PF2(KT, KF, ...)                                                \
	do {                                                                       \
		if (mask)                                                              \
			hipLaunchKernelGGL(KT, dim3((uint32_t)nblocks), dim3(THREADS), 0,  \
			                   ctx->stream, __VA_ARGS__, rows_per_block,       \
			                   ctx->pf_scores, (Cand *)ctx->block_out,         \
			                   cand_cnt, mask);                                \
		else                                                                   \
			hipLaunchKernelGGL(KF, dim3((uint32_t)nblocks), dim3(THREADS), 0,  \
			                   ctx->stream, __VA_ARGS__, rows_per_block,       \
			                   ctx->pf_scores, (Cand *)ctx->block_out,         \
			                   cand_cnt, mask);                                \
	} while (0)
#define LAUNCH_PF(KERNEL, ...)                                                 \
	LAUNCH_PF2(KERNEL<true>, KERNEL<false>, __VA_ARGS__)
	switch (kind) {
	case 1:
		LAUNCH_PF(k_prefilter, (const uint16_t *)sh.codes, sh.pinv(), t.n,
		          sh.sn_pad, t.d, ctx->q_dev, inv_q, k);
		break;
	case 2:
		LAUNCH_PF(k_prefilter_i8, (const uint8_t *)sh.codes, sh.pscale(),
		          sh.peps(), t.n, sh.sn_pad, t.d, ctx->q_dev, inv_q, qbias, k);
		break;
	case 3:
		LAUNCH_PF(k_prefilter_i6, (const uint4 *)sh.plane_h(),
		          (const uint2 *)sh.plane_l(t.d), sh.pscale(), sh.peps(),
		          sh.xsum(), t.n, sh.sn_pad, (t.d + 31) / 32,
		          (const uint32_t *)(ctx->q_dev + t.d), q6.qscale, q6.qeps,
		          q6.bias, k);
		break;
	case 5: // the int8 stream with the euclidean finish: inv_q is not read
		LAUNCH_PF2((k_prefilter_i8<true, true>), (k_prefilter_i8<false, true>),
		           (const uint8_t *)sh.codes, sh.pscale(), sh.l2_xx(), t.n,
		           sh.sn_pad, t.d, ctx->q_dev, 0.f, qbias, k);
		break;
	}
#undef LAUNCH_PF2
#undef LAUNCH_PF
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	// K smallest approximate distances (int8, int6: upper bounds) ->
	// final_out (A_K, or U_K, = entry k-1)
	launch_merge_tree(ctx, nblocks, k);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	{
		uint64_t ngrp = (t.n + 3) / 4;
		uint64_t nb = (ngrp + THREADS - 1) / THREADS;
		if (nb > 2048)
			nb = 2048;
		if (nb == 0)
			nb = 1;
		hipLaunchKernelGGL(k_pf_compact, dim3((uint32_t)nb), dim3(THREADS), 0,
		                   ctx->stream, ctx->pf_scores, t.n,
		                   (const Cand *)ctx->final_out, k,
		                   // per-row bounds (int8, int6, l2): no window on top
		                   kind == 1 ? pf_eps(t.d) : 0.0f, cand_cnt,
		                   ctx->pf_rows);
		if (kind == 5)
			hipLaunchKernelGGL(k_pf_rescore<1>, dim3(PF_RESCORE_BLOCKS),
			                   dim3(64), 0, ctx->stream, t.cm, t.norms,
			                   t.ids_dev, t.n_pad, t.d, ctx->q_dev, q_norm,
			                   cand_cnt, ctx->pf_rows, (Cand *)ctx->pf_cands);
		else
			hipLaunchKernelGGL(k_pf_rescore<0>, dim3(PF_RESCORE_BLOCKS),
			                   dim3(64), 0, ctx->stream, t.cm, t.norms,
			                   t.ids_dev, t.n_pad, t.d, ctx->q_dev, q_norm,
			                   cand_cnt, ctx->pf_rows, (Cand *)ctx->pf_cands);
	}
	HIP_CHECK(ctx, hipEventRecord(ctx->ev3, ctx->stream));
	hipLaunchKernelGGL(k_pf_final, dim3(1), dim3(THREADS), 0, ctx->stream,
	                   (Cand *)ctx->pf_cands, cand_cnt, k, res);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev4, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(host_out, res, (k + 1) * sizeof(Cand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	*ncand = (uint32_t)host_out[k].id;

	float ms_pre = 0, ms_sel = 0, ms_rescore = 0, ms_final = 0;
	(void)hipEventElapsedTime(&ms_pre, ctx->ev0, ctx->ev1);
	(void)hipEventElapsedTime(&ms_sel, ctx->ev1, ctx->ev2);
	(void)hipEventElapsedTime(&ms_rescore, ctx->ev2, ctx->ev3);
	(void)hipEventElapsedTime(&ms_final, ctx->ev3, ctx->ev4);
	ctx->stats.last_scan_kernel_ms = (double)ms_pre + ms_rescore;
	ctx->stats.last_merge_kernel_ms = (double)ms_sel + ms_final;
	if (!mask) // the filtered call keeps its allowed-row count
		ctx->stats.last_rows_scanned = t.n;
	return SDBV_OK;
}

// SDBV_SCAN_PREFILTER_H4_LIST_MAX, read at each call: the capacity of the
// two-stage path's first list. Default and ceiling PF4_LIST_CAP.
static uint32_t pf4_list_max() {
	uint64_t cap = PF4_LIST_CAP;
	const char *e = getenv("SDBV_SCAN_PREFILTER_H4_LIST_MAX");
	if (e && *e) {
		uint64_t v = strtoull(e, nullptr, 10);
		if (v < cap)
			cap = v;
	}
	return (uint32_t)cap;
}

// The two-stage path of sdbv_knn_bruteforce over an int6 shadow with the
// H-only side data (conditions and outputs as for knn_prefilter, unmasked;
// DESIGN.md §11d): stream plane H alone, take T from the exact distances of
// the K rows with the smallest H-only upper bounds, list the rows whose
// H-only lower bound is not above T, keep of those the rows whose int6 lower
// bound is not above T, then rescore and select as knn_prefilter does.
// *nstage1 receives the first list's raw count; above list_cap that list
// overflowed, nothing behind it ran and host_out is void: the caller takes
// knn_prefilter. host_out needs MAX_K + 2 entries: the one D2H copy carries
// the device counters behind the results.
static int knn_prefilter_h4(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                            const PfQ6 &q6, uint32_t list_cap, Cand *host_out,
                            uint32_t *ncand, uint32_t *nstage1) {
	const Shadow &sh = t.sh;
	int rc = ensure_prefilter_scratch(ctx, sh.sn_pad);
	if (rc != SDBV_OK)
		return rc;
	if (!ctx->pf4_list)
		HIP_CHECK(ctx, hipMalloc(&ctx->pf4_list,
		                         PF4_LIST_CAP * sizeof(uint32_t)));
	if (!ctx->pf4_thr)
		HIP_CHECK(ctx, hipMalloc(&ctx->pf4_thr, MAX_K * sizeof(Cand)));

	uint64_t rows_per_block = 0;
	const uint64_t nblocks =
	    prefilter_grid(ctx, t.n, 4, false, &rows_per_block);
	Cand *res = (Cand *)ctx->pf_res;
	// device counters behind the results: [0] the candidates, [1] the first
	// list
	uint32_t *cand_cnt = (uint32_t *)&res[MAX_K + 1];
	const uint32_t ngroups = (t.d + 31) / 32;
	const uint32_t *qd = (const uint32_t *)(ctx->q_dev + t.d);
	const Cand *thr = (const Cand *)ctx->pf4_thr;

	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	hipLaunchKernelGGL((k_prefilter_i6<false, true>), dim3((uint32_t)nblocks),
	                   dim3(THREADS), 0, ctx->stream,
	                   (const uint4 *)sh.plane_h(), (const uint2 *)nullptr,
	                   sh.pscale(), sh.peps4(), sh.xsum_h(), t.n, sh.sn_pad,
	                   ngroups, qd, q6.qscale, q6.qeps, q6.bias4, k,
	                   rows_per_block, ctx->pf_scores, (Cand *)ctx->block_out,
	                   cand_cnt, (const uint64_t *)nullptr);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	// K smallest H-only upper bounds, id = row position: in final_out, or
	// as level-1 winners in merge_tmp that k_pf4_threshold selects from
	uint32_t fold = 0;
	launch_merge_tree(ctx, nblocks, k, &fold);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	{
		hipLaunchKernelGGL(k_pf4_threshold, dim3(k), dim3(64), 0, ctx->stream,
		                   t.cm, t.norms, t.ids_dev, t.n_pad, t.d, ctx->q_dev,
		                   q_norm,
		                   (const Cand *)(fold ? ctx->merge_tmp : ctx->final_out),
		                   fold, k, (Cand *)ctx->pf4_thr);
		uint64_t ngrp = (t.n + 3) / 4;
		uint64_t nb = (ngrp + THREADS * PF4_PASSES - 1) / (THREADS * PF4_PASSES);
		if (nb > 512)
			nb = 512;
		if (nb == 0)
			nb = 1;
		hipLaunchKernelGGL(k_pf4_compact, dim3((uint32_t)nb), dim3(THREADS), 0,
		                   ctx->stream, ctx->pf_scores, t.n, thr, k, list_cap,
		                   cand_cnt + 1, ctx->pf4_list);
		hipLaunchKernelGGL(k_pf4_refine, dim3(2048), dim3(THREADS), 0,
		                   ctx->stream, (const uint4 *)sh.plane_h(),
		                   (const uint2 *)sh.plane_l(t.d), sh.pscale(),
		                   sh.peps(), sh.xsum(), sh.sn_pad, ngroups, qd,
		                   q6.qscale, q6.qeps, q6.bias, thr, k, list_cap,
		                   cand_cnt + 1, ctx->pf4_list, cand_cnt,
		                   ctx->pf_rows);
		hipLaunchKernelGGL(k_pf_rescore<0>, dim3(PF_RESCORE_BLOCKS), dim3(64),
		                   0, ctx->stream, t.cm, t.norms, t.ids_dev, t.n_pad,
		                   t.d, ctx->q_dev, q_norm, cand_cnt, ctx->pf_rows,
		                   (Cand *)ctx->pf_cands);
	}
	HIP_CHECK(ctx, hipEventRecord(ctx->ev3, ctx->stream));
	hipLaunchKernelGGL(k_pf_final, dim3(1), dim3(THREADS), 0, ctx->stream,
	                   (Cand *)ctx->pf_cands, cand_cnt, k, res);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev4, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(host_out, res, (MAX_K + 2) * sizeof(Cand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	*ncand = (uint32_t)host_out[k].id;
	uint32_t counters[2];
	std::memcpy(counters, &host_out[MAX_K + 1], sizeof(counters));
	*nstage1 = counters[1];

	float ms_pre = 0, ms_sel = 0, ms_rescore = 0, ms_final = 0;
	(void)hipEventElapsedTime(&ms_pre, ctx->ev0, ctx->ev1);
	(void)hipEventElapsedTime(&ms_sel, ctx->ev1, ctx->ev2);
	(void)hipEventElapsedTime(&ms_rescore, ctx->ev2, ctx->ev3);
	(void)hipEventElapsedTime(&ms_final, ctx->ev3, ctx->ev4);
	ctx->stats.last_scan_kernel_ms = (double)ms_pre + ms_rescore;
	ctx->stats.last_merge_kernel_ms = (double)ms_sel + ms_final;
	ctx->stats.last_rows_scanned = t.n;
	return SDBV_OK;
}

// The exact scan of sdbv_knn_bruteforce: k_scan over the f32 store, then the
// tree merge; host_out[0..k) receives the top-k. q already in ctx->q_dev.
// Caller holds ctx->mu.
static int knn_exact_scan(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                          uint64_t nblocks, uint64_t rows_per_block,
                          Cand *host_out) {
	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	launch_scan(ctx, t, k, q_norm, nblocks, rows_per_block, nullptr);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	launch_merge_tree(ctx, nblocks, k);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->final_out, k * sizeof(Cand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());

	float ms_scan = 0, ms_merge = 0;
	(void)hipEventElapsedTime(&ms_scan, ctx->ev0, ctx->ev1);
	(void)hipEventElapsedTime(&ms_merge, ctx->ev1, ctx->ev2);
	ctx->stats.last_scan_kernel_ms = ms_scan;
	ctx->stats.last_merge_kernel_ms = ms_merge;
	ctx->stats.last_rows_scanned = t.n;
	return SDBV_OK;
}

int sdbv_knn_bruteforce(sdbv_ctx *ctx, uint64_t table, const float *q,
                        uint32_t d, uint32_t k, uint64_t *out_ids,
                        double *out_dists, uint32_t *out_n) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	if (d != t.d)
		return SDBV_ERR_BAD_ARG;
	if (k == 0 || k > (1u << 22))
		return SDBV_ERR_BAD_ARG;
	ctx->stats.last_scan_path = 0;
	ctx->stats.last_prefilter_candidates = 0;
	ctx->stats.last_prefilter_stage1 = 0;
	if (k > MAX_K || t.metric > SDBV_METRIC_EUCLIDEAN)
		return knn_all_dists_route(ctx, t, q, d, k, nullptr, t.n, out_ids,
		                           out_dists, out_n);

	uint64_t rows_per_block = 0;
	const uint64_t nblocks = scan_grid(t.n, &rows_per_block);
	// block_out serves whichever of the grids runs
	const int kind = shadow_kind(t);
	// the two-stage path is chosen at each call, over an int6 shadow that
	// was built with its side data
	const bool use_h4 = kind == 3 && t.sh.h4 && h4_policy(&t);
	uint64_t pf_rows_per_block = 0;
	uint64_t scratch_blocks = std::max(
	    nblocks,
	    kind ? prefilter_grid(ctx, t.n, kind, false, &pf_rows_per_block) : 0);
	if (use_h4)
		scratch_blocks = std::max(
		    scratch_blocks,
		    prefilter_grid(ctx, t.n, 4, false, &pf_rows_per_block));
	int rc = ensure_query_scratch(ctx, d, scratch_blocks, k);
	if (rc != SDBV_OK)
		return rc;
	double q_norm = sqrt((double)h_sumsq_f32(q, d));
	// Prefilter path: a shadowed table and a query whose norm lies in the
	// window the bound is proven for (a non-finite element makes the norm
	// non-finite); the l2 tier's window is pf_l2_query's and holds the zero
	// query. Everything else, and a query whose candidate list overflowed,
	// takes the exact scan; results never depend on the choice.
	PfL2Q l2q;
	const bool use_pf =
	    kind == 5 ? pf_l2_query(q, d, &l2q)
	              : kind != 0 && q_norm >= PF_NORM_MIN && q_norm <= PF_NORM_MAX;
	PfQ6 q6;
	float qbias = 0.f;
	rc = stage_query_pf(ctx, q, d, q_norm, use_pf ? kind : 0, &q6, &qbias,
	                    &l2q);
	if (rc != SDBV_OK)
		return rc;

	auto t_start = std::chrono::steady_clock::now();
	Cand host_out[MAX_K + 2];
	bool served = false; // by the two-stage path, overflowed or not
	if (use_pf && use_h4) {
		const uint32_t list_cap = pf4_list_max();
		uint32_t ncand = 0, nstage1 = 0;
		rc = knn_prefilter_h4(ctx, t, k, q_norm, q6, list_cap, host_out,
		                      &ncand, &nstage1);
		if (rc != SDBV_OK)
			return rc;
		ctx->stats.last_prefilter_stage1 = nstage1;
		if (nstage1 <= list_cap) {
			served = true;
			ctx->stats.last_prefilter_candidates = ncand;
			ctx->stats.last_scan_path = ncand <= PF_CAND_CAP ? 15u : 16u;
		}
	}
	if (use_pf && !served) {
		uint32_t ncand = 0;
		rc = knn_prefilter(ctx, t, k, q_norm, qbias, q6, nullptr, host_out,
		                   &ncand);
		if (rc != SDBV_OK)
			return rc;
		ctx->stats.last_prefilter_candidates = ncand;
		// 1..6 by cosine tier; the l2 tier's 17 / 18 lie behind the filtered
		// call's and the two-stage path's numbers
		ctx->stats.last_scan_path = (ncand <= PF_CAND_CAP ? 1u : 2u) +
		                            (kind == 5 ? 16u : 2u * (uint32_t)(kind - 1));
	}
	if (!(ctx->stats.last_scan_path & 1u)) {
		rc = knn_exact_scan(ctx, t, k, q_norm, nblocks, rows_per_block,
		                    host_out);
		if (rc != SDBV_OK)
			return rc;
	}
	ctx->stats.last_total_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t_start)
	        .count();

	copy_results(host_out, (uint32_t)(k < t.n ? k : t.n), out_ids, out_dists,
	             out_n);
	return SDBV_OK;
}

// ---------------------------------------------------------------------------
// Filtered brute-force KNN
// ---------------------------------------------------------------------------

// Host-only: count the allowed rows below n and list the first cap of them,
// ascending. Bits at or past n are ignored; words the caller did not supply
// count as zero. The filtered call counts rows and builds its row list with
// this same routine.
uint64_t sdbv_filter_rows(const uint64_t *allow, uint64_t allow_words,
                          uint64_t n, uint32_t *out_rows, uint64_t cap) {
	if (!allow)
		return 0;
	uint64_t words = (n + 63) / 64;
	if (words > allow_words)
		words = allow_words;
	if (!out_rows)
		cap = 0;
	uint64_t count = 0;
	for (uint64_t w = 0; w < words; w++) {
		uint64_t bits = allow[w];
		if (w == n / 64) // the partial last word: drop its tail
			bits &= (1ULL << (n & 63)) - 1;
		if (!bits)
			continue;
		const uint64_t pc = (uint64_t)__builtin_popcountll(bits);
		if (count < cap) {
			uint64_t at = count;
			for (uint64_t b = bits; b && at < cap; b &= b - 1)
				out_rows[at++] =
				    (uint32_t)(w * 64 + (uint64_t)__builtin_ctzll(b));
		}
		count += pc;
	}
	return count;
}

// Host-only twin of the device select: the same digit walk (sel_match,
// sel_digit, sel_step) on host histograms, then the rows at or below the
// threshold in result order.
int sdbv_select_topk(const double *dists, uint64_t n, const uint64_t *allow,
                     uint32_t k, uint32_t *out_rows, uint32_t *out_n) {
	if (!out_n || (n && !dists) || n >= (1ULL << 32))
		return SDBV_ERR_BAD_ARG;
	auto allowed = [&](uint64_t r) {
		return !allow || ((allow[r >> 6] >> (r & 63)) & 1ULL);
	};
	uint64_t count = 0;
	for (uint64_t r = 0; r < n; r++)
		count += allowed(r) ? 1 : 0;
	const uint32_t k_eff = (uint32_t)(k < count ? k : count);
	*out_n = 0;
	if (k_eff == 0)
		return SDBV_OK;
	if (!out_rows)
		return SDBV_ERR_BAD_ARG;
	SelState s{0, 0, k_eff, 0, 0};
	uint32_t hist[256];
	for (int pass = 0; pass < SEL_PASSES && !s.done; pass++) {
		std::memset(hist, 0, sizeof(hist));
		for (uint64_t r = 0; r < n; r++) {
			if (!allowed(r))
				continue;
			const uint64_t key = sel_total_key(dists[r]);
			if (sel_match(key, (uint32_t)r, s, pass))
				hist[sel_digit(key, (uint32_t)r, pass)]++;
		}
		sel_step(hist, pass, &s);
	}
	std::vector<std::pair<uint64_t, uint32_t>> got;
	got.reserve(k_eff);
	for (uint64_t r = 0; r < n; r++) {
		if (!allowed(r))
			continue;
		const uint64_t key = sel_total_key(dists[r]);
		if (sel_below(key, (uint32_t)r, s))
			got.emplace_back(key, (uint32_t)r);
	}
	if (!s.done || got.size() != k_eff)
		return SDBV_ERR_HIP; // the walk disagrees with itself: never expected
	std::sort(got.begin(), got.end());
	for (uint32_t i = 0; i < k_eff; i++)
		out_rows[i] = got[i].second;
	*out_n = k_eff;
	return SDBV_OK;
}

// SDBV_FILTER_ROWLIST_MAX, read at each call: the largest allowed-row count
// the row-list path serves. Default and ceiling PF_CAND_CAP; 0 sends every
// filtered call to the masked scan.
static uint64_t filter_rowlist_max() {
	uint64_t cap = PF_CAND_CAP;
	const char *e = getenv("SDBV_FILTER_ROWLIST_MAX");
	if (e && *e) {
		uint64_t v = strtoull(e, nullptr, 10);
		if (v < cap)
			cap = v;
	}
	return cap;
}

// SDBV_FILTER_PREFILTER / SDBV_FILTER_PREFILTER_MIN_ROWS, read at each call:
// whether a filtered call on this shadowed table may stream the shadow. The
// default minimum is the unfiltered tiers' stream-vs-fixed-cost crossover,
// the smallest table that gets a shadow by policy.
static bool filter_prefilter_policy(const Table &t) {
	return shadow_policy(&t, "SDBV_FILTER_PREFILTER",
	                     "SDBV_FILTER_PREFILTER_MIN_ROWS", PF_DEFAULT_MIN_ROWS);
}

// Upload the bitmap of the filtered call to ctx->flt_mask, once per call:
// pinned copy, tail of the last word cleared, zero-filled behind it, one H2D
// copy. The buffers hold max(n_pad, sn_pad) / 64 words on a table as staged:
// k_scan<., true> reads words below roundup(n, TILE) / 64, the masked
// prefilter kernels address rows up to roundup(n, the tier's tile).
static int upload_filter_mask(sdbv_ctx *ctx, const Table &t,
                              const uint64_t *allow, uint64_t allow_words) {
	// No kernel reads a mask word past the last tile that holds rows, and the
	// largest tile (PF8_TILE) is 4096 rows: a capacity that reaches further
	// (a table appended to or reserved) costs no words.
	const uint64_t mwords =
	    std::min(std::max(t.n_pad, t.sh.kind ? t.sh.sn_pad : 0),
	             (t.n + 4095) / 4096 * 4096) /
	    64;
	if (ctx->flt_mask_cap < mwords) {
		if (ctx->flt_mask)
			(void)hipFree(ctx->flt_mask);
		if (ctx->flt_mask_pin)
			(void)hipHostFree(ctx->flt_mask_pin);
		ctx->flt_mask = nullptr;
		ctx->flt_mask_pin = nullptr;
		ctx->flt_mask_cap = 0;
		HIP_CHECK(ctx, hipMalloc(&ctx->flt_mask, mwords * sizeof(uint64_t)));
		HIP_CHECK(ctx,
		          hipHostMalloc(&ctx->flt_mask_pin, mwords * sizeof(uint64_t)));
		ctx->flt_mask_cap = mwords;
	}
	std::memcpy(ctx->flt_mask_pin, allow, allow_words * sizeof(uint64_t));
	if (t.n & 63)
		ctx->flt_mask_pin[allow_words - 1] &= (1ULL << (t.n & 63)) - 1;
	std::memset(ctx->flt_mask_pin + allow_words, 0,
	            (mwords - allow_words) * sizeof(uint64_t));
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->flt_mask, ctx->flt_mask_pin,
	                              mwords * sizeof(uint64_t),
	                              hipMemcpyHostToDevice, ctx->stream));
	return SDBV_OK;
}

// Masked scan of the filtered call: k_scan<., true> over scan_grid under the
// bitmap upload_filter_mask left in ctx->flt_mask, then the merge tree. q
// already in ctx->q_dev, scratch sized for nblocks. Caller holds ctx->mu.
static int knn_masked_scan(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                           uint64_t nblocks, uint64_t rows_per_block,
                           Cand *host_out) {
	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	launch_scan(ctx, t, k, q_norm, nblocks, rows_per_block, ctx->flt_mask);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	launch_merge_tree(ctx, nblocks, k);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->final_out, k * sizeof(Cand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	return SDBV_OK;
}

// Row-list path of the filtered call: upload the count allowed rows the host
// listed in ctx->flt_rows_pin, k_rows_exact on them, one single-block
// k_merge. q already in ctx->q_dev. Caller holds ctx->mu.
static int knn_row_list(sdbv_ctx *ctx, Table &t, uint32_t k, double q_norm,
                        uint32_t count, Cand *host_out) {
	if (!ctx->flt_rows)
		HIP_CHECK(ctx,
		          hipMalloc(&ctx->flt_rows, PF_CAND_CAP * sizeof(uint32_t)));
	if (!ctx->flt_cands)
		HIP_CHECK(ctx, hipMalloc(&ctx->flt_cands, PF_CAND_CAP * sizeof(Cand)));
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->flt_rows, ctx->flt_rows_pin,
	                              count * sizeof(uint32_t),
	                              hipMemcpyHostToDevice, ctx->stream));
	const uint32_t nb = count < PF_RESCORE_BLOCKS ? count : PF_RESCORE_BLOCKS;
	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	if (t.metric == SDBV_METRIC_COSINE)
		hipLaunchKernelGGL(k_rows_exact<0>, dim3(nb), dim3(64), 0, ctx->stream,
		                   t.cm, t.norms, t.ids_dev, t.n_pad, t.d, ctx->q_dev,
		                   q_norm, ctx->flt_rows, count,
		                   (Cand *)ctx->flt_cands);
	else
		hipLaunchKernelGGL(k_rows_exact<1>, dim3(nb), dim3(64), 0, ctx->stream,
		                   t.cm, t.norms, t.ids_dev, t.n_pad, t.d, ctx->q_dev,
		                   q_norm, ctx->flt_rows, count,
		                   (Cand *)ctx->flt_cands);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	hipLaunchKernelGGL(k_merge, dim3(1), dim3(THREADS), 0, ctx->stream,
	                   (Cand *)ctx->flt_cands, (uint64_t)count, k,
	                   (uint64_t)count, (Cand *)ctx->final_out);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(host_out, ctx->final_out, k * sizeof(Cand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	return SDBV_OK;
}

int sdbv_knn_bruteforce_filtered(sdbv_ctx *ctx, uint64_t table, const float *q,
                                 uint32_t d, uint32_t k, const uint64_t *allow,
                                 uint64_t allow_words, uint64_t *out_ids,
                                 double *out_dists, uint32_t *out_n) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	if (d != t.d)
		return SDBV_ERR_BAD_ARG;
	if (k == 0 || k > (1u << 22))
		return SDBV_ERR_BAD_ARG;
	if (!allow || allow_words != (t.n + 63) / 64)
		return SDBV_ERR_BAD_ARG;
	auto t_start = std::chrono::steady_clock::now();
	const bool device_topk = k <= MAX_K && t.metric <= SDBV_METRIC_EUCLIDEAN;
	const uint64_t list_max = device_topk ? filter_rowlist_max() : 0;
	if (list_max && !ctx->flt_rows_pin)
		HIP_CHECK(ctx, hipHostMalloc(&ctx->flt_rows_pin,
		                             PF_CAND_CAP * sizeof(uint32_t)));
	const uint64_t count = sdbv_filter_rows(allow, allow_words, t.n,
	                                        ctx->flt_rows_pin, list_max);
	ctx->stats.last_scan_path = 0;
	ctx->stats.last_prefilter_candidates = 0;
	ctx->stats.last_prefilter_stage1 = 0;
	ctx->stats.last_filter_rows = count;
	ctx->stats.last_rows_scanned = count;
	ctx->stats.last_scan_kernel_ms = 0;
	ctx->stats.last_merge_kernel_ms = 0;
	ctx->stats.last_total_ms = 0;
	if (count == 0) { // nothing allowed: no launch
		*out_n = 0;
		return SDBV_OK;
	}
	if (!device_topk)
		return knn_all_dists_route(ctx, t, q, d, k, allow, count, out_ids,
		                           out_dists, out_n);

	const bool by_list = count <= list_max;
	double q_norm = sqrt((double)h_sumsq_f32(q, d));
	// Shadow path: more allowed rows than the list serves,
	// a shadowed table the policy admits, and a query inside the window the
	// tier's bounds are proven for. Everything else, and a call whose
	// candidate list overflowed, takes the path it took before; results
	// never depend on the choice.
	const int kind = shadow_kind(t);
	PfL2Q l2q;
	const bool use_pf =
	    !by_list && kind != 0 && filter_prefilter_policy(t) &&
	    (kind == 5 ? pf_l2_query(q, d, &l2q)
	               : q_norm >= PF_NORM_MIN && q_norm <= PF_NORM_MAX);
	// the masked scan runs on k_scan's grid; block_out serves whichever of
	// the two grids runs, since an overflow reruns the masked scan
	uint64_t rows_per_block = 0;
	const uint64_t nblocks = scan_grid(t.n, &rows_per_block);
	uint64_t pf_rows_per_block = 0;
	const uint64_t scratch_blocks = std::max(
	    nblocks,
	    use_pf ? prefilter_grid(ctx, t.n, kind, true, &pf_rows_per_block) : 0);
	int rc = ensure_query_scratch(ctx, d, by_list ? 1 : scratch_blocks, k);
	if (rc != SDBV_OK)
		return rc;
	PfQ6 q6;
	float qbias = 0.f;
	rc = stage_query_pf(ctx, q, d, q_norm, use_pf ? kind : 0, &q6, &qbias,
	                    &l2q);
	if (rc != SDBV_OK)
		return rc;
	if (!by_list) {
		rc = upload_filter_mask(ctx, t, allow, allow_words);
		if (rc != SDBV_OK)
			return rc;
	}
	Cand host_out[MAX_K + 1];
	if (use_pf) {
		uint32_t ncand = 0;
		rc = knn_prefilter(ctx, t, k, q_norm, qbias, q6, ctx->flt_mask,
		                   host_out, &ncand);
		if (rc != SDBV_OK)
			return rc;
		ctx->stats.last_prefilter_candidates = ncand;
		ctx->stats.last_scan_path = (ncand <= PF_CAND_CAP ? 9u : 10u) +
		                            (kind == 5 ? 10u : 2u * (uint32_t)(kind - 1));
	}
	if (!(ctx->stats.last_scan_path & 1u)) {
		// no shadow pass, or one that overflowed: the mask is on the device
		if (by_list)
			rc = knn_row_list(ctx, t, k, q_norm, (uint32_t)count, host_out);
		else
			rc = knn_masked_scan(ctx, t, k, q_norm, nblocks, rows_per_block,
			                     host_out);
		if (rc != SDBV_OK)
			return rc;
		float ms_scan = 0, ms_merge = 0;
		(void)hipEventElapsedTime(&ms_scan, ctx->ev0, ctx->ev1);
		(void)hipEventElapsedTime(&ms_merge, ctx->ev1, ctx->ev2);
		ctx->stats.last_scan_kernel_ms = ms_scan;
		ctx->stats.last_merge_kernel_ms = ms_merge;
		if (!use_pf)
			ctx->stats.last_scan_path = by_list ? 8u : 7u;
	}
	ctx->stats.last_total_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t_start)
	        .count();

	copy_results(host_out, (uint32_t)(k < count ? k : count), out_ids,
	             out_dists, out_n);
	return SDBV_OK;
}

// Debug/parity: dump all n distances (small n only; n doubles to host).
int sdbv_all_distances(sdbv_ctx *ctx, uint64_t table, const float *q,
                       uint32_t d, double *out) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	if (d != t.d)
		return SDBV_ERR_BAD_ARG;
	int rc = ensure_query_scratch(ctx, d, 1, 1);
	if (rc != SDBV_OK)
		return rc;
	std::memcpy(ctx->q_pin, q, d * sizeof(float)); // pinned staging
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->q_dev, ctx->q_pin, d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	double *dout = nullptr;
	HIP_CHECK(ctx, hipMalloc(&dout, t.n * sizeof(double)));
	launch_all_dists(ctx, t, q, dout);
	HIP_CHECK(ctx, hipMemcpyAsync(out, dout, t.n * sizeof(double),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	(void)hipFree(dout);
	return SDBV_OK;
}

int sdbv_gather_distance(sdbv_ctx *ctx, uint64_t table, const uint32_t *rows,
                         uint32_t nrows, const float *q, uint32_t d,
                         double *out_dists) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	if (d != t.d || nrows == 0)
		return SDBV_ERR_BAD_ARG;
	int rc = ensure_query_scratch(ctx, d, 1, 1);
	if (rc != SDBV_OK)
		return rc;
	std::memcpy(ctx->q_pin, q, d * sizeof(float)); // pinned staging
	HIP_CHECK(ctx, hipMemcpyAsync(ctx->q_dev, ctx->q_pin, d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	double q_norm = sqrt((double)h_sumsq_f32(q, d));
	uint32_t *rows_dev = nullptr;
	double *dout = nullptr;
	HIP_CHECK(ctx, hipMalloc(&rows_dev, nrows * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipMalloc(&dout, nrows * sizeof(double)));
	HIP_CHECK(ctx, hipMemcpyAsync(rows_dev, rows, nrows * sizeof(uint32_t),
	                              hipMemcpyHostToDevice, ctx->stream));
	if (t.metric == SDBV_METRIC_COSINE)
		hipLaunchKernelGGL(k_gather_dist<0>, dim3(nrows), dim3(64), 0,
		                   ctx->stream, t.cm, t.norms, t.n_pad, t.d, rows_dev,
		                   nrows, ctx->q_dev, q_norm, dout);
	else
		hipLaunchKernelGGL(k_gather_dist<1>, dim3(nrows), dim3(64), 0,
		                   ctx->stream, t.cm, t.norms, t.n_pad, t.d, rows_dev,
		                   nrows, ctx->q_dev, q_norm, dout);
	HIP_CHECK(ctx, hipMemcpyAsync(out_dists, dout, nrows * sizeof(double),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	(void)hipFree(rows_dev);
	(void)hipFree(dout);
	return SDBV_OK;
}

static int ensure_cap(sdbv_ctx *ctx, void **buf, uint64_t *cap, uint64_t need) {
	if (*cap >= need)
		return SDBV_OK;
	if (*buf)
		(void)hipFree(*buf);
	*buf = nullptr;
	*cap = 0;
	HIP_CHECK(ctx, hipMalloc(buf, need));
	*cap = need;
	return SDBV_OK;
}

// ---------------------------------------------------------------------------
// Appending rows to a staged table
// ---------------------------------------------------------------------------
// Capacities grow to multiples of this: the least common multiple of TILE
// and the shadow tiers' tiles, so a grown table has sn_pad == n_pad.
#define APPEND_CAP_ALIGN 4096ull
static_assert(APPEND_CAP_ALIGN % TILE == 0 && APPEND_CAP_ALIGN % PF_TILE == 0 &&
                  APPEND_CAP_ALIGN % PF8_TILE == 0 &&
                  APPEND_CAP_ALIGN % PF6_TILE == 0,
              "a grown capacity must be whole tiles on every tier");
// Rows of one append go through the context's staging buffer in chunks of
// at most this many bytes.
#define APPEND_CHUNK_BYTES (256ull << 20)

uint64_t sdbv_append_capacity(uint64_t n_pad, uint64_t need) {
	if (need <= n_pad)
		return n_pad;
	const uint64_t want = std::max(need, n_pad + n_pad / 2);
	return (want + APPEND_CAP_ALIGN - 1) / APPEND_CAP_ALIGN * APPEND_CAP_ALIGN;
}

// Device bytes of a table's per-row arrays at capacity cap, as staging
// counts them (the shadow and the fixed 4 KiB of bunc aside).
static uint64_t table_store_bytes(const Table &t, uint64_t cap) {
	uint64_t b = (uint64_t)t.d * cap * sizeof(float) + cap * sizeof(uint64_t);
	if (t.norms)
		b += cap * sizeof(double);
	if (t.aux)
		b += cap * sizeof(float);
	return b;
}

// Regrow a table's store to new_cap > n_pad rows (a multiple of
// APPEND_CAP_ALIGN). The new arrays are allocated before the old ones are
// freed, so a failed allocation leaves the table as it was (SDBV_ERR_OOM) and
// the peak is old plus new. cm is copied column by column at the new stride
// with zeros behind the old stride; the per-row arrays keep their first n
// entries. A shadow is rebuilt at the new capacity, same kind and side data;
// one that no longer fits is dropped and the table goes on without.
static int grow_table(sdbv_ctx *ctx, Table *t, uint64_t new_cap) {
	float *cm = nullptr, *aux = nullptr;
	double *norms = nullptr;
	uint64_t *ids = nullptr;
	const bool ok =
	    hipMalloc(&cm, (uint64_t)t->d * new_cap * sizeof(float)) == hipSuccess &&
	    (!t->norms ||
	     hipMalloc(&norms, new_cap * sizeof(double)) == hipSuccess) &&
	    (!t->aux || hipMalloc(&aux, new_cap * sizeof(float)) == hipSuccess) &&
	    hipMalloc(&ids, new_cap * sizeof(uint64_t)) == hipSuccess;
	auto free_new = [&]() {
		for (void *p : {(void *)cm, (void *)norms, (void *)aux, (void *)ids})
			if (p)
				(void)hipFree(p);
	};
	if (!ok) {
		(void)hipGetLastError(); // allocation failure is not sticky
		free_new();
		ctx->err = "grow_table: allocation failed";
		return SDBV_ERR_OOM;
	}
	hipLaunchKernelGGL(k_grow_cm, dim3(8192), dim3(256), 0, ctx->stream, t->cm,
	                   cm, t->n_pad, new_cap, t->d);
	hipError_t e = hipSuccess;
	if (t->n) {
		if (norms)
			e = hipMemcpyAsync(norms, t->norms, t->n * sizeof(double),
			                   hipMemcpyDeviceToDevice, ctx->stream);
		if (aux && e == hipSuccess)
			e = hipMemcpyAsync(aux, t->aux, t->n * sizeof(float),
			                   hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess)
			e = hipMemcpyAsync(ids, t->ids_dev, t->n * sizeof(uint64_t),
			                   hipMemcpyDeviceToDevice, ctx->stream);
	}
	if (e == hipSuccess)
		e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess)
		e = hipGetLastError();
	if (e != hipSuccess) {
		free_new();
		ctx->err = std::string("grow_table: ") + hipGetErrorString(e);
		return SDBV_ERR_HIP;
	}
	(void)hipFree(t->cm);
	if (t->norms)
		(void)hipFree(t->norms);
	if (t->aux)
		(void)hipFree(t->aux);
	(void)hipFree(t->ids_dev);
	t->cm = cm;
	t->norms = norms;
	t->aux = aux;
	t->ids_dev = ids;
	t->n_pad = new_cap;
	t->bytes = table_store_bytes(*t, new_cap) + t->sh.bytes;
	refresh_bytes_staged(ctx);
	if (t->sh.kind) {
		const int kind = t->sh.kind;
		const bool h4 = t->sh.h4;
		free_shadow(ctx, t);
		int rc = build_shadow(ctx, t, kind, h4);
		if (rc != SDBV_OK && rc != SDBV_ERR_OOM)
			return rc;
	}
	return SDBV_OK;
}

uint64_t sdbv_table_capacity(sdbv_ctx *ctx, uint64_t table) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	return it == ctx->tables.end() ? 0 : it->second.n_pad;
}

int sdbv_table_reserve(sdbv_ctx *ctx, uint64_t table, uint64_t rows) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table *t = &it->second;
	if (!t->scan_table)
		return SDBV_ERR_UNSUPPORTED;
	if (rows <= t->n_pad)
		return SDBV_OK;
	if (rows >= (1ULL << 32))
		return SDBV_ERR_BAD_ARG;
	return grow_table(ctx, t, (rows + APPEND_CAP_ALIGN - 1) / APPEND_CAP_ALIGN *
	                              APPEND_CAP_ALIGN);
}

int sdbv_append_rows(sdbv_ctx *ctx, uint64_t table, const float *rows,
                     const uint64_t *ids, uint64_t m, uint32_t d) {
	auto t_start = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table *t = &it->second;
	if (!t->scan_table)
		return SDBV_ERR_UNSUPPORTED;
	if (d != t->d)
		return SDBV_ERR_BAD_ARG;
	if (m == 0)
		return SDBV_OK;
	if (!rows || m >= (1ULL << 32) || t->n + m >= (1ULL << 32))
		return SDBV_ERR_BAD_ARG;
	// tie-break contract: the ids of the whole table stay strictly increasing
	if (ids) {
		if (t->n && ids[0] <= t->last_id)
			return SDBV_ERR_IDS_UNSORTED;
		for (uint64_t i = 1; i < m; i++)
			if (ids[i] <= ids[i - 1])
				return SDBV_ERR_IDS_UNSORTED;
	}
	const uint64_t id_next = t->n ? t->last_id + 1 : 0;

	const uint64_t cap = sdbv_append_capacity(t->n_pad, t->n + m);
	const bool regrow = cap != t->n_pad;
	if (regrow) {
		int rc = grow_table(ctx, t, cap);
		if (rc != SDBV_OK)
			return rc;
	}

	const uint64_t row_bytes = (uint64_t)d * sizeof(float);
	const uint64_t chunk_rows =
	    std::max<uint64_t>(1, APPEND_CHUNK_BYTES / row_bytes);
	int rc = ensure_cap(ctx, &ctx->app_buf, &ctx->app_buf_cap,
	                    std::min(m, chunk_rows) *
	                        (row_bytes + sizeof(uint64_t)));
	if (rc != SDBV_OK)
		return rc;
	BatchAuxHdr *hdr =
	    t->bunc ? (BatchAuxHdr *)(t->bunc + BATCH_UNC_CAP) : nullptr;
	double kernel_ms = 0;
	for (uint64_t done = 0; done < m;) {
		const uint64_t c = std::min(chunk_rows, m - done);
		// d % 4 == 0: the ids behind the rows are 8-byte aligned
		float *rm = (float *)ctx->app_buf;
		uint64_t *idb = (uint64_t *)((char *)ctx->app_buf + c * row_bytes);
		HIP_CHECK(ctx, hipMemcpyAsync(rm, rows + done * d, c * row_bytes,
		                              hipMemcpyHostToDevice, ctx->stream));
		if (ids)
			HIP_CHECK(ctx, hipMemcpyAsync(idb, ids + done, c * sizeof(uint64_t),
			                              hipMemcpyHostToDevice, ctx->stream));
		const uint64_t n0 = t->n + done; // n0 + c <= n_pad
		const uint64_t waves = (n0 + c + 63) / 64 - n0 / 64;
		HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
		hipLaunchKernelGGL(k_append_rows, dim3((uint32_t)waves), dim3(64), 0,
		                   ctx->stream, rm, ids ? idb : (const uint64_t *)nullptr,
		                   id_next + done, t->cm, t->norms, t->aux, t->ids_dev,
		                   n0, c, t->n_pad, d, (int)t->metric, t->bunc, hdr);
		done += c;
		if (done == m && t->sh.kind) {
			// the 256-row blocks that hold [n, n + m): the new rows get their
			// codes, rows that stop being padding lose their NaN side value
			const uint64_t end = (t->n + m + 255) / 256 * 256;
			launch_shadow_rows(ctx, t, t->n + m, t->n / 256 * 256, end);
		}
		HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		HIP_CHECK(ctx, hipGetLastError());
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
		kernel_ms += ms;
	}
	if (hdr) { // as finish_stage reads them
		BatchAuxHdr h;
		HIP_CHECK(ctx, hipMemcpy(&h, hdr, sizeof(h), hipMemcpyDeviceToHost));
		t->bunc_n = h.n_unc;
		std::memcpy(&t->bmax_norm, &h.max_norm_bits, sizeof(double));
	}
	t->last_id = ids ? ids[m - 1] : id_next + m - 1;
	t->n += m;
	ctx->stats.last_append_kernel_ms = kernel_ms;
	ctx->stats.last_append_realloc = regrow ? 1u : 0u;
	ctx->stats.last_append_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t_start)
	        .count();
	return SDBV_OK;
}

// ---------------------------------------------------------------------------
// Updating staged rows in place
// ---------------------------------------------------------------------------
uint64_t sdbv_update_blocks(const uint32_t *row_idx, uint64_t m,
                            uint32_t *out_blocks, uint64_t cap) {
	uint64_t count = 0;
	for (uint64_t i = 0; i < m; i++) {
		const uint32_t b = row_idx[i] / 256;
		if (i && b == row_idx[i - 1] / 256)
			continue;
		if (count < cap)
			out_blocks[count] = b;
		count++;
	}
	return count;
}

int sdbv_update_rows(sdbv_ctx *ctx, uint64_t table, const uint32_t *row_idx,
                     const float *rows, uint64_t m, uint32_t d) {
	auto t_start = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table *t = &it->second;
	if (!t->scan_table)
		return SDBV_ERR_UNSUPPORTED;
	if (d != t->d)
		return SDBV_ERR_BAD_ARG;
	if (m == 0)
		return SDBV_OK;
	if (!rows || !row_idx)
		return SDBV_ERR_BAD_ARG;
	// strictly increasing and below n: no position twice, so m <= n
	for (uint64_t i = 0; i < m; i++)
		if (row_idx[i] >= t->n || (i && row_idx[i] <= row_idx[i - 1]))
			return SDBV_ERR_BAD_ARG;

	// the touched 256-row blocks of the shadow, uploaded once behind the
	// largest chunk
	std::vector<uint32_t> blocks;
	if (t->sh.kind) {
		blocks.resize(sdbv_update_blocks(row_idx, m, nullptr, 0));
		(void)sdbv_update_blocks(row_idx, m, blocks.data(), blocks.size());
	}
	const uint64_t row_bytes = (uint64_t)d * sizeof(float);
	const uint64_t chunk_rows =
	    std::max<uint64_t>(1, APPEND_CHUNK_BYTES / row_bytes);
	const uint64_t list_off =
	    std::min(m, chunk_rows) * (row_bytes + sizeof(uint32_t));
	int rc = ensure_cap(ctx, &ctx->app_buf, &ctx->app_buf_cap,
	                    list_off + blocks.size() * sizeof(uint32_t));
	if (rc != SDBV_OK)
		return rc;
	float *rm = (float *)ctx->app_buf;
	uint32_t *blist = (uint32_t *)((char *)ctx->app_buf + list_off);
	if (!blocks.empty())
		HIP_CHECK(ctx, hipMemcpyAsync(blist, blocks.data(),
		                              blocks.size() * sizeof(uint32_t),
		                              hipMemcpyHostToDevice, ctx->stream));
	double kernel_ms = 0;
	for (uint64_t done = 0; done < m;) {
		const uint64_t c = std::min(chunk_rows, m - done);
		uint32_t *idb = (uint32_t *)((char *)ctx->app_buf + c * row_bytes);
		HIP_CHECK(ctx, hipMemcpyAsync(rm, rows + done * d, c * row_bytes,
		                              hipMemcpyHostToDevice, ctx->stream));
		HIP_CHECK(ctx, hipMemcpyAsync(idb, row_idx + done, c * sizeof(uint32_t),
		                              hipMemcpyHostToDevice, ctx->stream));
		HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
		hipLaunchKernelGGL(k_update_rows, dim3((uint32_t)((c + 63) / 64)),
		                   dim3(64), 0, ctx->stream, rm, idb, t->cm, t->norms,
		                   t->aux, c, t->n_pad, d, (int)t->metric);
		done += c;
		if (done == m) {
			// the shadow over exactly the touched blocks, one launch; then the
			// batch header again from aux (and norms): the fold the append
			// continues cannot forget the row that held the maximum, or a row
			// that had no key and now has one
			launch_shadow_blocks(ctx, t, t->n, 0, blocks.size(), blist);
			if (t->bunc) {
				BatchAuxHdr *hdr = (BatchAuxHdr *)(t->bunc + BATCH_UNC_CAP);
				HIP_CHECK(ctx, hipMemsetAsync(hdr, 0, sizeof(BatchAuxHdr),
				                              ctx->stream));
				const uint64_t nb = std::min<uint64_t>(
				    (t->n + THREADS - 1) / THREADS, REFOLD_MAX_BLOCKS);
				hipLaunchKernelGGL(k_aux_refold, dim3((uint32_t)nb),
				                   dim3(THREADS), 0, ctx->stream, t->aux,
				                   t->norms, t->n, t->bunc, hdr);
			}
		}
		HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		HIP_CHECK(ctx, hipGetLastError());
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
		kernel_ms += ms;
	}
	if (t->bunc) { // as finish_stage reads them
		BatchAuxHdr h;
		HIP_CHECK(ctx, hipMemcpy(&h, t->bunc + BATCH_UNC_CAP, sizeof(h),
		                         hipMemcpyDeviceToHost));
		t->bunc_n = h.n_unc;
		std::memcpy(&t->bmax_norm, &h.max_norm_bits, sizeof(double));
	}
	ctx->stats.last_update_kernel_ms = kernel_ms;
	ctx->stats.last_update_blocks = blocks.size();
	ctx->stats.last_update_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t_start)
	        .count();
	return SDBV_OK;
}

int sdbv_knn_batch(sdbv_ctx *ctx, uint64_t table, const float *Q, uint32_t b,
                   uint32_t d, uint32_t k, uint64_t *out_ids,
                   double *out_dists) {
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	if (d != t.d || b == 0 || k == 0 || k > MAX_K - BATCH_SLACK)
		return SDBV_ERR_BAD_ARG;
	if (t.metric > SDBV_METRIC_EUCLIDEAN) {
		// non-GEMM metrics: per-query all-distances route (exact; the MFMA
		// batch path is only for the genuinely dense cosine/euclidean case)
		for (uint32_t j = 0; j < b; j++) {
			uint32_t m = 0;
			int rc = knn_all_dists_route(ctx, t, Q + (uint64_t)j * d, d, k,
			                             nullptr, t.n,
			                             out_ids + (uint64_t)j * k,
			                             out_dists + (uint64_t)j * k, &m);
			if (rc)
				return rc;
			for (uint32_t i = m; i < k; i++) {
				out_ids[(uint64_t)j * k + i] = ~0ULL;
				out_dists[(uint64_t)j * k + i] =
				    std::numeric_limits<double>::infinity();
			}
		}
		return SDBV_OK;
	}
	const int kk = (int)k + BATCH_SLACK;
	ctx->stats.last_batch_exact_queries = 0;
	ctx->stats.last_batch_refold = 0;

	// Which queries the window serves, which the exact scan (to_exact): a
	// query whose norm the key bound does not cover (zero, non-finite, outside
	// the window's norm range) goes there at once, and so does every query
	// of a table with more rows without a usable key than the list holds;
	// the others only if their window fails its certificate below.
	// The norms are k_qnorms' (the chain of h_sumsq_f32), read back at the
	// call's first synchronisation.
	std::vector<double> h_qnorm(b);
	std::vector<uint8_t> to_exact(b, 0);
	bool qnorms_read = false;
	auto read_qnorms = [&]() -> int {
		if (qnorms_read)
			return SDBV_OK;
		qnorms_read = true;
		HIP_CHECK(ctx, hipMemcpyAsync(h_qnorm.data(), ctx->qnorms,
		                              b * sizeof(double),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		for (uint32_t j = 0; j < b; j++)
			if (!(h_qnorm[j] >= PF_NORM_MIN && h_qnorm[j] <= PF_NORM_MAX) ||
			    t.bunc_n > BATCH_UNC_CAP)
				to_exact[j] = 1;
		return SDBV_OK;
	};

	if (!ctx->blas) {
		if (rocblas_create_handle(&ctx->blas) != rocblas_status_success) {
			ctx->err = "rocblas_create_handle failed";
			return SDBV_ERR_HIP;
		}
		rocblas_set_stream(ctx->blas, ctx->stream);
	}

	// chunk size: multiple of TILE, bounded scratch (<=1 GiB at b=1024)
	// (n_tile, not n_pad: the capacity of a table that was appended to or
	// reserved reaches past the last tile that holds rows)
	const uint64_t n_tile = (t.n + TILE - 1) / TILE * TILE;
	uint64_t chunk = 262144;
	if (chunk > n_tile)
		chunk = n_tile;
	int rc;
	if ((rc = ensure_cap(ctx, (void **)&ctx->S, &ctx->S_cap,
	                     chunk * b * sizeof(float))))
		return rc;
	if ((rc = ensure_cap(ctx, (void **)&ctx->bstate, &ctx->bstate_cap,
	                     (uint64_t)b * kk * sizeof(BCand))))
		return rc;
	if ((rc = ensure_cap(ctx, (void **)&ctx->Q_dev, &ctx->Q_cap,
	                     (uint64_t)b * d * sizeof(float))))
		return rc;
	if ((rc = ensure_cap(ctx, (void **)&ctx->qnorms, &ctx->qnorms_cap,
	                     (uint64_t)b * sizeof(double))))
		return rc;
	// rows without a usable key that every window query recomputes exactly
	const uint32_t n_unc = t.bunc_n <= BATCH_UNC_CAP ? t.bunc_n : 0;
	if ((rc = ensure_cap(ctx, (void **)&ctx->bdists, &ctx->bdists_cap,
	                     (uint64_t)b * std::max<uint32_t>(kk, n_unc) *
	                         sizeof(double))))
		return rc;

	HIP_CHECK(ctx, hipMemcpyAsync(ctx->Q_dev, Q,
	                              (uint64_t)b * d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(k_qnorms, dim3((b + 255) / 256), dim3(256), 0,
	                   ctx->stream, ctx->Q_dev, b, d, ctx->qnorms);
	{
		uint64_t total = (uint64_t)b * kk;
		hipLaunchKernelGGL(k_binit, dim3((uint32_t)((total + 255) / 256)),
		                   dim3(256), 0, ctx->stream, (BCand *)ctx->bstate,
		                   total);
	}

	// Fused MFMA path (default): bootstrap per-query thresholds on the
	// first rows via the legacy rocBLAS + k_batch_topk pass, then ONE
	// hand-written MFMA launch (k_mfma_scan_topk) covers the rest — the
	// score matrix never touches HBM. SDBV_BATCH_LEGACY=1 forces the
	// round-1 path (A/B comparisons); shape constraints fall back too.
	const bool use_fused = (d % FMM_BK) == 0 && (b % FMM_BN) == 0 &&
	                       !std::getenv("SDBV_BATCH_LEGACY");
	uint64_t fused_row0 = t.n; // rows from here on go to the fused kernel
	if (use_fused && t.n > 65536)
		fused_row0 = 65536; // multiple of FMM_BM and TILE

	double ms_gemm = 0, ms_select = 0;
	auto legacy_rows = [&](uint64_t from, uint64_t to) -> int {
		// `to` == t.n means "to the end": extend the last chunk over the
		// padded rows exactly like the round-1 loop (k_batch_topk's n
		// guard skips them); a bounded `to` (the TILE-aligned bootstrap)
		// is covered exactly.
		for (uint64_t row0 = from; row0 < to; row0 += chunk) {
			uint64_t lim = (to == t.n) ? n_tile : to;
			uint32_t nc = (uint32_t)std::min<uint64_t>(chunk, lim - row0);
			const float alpha = 1.0f, beta = 0.0f;
			HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
			// S[nc x b] = corpus[nc x d] (col-major view of cm, lda n_pad)
			//           x Q^T[d x b]    (col-major view of row-major Q)
			if (rocblas_sgemm(ctx->blas, rocblas_operation_none,
			                  rocblas_operation_none, (rocblas_int)nc,
			                  (rocblas_int)b, (rocblas_int)d, &alpha,
			                  t.cm + row0, (rocblas_int)t.n_pad, ctx->Q_dev,
			                  (rocblas_int)d, &beta, ctx->S,
			                  (rocblas_int)nc) != rocblas_status_success) {
				ctx->err = "rocblas_sgemm failed";
				return SDBV_ERR_HIP;
			}
			HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
			hipLaunchKernelGGL(k_batch_topk, dim3(b), dim3(THREADS), 0,
			                   ctx->stream, ctx->S, t.aux, row0, nc, t.n,
			                   (int)t.metric, (BCand *)ctx->bstate, kk);
			HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
			HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
			float m0 = 0, m1 = 0;
			(void)hipEventElapsedTime(&m0, ctx->ev0, ctx->ev1);
			(void)hipEventElapsedTime(&m1, ctx->ev1, ctx->ev2);
			ms_gemm += m0;
			ms_select += m1;
		}
		return SDBV_OK;
	};
	if ((rc = legacy_rows(0, fused_row0)))
		return rc;
	if (fused_row0 < t.n) {
		if ((rc = ensure_cap(ctx, (void **)&ctx->btheta, &ctx->btheta_cap,
		                     (uint64_t)b * sizeof(uint32_t))))
			return rc;
		if ((rc = ensure_cap(ctx, (void **)&ctx->bcand, &ctx->bcand_cap,
		                     (uint64_t)b * FMM_CAND_CAP * sizeof(BCand))))
			return rc;
		if ((rc = ensure_cap(ctx, (void **)&ctx->bcand_cnt,
		                     &ctx->bcand_cnt_cap,
		                     (uint64_t)b * sizeof(uint32_t))))
			return rc;
		hipLaunchKernelGGL(k_theta_init, dim3((b + 255) / 256), dim3(256),
		                   0, ctx->stream, (const BCand *)ctx->bstate, kk, b,
		                   ctx->btheta);
		HIP_CHECK(ctx, hipMemsetAsync(ctx->bcand_cnt, 0,
		                              b * sizeof(uint32_t), ctx->stream));
		uint32_t gx = (uint32_t)((t.n - fused_row0 + FMM_BM - 1) / FMM_BM);
		HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
		hipLaunchKernelGGL(k_mfma_scan_topk, dim3(gx, b / FMM_BN),
		                   dim3(256), 0, ctx->stream, t.cm, t.n_pad, d,
		                   ctx->Q_dev, b, fused_row0, t.n, t.aux,
		                   (int)t.metric, ctx->btheta, (BCand *)ctx->bcand,
		                   ctx->bcand_cnt);
		HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
		hipLaunchKernelGGL(k_cand_fold, dim3(b), dim3(THREADS), 0,
		                   ctx->stream, (const BCand *)ctx->bcand,
		                   ctx->bcand_cnt, (BCand *)ctx->bstate, kk);
		HIP_CHECK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
		std::vector<uint32_t> h_cnt(b);
		HIP_CHECK(ctx, hipMemcpyAsync(h_cnt.data(), ctx->bcand_cnt,
		                              b * sizeof(uint32_t),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		HIP_CHECK(ctx, hipGetLastError());
		float m0 = 0, m1 = 0;
		(void)hipEventElapsedTime(&m0, ctx->ev0, ctx->ev1);
		(void)hipEventElapsedTime(&m1, ctx->ev1, ctx->ev2);
		ms_gemm += m0;
		ms_select += m1;
		if ((rc = read_qnorms()))
			return rc;
		bool overflow = false;
		// (the window of a query bound for the exact scan is never read)
		for (uint32_t j = 0; j < b; j++)
			if (h_cnt[j] > FMM_CAND_CAP && !to_exact[j])
				overflow = true;
		if (overflow) {
			// a candidate buffer filled (adversarially ordered corpus), so
			// appends were dropped: start every state over and run ALL rows
			// through the legacy pass. Presenting only the fused rows on
			// top of the folded state would take the rows already in it a
			// second time (neither k_batch_topk nor block_select_topk
			// deduplicates).
			ctx->stats.last_batch_refold = 1;
			uint64_t total = (uint64_t)b * kk;
			hipLaunchKernelGGL(k_binit, dim3((uint32_t)((total + 255) / 256)),
			                   dim3(256), 0, ctx->stream, (BCand *)ctx->bstate,
			                   total);
			if ((rc = legacy_rows(0, t.n)))
				return rc;
		}
	}

	// exact recompute of survivors with the restated chain
	HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	hipLaunchKernelGGL(k_batch_exact, dim3(b, kk), dim3(64), 0, ctx->stream,
	                   t.cm, t.norms, t.n_pad, t.d, ctx->Q_dev, ctx->qnorms,
	                   (int)t.metric, (const BCand *)ctx->bstate,
	                   (const uint32_t *)nullptr, kk, ctx->bdists);
	HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));

	std::vector<BCand> h_state((uint64_t)b * kk);
	std::vector<double> h_dists((uint64_t)b * kk);
	HIP_CHECK(ctx, hipMemcpyAsync(h_state.data(), ctx->bstate,
	                              h_state.size() * sizeof(BCand),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipMemcpyAsync(h_dists.data(), ctx->bdists,
	                              h_dists.size() * sizeof(double),
	                              hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	HIP_CHECK(ctx, hipGetLastError());
	if ((rc = read_qnorms()))
		return rc;
	float me = 0;
	(void)hipEventElapsedTime(&me, ctx->ev0, ctx->ev1);

	// The rows without a usable key were kept out of every window: each
	// query gets their exact distances as well (the same rows for all).
	std::vector<uint32_t> h_unc(n_unc);
	std::vector<double> h_unc_dists((uint64_t)b * n_unc);
	if (n_unc) {
		hipLaunchKernelGGL(k_batch_exact, dim3(b, n_unc), dim3(64), 0,
		                   ctx->stream, t.cm, t.norms, t.n_pad, t.d, ctx->Q_dev,
		                   ctx->qnorms, (int)t.metric, (const BCand *)nullptr,
		                   (const uint32_t *)t.bunc, (int)n_unc, ctx->bdists);
		HIP_CHECK(ctx, hipMemcpyAsync(h_unc.data(), t.bunc,
		                              n_unc * sizeof(uint32_t),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipMemcpyAsync(h_unc_dists.data(), ctx->bdists,
		                              h_unc_dists.size() * sizeof(double),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		HIP_CHECK(ctx, hipGetLastError());
	}

	// final exact rank per query: ascending (total_cmp(dist), id)
	std::vector<uint64_t> ids_host(t.n);
	HIP_CHECK(ctx, hipMemcpy(ids_host.data(), t.ids_dev,
	                         t.n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	auto total_key = [](double x) {
		uint64_t bits;
		std::memcpy(&bits, &x, 8);
		return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
	};
	std::vector<std::pair<std::pair<uint64_t, uint64_t>, double>> cand(kk +
	                                                                   n_unc);
	for (uint32_t j = 0; j < b; j++) {
		if (to_exact[j])
			continue;
		size_t m = 0;
		float bkey = -std::numeric_limits<float>::infinity();
		for (int c = 0; c < kk; c++) {
			BCand bc = h_state[(uint64_t)j * kk + c];
			if (bc.row == ~0u)
				continue;
			double dd = h_dists[(uint64_t)j * kk + c];
			cand[m++] = {{total_key(dd), ids_host[bc.row]}, dd};
			bkey = std::max(bkey, bc.key);
		}
		std::sort(cand.begin(), cand.begin() + m);
		// Window certificate. A window that is not full
		// holds every row with a key. A full one holds every row whose key
		// is below its largest key bkey; a row as near as the window's k-th
		// nearest (exact distance dk, E(dk) in the key's domain) has a key
		// of at most E(dk) + bound, so bkey above that proves that the
		// k nearest rows with a key are all inside. E is monotone in the
		// distance, in f64 as computed here.
		if (m == (size_t)kk) {
			const double dk = cand[k - 1].second, qn = h_qnorm[j];
			const double ek = t.metric == SDBV_METRIC_COSINE
			                      ? -((1.0 - dk) * qn)
			                      : dk * dk - qn * qn;
			const double bound =
			    sdbv_batch_key_bound(t.metric, d, qn, t.bmax_norm);
			if (!((double)bkey > ek + bound)) {
				to_exact[j] = 1;
				continue;
			}
		}
		for (uint32_t c = 0; c < n_unc; c++) {
			double dd = h_unc_dists[(uint64_t)j * n_unc + c];
			cand[m++] = {{total_key(dd), ids_host[h_unc[c]]}, dd};
		}
		if (n_unc)
			std::sort(cand.begin(), cand.begin() + m);
		uint32_t out_m = (uint32_t)std::min<size_t>(k, m);
		for (uint32_t c = 0; c < out_m; c++) {
			out_ids[(uint64_t)j * k + c] = cand[c].first.second;
			out_dists[(uint64_t)j * k + c] = cand[c].second;
		}
		for (uint32_t c = out_m; c < k; c++) {
			out_ids[(uint64_t)j * k + c] = ~0ULL;
			out_dists[(uint64_t)j * k + c] =
			    std::numeric_limits<double>::infinity();
		}
	}

	// The queries the window could not answer: the single-query exact scan.
	uint64_t rows_per_block = 0;
	const uint64_t nblocks = scan_grid(t.n, &rows_per_block);
	bool scratch_ready = false;
	for (uint32_t j = 0; j < b; j++) {
		if (!to_exact[j])
			continue;
		if (!scratch_ready) {
			if ((rc = ensure_query_scratch(ctx, d, nblocks, k)))
				return rc;
			scratch_ready = true;
		}
		const float *q = Q + (uint64_t)j * d;
		if ((rc = stage_query(ctx, q, d, d * sizeof(float))))
			return rc;
		Cand host_out[MAX_K];
		if ((rc = knn_exact_scan(ctx, t, k, h_qnorm[j], nblocks, rows_per_block,
		                         host_out)))
			return rc;
		const uint32_t out_m = (uint32_t)std::min<uint64_t>(k, t.n);
		for (uint32_t c = 0; c < out_m; c++) {
			out_ids[(uint64_t)j * k + c] = host_out[c].id;
			out_dists[(uint64_t)j * k + c] = host_out[c].dist;
		}
		for (uint32_t c = out_m; c < k; c++) {
			out_ids[(uint64_t)j * k + c] = ~0ULL;
			out_dists[(uint64_t)j * k + c] =
			    std::numeric_limits<double>::infinity();
		}
		ctx->stats.last_batch_exact_queries++;
	}
	ctx->ms_gemm = ms_gemm;
	ctx->ms_select = ms_select;
	ctx->ms_exact = me;
	ctx->stats.last_scan_kernel_ms = ms_gemm; // dominant kernel of the batch
	ctx->stats.last_merge_kernel_ms = ms_select;
	ctx->stats.last_rows_scanned = t.n;
	return SDBV_OK;
}
} // extern "C"

// ===========================================================================
// HNSW — product implementation of the reference graph algorithm
// (hnsw/mod.rs, layer.rs, heuristic.rs, knn.rs queues). Host-side topology +
// build (as in the reference engine); layer-0 query expansion = the GPU
// batched gather+distance kernel. Independent of oracle/ (the oracle is the
// parity checker for this code, never a dependency).
// ===========================================================================

namespace hnsw {

// f64 total_cmp key (knn.rs:128-160)
static inline uint64_t total_key(double x) {
	uint64_t bits;
	std::memcpy(&bits, &x, 8);
	return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
}

// DoublePriorityQueue restatement (knn.rs:15-123): ordered by total_cmp(dist),
// FIFO within equal distance (push order); pop_last removes the LATEST of
// the max key. Implemented as a sorted (key, seq) vector with a lazy head —
// exactly the BTreeMap<FloatKey, VecDeque> observable order, without the
// per-node allocations (this queue is the host build/search hot path).
struct PQ {
	struct E {
		uint64_t key;
		uint32_t seq;
		uint32_t id;
		double d;
	};
	std::vector<E> v; // ascending (key, seq); v[head..] is the live queue
	size_t head = 0;
	uint32_t next_seq = 0;
	size_t n = 0;
	void push(double d, uint32_t id) {
		E e{total_key(d), next_seq++, id, d};
		auto it = std::upper_bound(
		    v.begin() + head, v.end(), e, [](const E &a, const E &b) {
			    return a.key != b.key ? a.key < b.key : a.seq < b.seq;
		    });
		v.insert(it, e);
		n++;
	}
	bool pop_first(double *d, uint32_t *id) {
		if (n == 0)
			return false;
		*d = v[head].d;
		*id = v[head].id;
		head++;
		n--;
		return true;
	}
	void pop_last() { // latest push of the max key == max (key, seq)
		if (n == 0)
			return;
		v.pop_back();
		n--;
	}
	bool peek_first(double *d, uint32_t *id) const {
		if (n == 0)
			return false;
		*d = v[head].d;
		*id = v[head].id;
		return true;
	}
	double peek_last_dist(double fb) const {
		return n == 0 ? fb : v.back().d;
	}
	std::vector<std::pair<double, uint32_t>> to_vec() const {
		std::vector<std::pair<double, uint32_t>> out;
		out.reserve(n);
		for (size_t i = head; i < v.size(); i++)
			out.push_back({v[i].d, v[i].id});
		return out;
	}
};

// Restated per-row distance chain on the host (same ops as the device
// kernels; the whole translation unit is compiled -ffp-contract=off).
static double host_dot_f32(const float *a, const float *b, uint32_t d) {
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t i = 0;
	for (; i + 8 <= d; i += 8)
		for (uint32_t t = 0; t < 8; t++)
			p[t] += a[i + t] * b[i + t];
	float s = 0;
	s += (p[0] + p[4]);
	s += (p[1] + p[5]);
	s += (p[2] + p[6]);
	s += (p[3] + p[7]);
	for (; i < d; i++)
		s += a[i] * b[i];
	return (double)s;
}
static double host_sumsq_f32(const float *a, uint32_t d) {
	float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t i = 0;
	for (; i + 8 <= d; i += 8)
		for (uint32_t t = 0; t < 8; t++)
			p[t] += a[i + t] * a[i + t];
	float s = 0;
	s += ((p[0] + p[4]) + (p[1] + p[5]));
	s += ((p[2] + p[6]) + (p[3] + p[7]));
	for (; i < d; i++)
		s += a[i] * a[i];
	return (double)s;
}

struct Layer {
	std::vector<std::vector<uint32_t>> edges;
	uint32_t m_max;
	// graph.rs nodes-map membership: get_edges is None for absent nodes and
	// layer.remove is a no-op on them. Kept alongside `edges` (which is
	// sized to the element count for lock-striped parallel inserts).
	std::vector<uint8_t> in_layer;
	bool has(uint32_t id) const {
		return id < in_layer.size() && in_layer[id];
	}
};

} // namespace hnsw

struct sdbv_hnsw {
	sdbv_ctx *ctx;
	uint32_t d;
	uint8_t metric;
	uint32_t m, m0, efc;
	bool extend, keep;
	double ml;
	uint64_t rng_state;
	std::vector<float> vecs;    // host row-major copy (build + upper layers)
	std::vector<double> norms;  // per-element f64 norm (cosine)
	std::vector<hnsw::Layer> layers;
	// elements-map membership (hnsw/elements.rs): remove() keeps the vector
	// slot but the element no longer exists for searches
	std::vector<uint8_t> elem_present;
	bool dirty = false; // host graph changed since finalize (device stale)
	int64_t enter_point = -1;
	uint64_t next_id = 0;
	// parallel build
	std::vector<std::mutex> node_locks{4096};
	std::mutex global_mu;
	// device side (after finalize)
	uint64_t table = ~0ULL;
	bool finalized = false;
	uint32_t *rows_dev = nullptr;
	double *dout_dev = nullptr;
	float *q_dev = nullptr;
	uint32_t *rows_pinned = nullptr; // pinned host staging (per-hop latency)
	double *dists_pinned = nullptr;
	// persistent-kernel search state (device graph + row-major vectors)
	float *rm_dev = nullptr;        // [n][d] row-major
	uint32_t *offsets_dev = nullptr; // layer-0 CSR
	uint32_t *edges_dev = nullptr;
	double *norms_dev = nullptr;    // per-element f64 norm (cosine)
	uint32_t *vis_dev = nullptr;    // visited bitsets scratch
	uint64_t vis_cap = 0;
	uint32_t max_deg = 0; // actual max layer-0 degree at finalize (scratch
	                      // sizing; a parallel build can transiently exceed
	                      // m0 — see layer_insert_apply's keep-back)
	// GPU snapshot-build state (padded layer-0 adjacency, delta-updated)
	uint32_t *adj_dev = nullptr; // [n][adj_stride]
	uint32_t *deg_dev = nullptr; // [n]
	uint32_t adj_stride = 0;
	uint64_t adj_nodes = 0; // allocated node capacity of adj_dev/deg_dev
	uint64_t dev_rows = 0;  // rows of rm_dev/norms_dev currently uploaded
	// Per-layer dirty tracking for the per-chunk adjacency syncs of the
	// GPU build (v3 keeps a padded device adjacency for EVERY layer):
	// flag dedup + append-only id list, so a sync never scans all nelem
	// flags (that scan was O(nelem x chunks) — quadratic at 10M rows).
	// Only active (allocated) inside the GPU snapshot build, where layers
	// are pre-created so h->layers never reallocates under workers.
	struct DirtyTrack {
		std::vector<uint8_t> flag;
		std::vector<uint32_t> list;
		std::atomic<uint32_t> n{0};
	};
	std::vector<std::unique_ptr<DirtyTrack>> dtrack; // indexed by layer
	// flag+append; callers serialize per node (node locks / sequential
	// loops), so the flag test-and-set cannot race for one node
	inline void mark_dirty(uint32_t layer, uint32_t e) {
		if (layer >= dtrack.size() || !dtrack[layer])
			return;
		DirtyTrack &D = *dtrack[layer];
		if (D.flag[e])
			return;
		D.flag[e] = 1;
		D.list[D.n.fetch_add(1, std::memory_order_relaxed)] = e;
	}
	std::string err;
};

namespace hnsw {

static inline const float *vec(const sdbv_hnsw *h, uint32_t id) {
	return h->vecs.data() + (uint64_t)id * h->d;
}

static double dist(const sdbv_hnsw *h, const float *a, double a_norm,
                   uint32_t id) {
	if (h->metric == SDBV_METRIC_COSINE) {
		double dot = host_dot_f32(a, vec(h, id), h->d);
		return 1.0 - dot / (a_norm * h->norms[id]);
	}
	float acc = 0;
	const float *b = vec(h, id);
	for (uint32_t i = 0; i < h->d; i++) {
		float diff = a[i] - b[i];
		acc += diff * diff;
	}
	return sqrt((double)acc);
}
static double dist_ee(const sdbv_hnsw *h, uint32_t a, uint32_t b) {
	return dist(h, vec(h, a), h->metric == SDBV_METRIC_COSINE ? h->norms[a] : 0,
	            b);
}

static std::vector<uint32_t> get_edges(sdbv_hnsw *h, const Layer &layer,
                                       uint32_t id, bool locked) {
	if (!locked)
		return id < layer.edges.size() ? layer.edges[id]
		                               : std::vector<uint32_t>{};
	std::lock_guard<std::mutex> lk(h->node_locks[id & 4095]);
	return id < layer.edges.size() ? layer.edges[id] : std::vector<uint32_t>{};
}

} // namespace hnsw
struct sdbv_index; // defined below (index layer)
namespace hnsw {

// Pending-docs context for index searches (hnsw/index.rs knn path): the
// DocId bitmap from search_pendings plus the element->docs accessor.
struct IdxPend {
	const std::set<uint64_t> *pending;
	const ::sdbv_index *ix;
};
static bool idx_all_docs_pending(const IdxPend *p, uint32_t e_id);

// Epoch-stamped visited set (build hot path): O(1) insert, no per-search
// allocation or clearing. Drop-in for unordered_set<uint32_t> in
// search_layer_host (template).
struct VisitSet {
	std::vector<uint32_t> stamp;
	uint32_t epoch = 0;
	void begin(size_t n) {
		if (stamp.size() < n)
			stamp.resize(n, 0);
		if (++epoch == 0) {
			std::fill(stamp.begin(), stamp.end(), 0);
			epoch = 1;
		}
	}
	// mimics unordered_set::insert().second
	struct R {
		bool second;
	};
	R insert(uint32_t id) {
		if (id >= stamp.size())
			stamp.resize(id + 1, 0);
		if (stamp[id] == epoch)
			return {false};
		stamp[id] = epoch;
		return {true};
	}
};

// layer.rs:184-223 — host-distance variant (build path + index host path).
// `pend`: an element whose docs are ALL pending is excluded from
// `candidates` only; it still enters `w` (layer.rs:209-212, the reference
// pushes to w outside the exclusion check — restated as-is).
template <class VS>
static void search_layer_host(sdbv_hnsw *h, const Layer &layer, const float *q,
                              double q_norm, PQ &candidates, VS &visited,
                              PQ &w, uint32_t ef, bool locked,
                              const IdxPend *pend = nullptr) {
	double fq = w.peek_last_dist(DBL_MAX);
	double cd;
	uint32_t doc;
	std::vector<uint32_t> scratch; // locked-mode edge snapshot (reused)
	while (candidates.pop_first(&cd, &doc)) {
		if (cd > fq)
			break;
		const std::vector<uint32_t> *edges_p;
		if (!locked) {
			static const std::vector<uint32_t> kEmpty;
			edges_p = doc < layer.edges.size() ? &layer.edges[doc] : &kEmpty;
		} else {
			scratch.clear();
			std::lock_guard<std::mutex> lk(h->node_locks[doc & 4095]);
			if (doc < layer.edges.size())
				scratch = layer.edges[doc];
			edges_p = &scratch;
		}
		// prefetch the frontier's vectors: the expansion reads ~m0 random
		// 3 KB rows far larger than any cache level at bench scale
		for (uint32_t e : *edges_p)
			__builtin_prefetch(vec(h, e), 0, 1);
		for (uint32_t e : *edges_p) {
			if (!visited.insert(e).second)
				continue;
			// elements.get_vector -> None for removed elements
			// (layer.rs:206): dangling edges left by insert-time pruning
			// asymmetry are skipped after the visited mark
			if (e < h->elem_present.size() && !h->elem_present[e])
				continue;
			double ed = dist(h, q, q_norm, e);
			if (ed < fq || w.n < ef) {
				if (!pend || !idx_all_docs_pending(pend, e))
					candidates.push(ed, e);
				w.push(ed, e);
				if (w.n > ef)
					w.pop_last();
				fq = w.peek_last_dist(DBL_MAX);
			}
		}
	}
}

// heuristic.rs:193-216
static bool is_closer(sdbv_hnsw *h, double ed, uint32_t e,
                      std::vector<uint32_t> &r) {
	for (uint32_t rid : r)
		if (ed > dist_ee(h, e, rid))
			return false;
	r.push_back(e);
	return true;
}

// heuristic.rs:35-116 (+ extend :118-157; `ignore` = heuristic.rs:130-134,
// the element being removed is excluded from the extension set)
static void select_neighbors(sdbv_hnsw *h, const Layer &layer, uint32_t q_id,
                             const float *q_pt, double q_norm, PQ c,
                             std::vector<uint32_t> &res, bool locked,
                             int64_t ignore = -1) {
	if (h->extend) {
		std::unordered_set<uint32_t> ex;
		auto base = c.to_vec();
		for (auto &e : base)
			ex.insert(e.second);
		if (ignore >= 0)
			ex.insert((uint32_t)ignore);
		for (auto &e : base)
			for (uint32_t adj : get_edges(h, layer, e.second, locked))
				if (adj != q_id && ex.insert(adj).second) {
					// get_distance -> None for removed elements
					if (adj < h->elem_present.size() &&
					    !h->elem_present[adj])
						continue;
					c.push(dist(h, q_pt, q_norm, adj), adj);
				}
	}
	uint32_t m_max = layer.m_max;
	if (c.n <= m_max) {
		for (auto &e : c.to_vec())
			res.push_back(e.second);
		return;
	}
	std::vector<uint32_t> pruned;
	double ed;
	uint32_t e;
	while (c.pop_first(&ed, &e)) {
		if (is_closer(h, ed, e, res)) {
			if (res.size() == m_max)
				break;
		} else if (h->keep) {
			pruned.push_back(e);
		}
	}
	if (h->keep) {
		size_t nmore = m_max - res.size();
		for (size_t i = 0; i < nmore && i < pruned.size(); i++)
			res.push_back(pruned[i]);
	}
}

// layer.rs:342-387
// The insert's apply half (select + bidirectional edges + prunes) over a
// precomputed candidate window `w` — shared by the classic insert (whose
// search ran just now) and the chunked snapshot build (whose search ran
// against the pre-chunk graph; see sdbv_hnsw_insert_batch_snapshot).
static void layer_insert_apply(sdbv_hnsw *h, Layer &layer, uint32_t q_id,
                               const float *q_pt, double q_norm, PQ w,
                               bool locked) {
	// device-adjacency dirty marking for the GPU build's classic-path
	// inserts (no-op unless a build allocated dtrack for this layer);
	// layers never reallocates during builds, so the index is stable
	const uint32_t li = (uint32_t)(&layer - h->layers.data());
	std::vector<uint32_t> neighbors;
	select_neighbors(h, layer, q_id, q_pt, q_norm, std::move(w), neighbors,
	                 locked);
	{
		// append (not overwrite): a concurrent inserter may already have
		// back-linked into q_id; sequential mode this is plain assignment
		std::lock_guard<std::mutex> lk(h->node_locks[q_id & 4095]);
		auto &eq = layer.edges[q_id];
		for (uint32_t e : neighbors)
			if (e != q_id &&
			    std::find(eq.begin(), eq.end(), e) == eq.end())
				eq.push_back(e);
		h->mark_dirty(li, q_id);
	}
	for (uint32_t e : neighbors) {
		if (e == q_id)
			continue;
		std::vector<uint32_t> conn;
		{
			std::lock_guard<std::mutex> lk(h->node_locks[e & 4095]);
			// graph.rs:52-64: the back-edge entry().or_insert IMPLICITLY
			// creates a missing target node (e.g. an upper-layer seed)
			if (e < layer.in_layer.size())
				layer.in_layer[e] = 1;
			auto &ee = layer.edges[e];
			if (std::find(ee.begin(), ee.end(), q_id) == ee.end()) {
				ee.push_back(q_id);
				h->mark_dirty(li, e);
			}
			if (ee.size() > layer.m_max)
				conn = ee;
		}
		if (!conn.empty()) {
			// prune (layer.rs:363-377) — distances computed outside the
			// lock. build_priority_list (layer.rs:389-404) SKIPS removed
			// elements (get_vector -> None), so a prune also cleanses any
			// dangling edges out of e's list.
			PQ ec;
			for (uint32_t nid : conn) {
				if (nid < h->elem_present.size() && !h->elem_present[nid])
					continue;
				ec.push(dist_ee(h, e, nid), nid);
			}
			std::vector<uint32_t> enew;
			select_neighbors(h, layer, e, vec(h, e),
			                 h->metric == SDBV_METRIC_COSINE ? h->norms[e] : 0,
			                 std::move(ec), enew, locked);
			std::lock_guard<std::mutex> lk(h->node_locks[e & 4095]);
			// keep any back-edges another inserter added since the snapshot
			// (parallel mode only; sequential sees none)
			for (uint32_t cur : layer.edges[e])
				if (std::find(conn.begin(), conn.end(), cur) == conn.end() &&
				    std::find(enew.begin(), enew.end(), cur) == enew.end())
					enew.push_back(cur);
			layer.edges[e] = enew;
			h->mark_dirty(li, e);
		}
	}
}

static PQ layer_insert(sdbv_hnsw *h, Layer &layer, uint32_t q_id,
                       const float *q_pt, double q_norm, PQ eps, bool locked) {
	PQ w = eps;
	static thread_local VisitSet visited;
	visited.begin(h->vecs.size() / h->d);
	for (auto &e : eps.to_vec())
		visited.insert(e.second);
	search_layer_host(h, layer, q_pt, q_norm, eps, visited, w, h->efc, locked);
	PQ out = w;
	layer_insert_apply(h, layer, q_id, q_pt, q_norm, std::move(w), locked);
	return out;
}

// hnsw/mod.rs:263-266 (level RNG restatement — same contract as the oracle)
static inline uint64_t splitmix_host(uint64_t z) {
	z += 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}
static uint32_t next_level(sdbv_hnsw *h) {
	h->rng_state = splitmix_host(h->rng_state);
	double u = (double)(h->rng_state >> 11) * 0x1.0p-53;
	if (u <= 0.0)
		u = 0x1.0p-53;
	double lvl = std::floor(-std::log(u) * h->ml);
	return (uint32_t)std::min(std::max(lvl, 0.0), 30.0);
}

// hnsw/mod.rs:230-394 insert at a given level (vector already appended)
static void insert_at(sdbv_hnsw *h, uint32_t q_id, uint32_t q_level,
                      bool locked) {
	const float *q_pt = vec(h, q_id);
	double q_norm = h->metric == SDBV_METRIC_COSINE ? h->norms[q_id] : 0;
	uint32_t top_up;
	{
		std::lock_guard<std::mutex> lk(h->global_mu);
		top_up = (uint32_t)h->layers.size() - 1;
		for (uint32_t i = top_up; i < q_level; i++)
			h->layers.push_back(hnsw::Layer{
			    std::vector<std::vector<uint32_t>>(h->vecs.size() / h->d),
			    h->m});
		uint64_t nelem = h->vecs.size() / h->d;
		for (auto &l : h->layers) {
			if (l.edges.size() <= q_id)
				l.edges.resize(nelem);
			if (l.in_layer.size() < nelem)
				l.in_layer.resize(nelem, 0);
		}
		// node membership on layers 0..=q_level (graph.rs add_node /
		// add_empty_node in insert_first_element and insert_element)
		for (uint32_t l = 0;
		     l < (uint32_t)h->layers.size() && l <= q_level; l++)
			h->layers[l].in_layer[q_id] = 1;
		h->dirty = true;
		if (h->enter_point < 0) {
			h->enter_point = q_id;
			return;
		}
	}
	uint64_t ep_id = (uint64_t)h->enter_point;
	double ep_dist = dist(h, q_pt, q_norm, (uint32_t)ep_id);
	if (q_level < top_up) {
		for (uint32_t l = top_up; l > q_level; l--) {
			PQ cand;
			cand.push(ep_dist, (uint32_t)ep_id);
			std::unordered_set<uint32_t> visited{(uint32_t)ep_id};
			PQ w = cand;
			search_layer_host(h, h->layers[l], q_pt, q_norm, cand, visited, w,
			                  1, locked);
			double dd;
			uint32_t ii;
			if (w.peek_first(&dd, &ii)) {
				ep_dist = dd;
				ep_id = ii;
			}
		}
	}
	PQ eps;
	eps.push(ep_dist, (uint32_t)ep_id);
	uint32_t ins_to = std::min(q_level, top_up);
	for (uint32_t l = ins_to; l >= 1; l--)
		eps = layer_insert(h, h->layers[l], q_id, q_pt, q_norm, std::move(eps),
		                   locked);
	layer_insert(h, h->layers[0], q_id, q_pt, q_norm, std::move(eps), locked);
	if (q_level > top_up) {
		std::lock_guard<std::mutex> lk(h->global_mu);
		h->enter_point = q_id;
	}
}

// Chunked SNAPSHOT searches (the §8f-rank-3 structure): per chunk, every
// element's efc-search runs against the graph AS OF the chunk start
// (read-only — no locks, embarrassingly parallel; the GPU build batches
// the same searches onto the persistent kernel).

// Upper-layer greedy descent only (host half shared by the CPU and GPU
// snapshot paths); returns the layer-0 entry point + distance.
static void snapshot_descend_one(sdbv_hnsw *h, uint32_t q_id, double q_norm,
                                 uint32_t *ep_out, double *epd_out) {
	const float *q_pt = vec(h, q_id);
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q_pt, q_norm, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q_pt, q_norm, cand, visited, w,
		                  1, false);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}
	*ep_out = ep_id;
	*epd_out = ep_dist;
}

static void snapshot_search_one(sdbv_hnsw *h, uint32_t q_id, PQ &w_out) {
	const float *q_pt = vec(h, q_id);
	double q_norm = h->metric == SDBV_METRIC_COSINE ? h->norms[q_id] : 0;
	uint32_t ep_id;
	double ep_dist;
	snapshot_descend_one(h, q_id, q_norm, &ep_id, &ep_dist);
	PQ eps;
	eps.push(ep_dist, ep_id);
	PQ w = eps;
	static thread_local VisitSet visited;
	visited.begin(h->vecs.size() / h->d);
	visited.insert(ep_id);
	search_layer_host(h, h->layers[0], q_pt, q_norm, eps, visited, w,
	                  h->efc, false);
	w_out = std::move(w);
}

// ef-search at ANY layer from a given eps window (the insert path's
// multi-ep seeding, layer.rs:342-358) against the snapshot graph.
static void snapshot_search_layer_eps(sdbv_hnsw *h, uint32_t layer_idx,
                                      uint32_t q_id, const PQ &eps_in,
                                      uint32_t ef, PQ &w_out) {
	const float *q_pt = vec(h, q_id);
	double q_norm = h->metric == SDBV_METRIC_COSINE ? h->norms[q_id] : 0;
	PQ eps = eps_in;
	PQ w = eps;
	static thread_local VisitSet visited;
	visited.begin(h->vecs.size() / h->d);
	for (auto &e : eps_in.to_vec())
		visited.insert(e.second);
	search_layer_host(h, h->layers[layer_idx], q_pt, q_norm, eps, visited,
	                  w, ef, false);
	w_out = std::move(w);
}

// Greedy descent through layers top..2 only (ef=1; the layer-1 hop is the
// batched builds' device work).
static void descend_to_layer2(sdbv_hnsw *h, uint32_t q_id, double q_norm,
                              uint32_t *ep_out, double *epd_out) {
	const float *q_pt = vec(h, q_id);
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q_pt, q_norm, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 2; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q_pt, q_norm, cand, visited, w,
		                  1, false);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}
	*ep_out = ep_id;
	*epd_out = ep_dist;
}

// ---- batched per-layer apply (snapshot-build v3) ----
// The same select/prune algorithm as layer_insert_apply, but in three
// bulk phases per chunk AND PER LAYER: (A) every element's neighbour
// select against the post-search graph, read-only and parallel; (B) all
// edge appends, in element order, sequential (deterministic and cheap);
// (C) one prune pass over every node that ended over m_max, parallel
// (prunes are independent: enew ⊆ conn, no cascading). This is ONE valid
// serialization of the parallel interleaved apply — same algorithm, a
// fixed schedule — and the form whose distance work (the RAM-bound part)
// batches onto the device in the GPU build. Quality is pinned by the same
// recall bars; the GPU twin must match this host twin bit-exactly.
struct ApplyItem {
	uint32_t q_id;
	PQ w;
	std::vector<uint32_t> neighbors; // phase-A output
};

static std::vector<uint32_t> batched_apply_phaseB(sdbv_hnsw *h,
                                                  uint32_t layer_idx,
                                                  std::vector<ApplyItem *> &it);
static void batched_apply_phaseC_host(sdbv_hnsw *h, uint32_t layer_idx,
                                      const std::vector<uint32_t> &overfull,
                                      int nthreads);

// host phase A + B + C (the twin's apply; the GPU build replaces A and C
// with k_pair_mats/k_heur_select)
static void batched_apply_host(sdbv_hnsw *h, uint32_t layer_idx,
                               std::vector<ApplyItem *> &items,
                               int nthreads) {
	Layer &L = h->layers[layer_idx];
	// phase A: selects (read-only graph)
	{
		std::atomic<uint64_t> cursor{0};
		auto worker = [&]() {
			uint64_t j;
			while ((j = cursor.fetch_add(1)) < items.size()) {
				ApplyItem &it = *items[j];
				const float *q_pt = vec(h, it.q_id);
				double q_norm = h->metric == SDBV_METRIC_COSINE
				                    ? h->norms[it.q_id]
				                    : 0;
				it.neighbors.clear();
				select_neighbors(h, L, it.q_id, q_pt, q_norm, it.w,
				                 it.neighbors, false);
			}
		};
		std::vector<std::thread> ts;
		int nt = std::max(1, std::min<int>(nthreads, (int)items.size()));
		for (int t = 1; t < nt; t++)
			ts.emplace_back(worker);
		worker();
		for (auto &t : ts)
			t.join();
	}
	auto overfull = batched_apply_phaseB(h, layer_idx, items);
	batched_apply_phaseC_host(h, layer_idx, overfull, nthreads);
}

// phase B: appends, element order (graph.rs:52-64 entry().or_insert —
// including the implicit creation of a missing back-edge target, e.g. an
// eps node from the layer above that is not a member of THIS layer);
// returns the deduped list of nodes that ended over m_max (prune targets)
static std::vector<uint32_t> batched_apply_phaseB(sdbv_hnsw *h,
                                                  uint32_t layer_idx,
                                                  std::vector<ApplyItem *> &items) {
	Layer &L = h->layers[layer_idx];
	std::vector<uint32_t> overfull;
	for (auto *itp : items) {
		auto &it = *itp;
		auto &eq = L.edges[it.q_id];
		for (uint32_t e : it.neighbors)
			if (e != it.q_id &&
			    std::find(eq.begin(), eq.end(), e) == eq.end())
				eq.push_back(e);
		L.in_layer[it.q_id] = 1;
		h->mark_dirty(layer_idx, it.q_id);
	}
	for (auto *itp : items) {
		auto &it = *itp;
		for (uint32_t e : it.neighbors) {
			if (e == it.q_id)
				continue;
			auto &ee = L.edges[e];
			if (e < L.in_layer.size())
				L.in_layer[e] = 1;
			if (std::find(ee.begin(), ee.end(), it.q_id) == ee.end()) {
				ee.push_back(it.q_id);
				if (ee.size() > L.m_max)
					overfull.push_back(e); // deduped below
				h->mark_dirty(layer_idx, e);
			}
		}
	}
	std::sort(overfull.begin(), overfull.end());
	overfull.erase(std::unique(overfull.begin(), overfull.end()),
	               overfull.end());
	return overfull;
}

// phase C: prunes (layer.rs:363-377), parallel over distinct nodes
static void batched_apply_phaseC_host(sdbv_hnsw *h, uint32_t layer_idx,
                                      const std::vector<uint32_t> &overfull,
                                      int nthreads) {
	Layer &L = h->layers[layer_idx];
	std::atomic<uint64_t> cursor{0};
	auto worker = [&]() {
		uint64_t i;
		while ((i = cursor.fetch_add(1)) < overfull.size()) {
			uint32_t e = overfull[i];
			const auto conn = L.edges[e]; // copy (read-only source)
			PQ ec;
			for (uint32_t nid : conn) {
				if (nid < h->elem_present.size() &&
				    !h->elem_present[nid])
					continue;
				ec.push(dist_ee(h, e, nid), nid);
			}
			std::vector<uint32_t> enew;
			select_neighbors(h, L, e, vec(h, e),
			                 h->metric == SDBV_METRIC_COSINE
			                     ? h->norms[e]
			                     : 0,
			                 std::move(ec), enew, false);
			L.edges[e] = enew;
			h->mark_dirty(layer_idx, e);
		}
	};
	std::vector<std::thread> ts;
	int nt = std::max(1, std::min<int>(nthreads,
	                                   (int)std::max<size_t>(overfull.size(),
	                                                         1)));
	for (int t = 1; t < nt; t++)
		ts.emplace_back(worker);
	worker();
	for (auto &t : ts)
		t.join();
}

// ---- graph element removal (sequential only: apply_pendings holds the
// reference's write lock; the parallel bench-mode build never removes) ----

// layer.rs:92-108 search_single_with_ignore: seeded FROM the ignored
// element; returns the closest found element or -1 (None).
static int64_t search_single_with_ignore(sdbv_hnsw *h, const Layer &layer,
                                         const float *pt, double pt_norm,
                                         uint32_t ignore_id, uint32_t ef) {
	std::unordered_set<uint32_t> visited{ignore_id};
	PQ candidates;
	candidates.push(dist(h, pt, pt_norm, ignore_id), ignore_id);
	PQ w;
	search_layer_host(h, layer, pt, pt_norm, candidates, visited, w, ef,
	                  false);
	double dd;
	uint32_t ii;
	if (w.peek_first(&dd, &ii))
		return (int64_t)ii;
	return -1;
}

// layer.rs:164-181 search_multi_with_ignore.
static PQ search_multi_with_ignore(sdbv_hnsw *h, const Layer &layer,
                                   const float *pt, double pt_norm,
                                   const std::vector<uint32_t> &ignore_ids,
                                   uint32_t efc) {
	PQ candidates;
	for (uint32_t id : ignore_ids)
		candidates.push(dist(h, pt, pt_norm, id), id);
	std::unordered_set<uint32_t> visited(ignore_ids.begin(),
	                                     ignore_ids.end());
	PQ w;
	search_layer_host(h, layer, pt, pt_norm, candidates, visited, w, efc,
	                  false);
	return w;
}

// layer.rs:408-460 HnswLayer::remove: drop node + back-edges, then repair
// each former neighbour (efc-search ignoring {q_id, e_id}, heuristic
// re-selection with ignore=e_id, one-directional set_node).
static bool layer_remove(sdbv_hnsw *h, Layer &layer, uint32_t e_id) {
	if (!layer.has(e_id))
		return false;
	std::vector<uint32_t> f_ids = std::move(layer.edges[e_id]);
	layer.edges[e_id].clear();
	layer.in_layer[e_id] = 0;
	for (uint32_t f : f_ids) {
		auto &fe = layer.edges[f];
		fe.erase(std::remove(fe.begin(), fe.end(), e_id), fe.end());
	}
	for (uint32_t q_id : f_ids) {
		const float *q_pt = vec(h, q_id);
		double q_norm =
		    h->metric == SDBV_METRIC_COSINE ? h->norms[q_id] : 0;
		PQ c = search_multi_with_ignore(h, layer, q_pt, q_norm,
		                                {q_id, e_id}, h->efc);
		std::vector<uint32_t> q_new_conn;
		select_neighbors(h, layer, q_id, q_pt, q_norm, std::move(c),
		                 q_new_conn, false, (int64_t)e_id);
		layer.edges[q_id] = q_new_conn; // graph.set_node
	}
	return true;
}

// hnsw/mod.rs:398-455 Hnsw::remove.
static bool hnsw_remove(sdbv_hnsw *h, uint32_t e_id) {
	if (e_id >= h->next_id || !h->elem_present[e_id])
		return false; // elements.get_vector -> None
	bool removed = false;
	const float *e_pt = vec(h, e_id);
	double e_norm = h->metric == SDBV_METRIC_COSINE ? h->norms[e_id] : 0;
	int64_t new_ep = ((int64_t)e_id == h->enter_point) ? -1 : h->enter_point;
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		if (new_ep < 0)
			new_ep = search_single_with_ignore(h, h->layers[l], e_pt,
			                                   e_norm, e_id, h->efc);
		if (layer_remove(h, h->layers[l], e_id))
			removed = true;
	}
	if (new_ep < 0)
		new_ep = search_single_with_ignore(h, h->layers[0], e_pt, e_norm,
		                                   e_id, h->efc);
	if (layer_remove(h, h->layers[0], e_id))
		removed = true;
	h->elem_present[e_id] = 0; // elements.remove
	h->enter_point = new_ep;
	h->dirty = true;
	return removed;
}

} // namespace hnsw

extern "C" {

// Host-side synthetic generator (same committed bit contract as k_gen_cm and
// the oracle); parallel over rows. Input prep for benches/tests — no GPU.
void sdbv_gen_f32(uint64_t seed, uint64_t row0, uint64_t nrows, uint32_t d,
                  float *out) {
	int nthreads = (int)std::thread::hardware_concurrency();
	if (nthreads < 1)
		nthreads = 1;
	if (nrows < 4096)
		nthreads = 1;
	std::vector<std::thread> ws;
	std::atomic<uint64_t> next{0};
	auto work = [&] {
		for (;;) {
			uint64_t i = next.fetch_add(4096);
			if (i >= nrows)
				break;
			uint64_t end = std::min(nrows, i + 4096);
			for (uint64_t r = i; r < end; r++)
				for (uint32_t j = 0; j < d; j++)
					out[r * d + j] =
					    d_gen_elem(seed, (row0 + r) * (uint64_t)d + j);
		}
	};
	for (int w = 0; w < nthreads - 1; w++)
		ws.emplace_back(work);
	work();
	for (auto &w : ws)
		w.join();
}

int sdbv_hnsw_create(sdbv_ctx *ctx, uint32_t d, uint8_t metric, uint32_t m,
                     uint32_t m0, uint32_t efc, int extend, int keep,
                     uint64_t seed, double ml, sdbv_hnsw **out) {
	// ctx may be NULL for a host-only (build/export) index; finalize and
	// knn require a context and fail loudly without one.
	if (d == 0 || d > MAX_D || (d % 4) != 0 ||
	    metric > SDBV_METRIC_EUCLIDEAN || m == 0 || m0 == 0)
		return SDBV_ERR_BAD_ARG;
	auto *h = new sdbv_hnsw();
	h->ctx = ctx;
	h->d = d;
	h->metric = metric;
	h->m = m;
	h->m0 = m0;
	h->efc = efc;
	h->extend = extend != 0;
	h->keep = keep != 0;
	h->ml = ml;
	h->rng_state = seed;
	h->layers.push_back(hnsw::Layer{{}, m0});
	*out = h;
	return SDBV_OK;
}

void sdbv_hnsw_destroy(sdbv_hnsw *h) {
	if (!h)
		return;
	if (h->rows_dev)
		(void)hipFree(h->rows_dev);
	if (h->dout_dev)
		(void)hipFree(h->dout_dev);
	if (h->q_dev)
		(void)hipFree(h->q_dev);
	if (h->rows_pinned)
		(void)hipHostFree(h->rows_pinned);
	if (h->dists_pinned)
		(void)hipHostFree(h->dists_pinned);
	for (void *p : {(void *)h->rm_dev, (void *)h->offsets_dev,
	                (void *)h->edges_dev, (void *)h->norms_dev,
	                (void *)h->vis_dev})
		if (p)
			(void)hipFree(p);
	delete h;
}

static void hnsw_free_device_state(sdbv_hnsw *h); // defined below finalize

static void hnsw_append_vec(sdbv_hnsw *h, const float *pt) {
	h->vecs.insert(h->vecs.end(), pt, pt + h->d);
	h->elem_present.push_back(1);
	if (h->metric == SDBV_METRIC_COSINE)
		h->norms.push_back(sqrt(hnsw::host_sumsq_f32(pt, h->d)));
}

int sdbv_hnsw_insert(sdbv_hnsw *h, const float *pt) {
	if (!h)
		return SDBV_ERR_BAD_ARG;
	// Writes on a finalized graph invalidate the device copy (same contract
	// as hnsw_remove): drop it and let the next search re-finalize. The
	// round-1 BAD_ARG guard here made idx_vd_insert silently skip the graph
	// insert for every update applied after a GPU search (driver GPUTEST_r01
	// failure: updated doc missing from post-apply top-K).
	if (h->finalized) {
		hnsw_free_device_state(h);
		h->dirty = true;
	}
	uint32_t q_id = (uint32_t)h->next_id++;
	hnsw_append_vec(h, pt);
	hnsw::insert_at(h, q_id, hnsw::next_level(h), /*locked=*/false);
	return SDBV_OK;
}

int sdbv_hnsw_insert_batch(sdbv_hnsw *h, const float *pts, uint64_t n,
                           int nthreads) {
	if (!h || h->finalized)
		return SDBV_ERR_BAD_ARG;
	if (nthreads <= 0)
		nthreads = (int)std::thread::hardware_concurrency();
	if (nthreads <= 1) {
		for (uint64_t i = 0; i < n; i++) {
			int rc = sdbv_hnsw_insert(h, pts + i * h->d);
			if (rc)
				return rc;
		}
		return SDBV_OK;
	}
	uint64_t base = h->next_id;
	// levels drawn deterministically per ordinal (sequential RNG)
	std::vector<uint32_t> levels(n);
	for (uint64_t i = 0; i < n; i++)
		levels[i] = hnsw::next_level(h);
	h->vecs.reserve(h->vecs.size() + n * h->d);
	for (uint64_t i = 0; i < n; i++)
		hnsw_append_vec(h, pts + i * h->d);
	h->next_id += n;
	// pre-size every layer to the final element count (no growth races)
	{
		uint32_t maxl = 0;
		for (auto l : levels)
			maxl = std::max(maxl, l);
		std::lock_guard<std::mutex> lk(h->global_mu);
		while (h->layers.size() <= maxl)
			h->layers.push_back(hnsw::Layer{{}, h->m});
		for (auto &l : h->layers)
			l.edges.resize(h->next_id);
	}
	// the first elements (empty/near-empty graph) go in alone so every
	// worker sees a connected entry point
	uint64_t start = 0;
	uint64_t warm = std::min<uint64_t>(n, h->enter_point < 0 ? 64 : 0);
	for (; start < warm; start++)
		hnsw::insert_at(h, (uint32_t)(base + start), levels[start], true);
	std::atomic<uint64_t> next{start};
	std::vector<std::thread> workers;
	for (int w = 0; w < nthreads; w++)
		workers.emplace_back([&] {
			for (;;) {
				uint64_t i = next.fetch_add(1);
				if (i >= n)
					break;
				hnsw::insert_at(h, (uint32_t)(base + i), levels[i], true);
			}
		});
	for (auto &w : workers)
		w.join();
	// Promote the enter point to a max-level element of this batch: with
	// pre-created layers insert_at's q_level > top_up promotion never
	// fires, which would leave the upper layers unreachable from a
	// level-0 enter point (greedy descents would pass through them).
	{
		uint32_t maxl = 0;
		for (auto l : levels)
			maxl = std::max(maxl, l);
		std::lock_guard<std::mutex> lk(h->global_mu);
		uint32_t cur_top = (uint32_t)h->layers.size() - 1;
		if (h->enter_point >= 0 && maxl >= cur_top &&
		    !h->layers[cur_top].has((uint32_t)h->enter_point)) {
			for (uint64_t i = 0; i < n; i++)
				if (levels[i] == maxl) {
					h->enter_point = (int64_t)(base + i);
					break;
				}
		}
	}
	return SDBV_OK;
}

// Chunked snapshot build (see hnsw::snapshot_search_one above):
int sdbv_hnsw_insert_batch_snapshot(sdbv_hnsw *h, const float *pts,
                                    uint64_t n, uint32_t chunk,
                                    int nthreads) {
	using namespace hnsw;
	if (!h || h->finalized || chunk == 0)
		return SDBV_ERR_BAD_ARG;
	if (nthreads <= 0)
		nthreads = (int)std::thread::hardware_concurrency();
	uint64_t base = h->next_id;
	std::vector<uint32_t> levels(n);
	for (uint64_t i = 0; i < n; i++)
		levels[i] = next_level(h); // sequential RNG contract, per ordinal
	h->next_id += n;
	for (uint64_t i = 0; i < n; i++)
		hnsw_append_vec(h, pts + i * h->d);
	// pre-create every layer the batch will need and size them up front:
	// concurrent insert_at must never grow h->layers (vector reallocation
	// under readers — same discipline as the classic parallel batch path)
	{
		std::lock_guard<std::mutex> lk(h->global_mu);
		uint32_t max_level = 0;
		for (uint64_t i = 0; i < n; i++)
			max_level = std::max(max_level, levels[i]);
		while (h->layers.size() <= max_level)
			h->layers.push_back(hnsw::Layer{{}, h->m});
		uint64_t nelem = h->vecs.size() / h->d;
		for (auto &l : h->layers) {
			if (l.edges.size() < nelem)
				l.edges.resize(nelem);
			if (l.in_layer.size() < nelem)
				l.in_layer.resize(nelem, 0);
		}
	}
	for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
		uint64_t c1 = std::min(n, c0 + chunk);
		// upper-level elements first (~1/m of the chunk) so the layer
		// structure exists before the snapshot searches; inserted with the
		// classic parallel path (striped locks) — the first element of an
		// empty graph goes alone to establish the enter point
		std::vector<uint64_t> upper, flat;
		for (uint64_t i = c0; i < c1; i++) {
			if (h->enter_point < 0)
				insert_at(h, (uint32_t)(base + i), levels[i], false);
			else if (levels[i] > 0)
				upper.push_back(i);
			else
				flat.push_back(i);
		}
		if (!upper.empty()) {
			std::atomic<uint64_t> ucursor{0};
			auto upper_worker = [&]() {
				uint64_t j;
				while ((j = ucursor.fetch_add(1)) < upper.size())
					insert_at(h, (uint32_t)(base + upper[j]),
					          levels[upper[j]], true);
			};
			std::vector<std::thread> ts;
			int nt = std::max(1, std::min<int>(nthreads,
			                                   (int)upper.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(upper_worker);
			upper_worker();
			for (auto &t : ts)
				t.join();
		}
		// snapshot searches: read-only graph, parallel, no locks
		std::vector<PQ> ws(flat.size());
		std::atomic<uint64_t> cursor{0};
		auto search_worker = [&]() {
			uint64_t j;
			while ((j = cursor.fetch_add(1)) < flat.size())
				snapshot_search_one(h, (uint32_t)(base + flat[j]), ws[j]);
		};
		{
			std::vector<std::thread> ts;
			int nt = std::max(1, std::min<int>(nthreads,
			                                   (int)flat.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(search_worker);
			search_worker();
			for (auto &t : ts)
				t.join();
		}
		// apply phase: striped node locks, parallel (the parallel build's
		// existing concurrency contract)
		for (uint64_t j : flat)
			h->layers[0].in_layer[base + j] = 1;
		std::atomic<uint64_t> acursor{0};
		auto apply_worker = [&]() {
			uint64_t j;
			while ((j = acursor.fetch_add(1)) < flat.size()) {
				uint32_t q_id = (uint32_t)(base + flat[j]);
				const float *q_pt = vec(h, q_id);
				double q_norm = h->metric == SDBV_METRIC_COSINE
				                    ? h->norms[q_id]
				                    : 0;
				layer_insert_apply(h, h->layers[0], q_id, q_pt, q_norm,
				                   std::move(ws[j]), true);
			}
		};
		{
			std::vector<std::thread> ts;
			int nt = std::max(1, std::min<int>(nthreads,
			                                   (int)flat.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(apply_worker);
			apply_worker();
			for (auto &t : ts)
				t.join();
		}
	}
	h->dirty = true;
	return SDBV_OK;
}

// Enter-point reachability fix shared by the batch builds (the classic
// parallel build's promotion, generalized): with pre-created layers the
// insert-time promotion never fires, which can leave the upper layers
// unreachable from a level-0 enter point; promote any top-layer member.
static void hnsw_promote_ep(sdbv_hnsw *h) {
	using namespace hnsw;
	if (h->enter_point < 0 || h->layers.size() < 2)
		return;
	std::lock_guard<std::mutex> lk(h->global_mu);
	uint32_t top = (uint32_t)h->layers.size() - 1;
	// the top non-empty layer
	while (top >= 1) {
		const auto &in = h->layers[top].in_layer;
		if (h->layers[top].has((uint32_t)h->enter_point))
			return;
		for (uint64_t i = 0; i < in.size(); i++)
			if (in[i]) {
				h->enter_point = (int64_t)i;
				return;
			}
		top--; // layer empty (pre-created): look lower
	}
}

// Host twin of the GPU batched-apply snapshot build ("snapshot2", v3):
// the full reference insert algorithm with a fixed batched schedule at
// EVERY layer. Per chunk, top-down through the layers: each element
// either greedy-descends (ef=1, layers above its level — search_ep,
// hnsw/mod.rs:521-548) or runs the efc-search whose w both seeds the
// next layer (layer.rs:358's cascade) and feeds the batched apply
// (select/append/prune) at that layer; layer 0 takes every element.
// Searches see the graph as of the chunk start (snapshot semantics at
// every layer — the same chunk/n quality relaxation the v1 snapshot
// build pinned with recall bars). This is the bit-exact CPU reference
// for sdbv_hnsw_insert_batch_snapshot_gpu.
int sdbv_hnsw_insert_batch_snapshot2(sdbv_hnsw *h, const float *pts,
                                     uint64_t n, uint32_t chunk,
                                     int nthreads) {
	using namespace hnsw;
	if (!h || h->finalized || chunk == 0 || n == 0)
		return SDBV_ERR_BAD_ARG;
	if (nthreads <= 0)
		nthreads = (int)std::thread::hardware_concurrency();
	uint64_t base = h->next_id;
	std::vector<uint32_t> levels(n);
	for (uint64_t i = 0; i < n; i++)
		levels[i] = next_level(h); // sequential RNG contract, per ordinal
	h->next_id += n;
	h->vecs.reserve(h->vecs.size() + n * h->d);
	for (uint64_t i = 0; i < n; i++)
		hnsw_append_vec(h, pts + i * h->d);
	{
		std::lock_guard<std::mutex> lk(h->global_mu);
		uint32_t max_level = 0;
		for (uint64_t i = 0; i < n; i++)
			max_level = std::max(max_level, levels[i]);
		while (h->layers.size() <= max_level)
			h->layers.push_back(hnsw::Layer{{}, h->m});
		uint64_t ne = h->vecs.size() / h->d;
		for (auto &l : h->layers) {
			if (l.edges.size() < ne)
				l.edges.resize(ne);
			if (l.in_layer.size() < ne)
				l.in_layer.resize(ne, 0);
		}
	}
	const uint32_t top = (uint32_t)h->layers.size() - 1;
	(void)top;
	// warm-up (the classic parallel build's bootstrap): while the graph is
	// near-empty every batched element can only select the enter point,
	// whose single prune then orphans most of them — the first elements
	// go in classically so batching starts on a connected graph
	const uint64_t warm_until =
	    h->enter_point < 0 ? base + 64 : 0;
	for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
		uint64_t c1 = std::min(n, c0 + chunk);
		std::vector<ApplyItem> items;
		std::vector<PQ> eps_of;
		std::vector<uint32_t> lvl_of;
		std::vector<std::pair<uint32_t, uint32_t>> upper2; // (q_id, level)
		for (uint64_t i = c0; i < c1; i++) {
			if (h->enter_point < 0 || base + i < warm_until) {
				insert_at(h, (uint32_t)(base + i), levels[i], false);
				continue;
			}
			if (levels[i] >= 2) {
				// levels >= 2 (0.4% of elements): FULL classic inserts —
				// progressive at every layer. Half-inserted elements must
				// never be search-visible: a descent terminating on a
				// node without lower-layer edges gives a degenerate ep
				// (measured: out-degree-1 orphans, recall cliff)
				upper2.push_back({(uint32_t)(base + i), levels[i]});
				continue;
			}
			items.push_back(ApplyItem{(uint32_t)(base + i), PQ{}, {}});
			eps_of.emplace_back();
			lvl_of.push_back(levels[i]);
		}
		if (!upper2.empty()) {
			std::atomic<uint64_t> cursor{0};
			auto worker = [&]() {
				uint64_t j;
				while ((j = cursor.fetch_add(1)) < upper2.size())
					insert_at(h, upper2[j].first, upper2[j].second, true);
			};
			std::vector<std::thread> ts;
			int nt = std::max(1,
			                  std::min<int>(nthreads, (int)upper2.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(worker);
			worker();
			for (auto &t : ts)
				t.join();
		}
		if (items.empty())
			continue;
		// levels <= 1: greedy descents through layers top..2 (read-only)
		{
			std::atomic<uint64_t> cursor{0};
			auto worker = [&]() {
				uint64_t j;
				while ((j = cursor.fetch_add(1)) < items.size()) {
					uint32_t q_id = items[j].q_id;
					double qn = h->metric == SDBV_METRIC_COSINE
					                ? h->norms[q_id]
					                : 0;
					uint32_t ep;
					double epd;
					descend_to_layer2(h, q_id, qn, &ep, &epd);
					eps_of[j].push(epd, ep);
				}
			};
			std::vector<std::thread> ts;
			int nt = std::max(1,
			                  std::min<int>(nthreads, (int)items.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(worker);
			worker();
			for (auto &t : ts)
				t.join();
		}
		// layer 1 (batched): search phase (snapshot, parallel), then the
		// apply for every element with level >= 1
		if (h->layers.size() >= 2) {
			{
				std::atomic<uint64_t> cursor{0};
				auto worker = [&]() {
					uint64_t j;
					while ((j = cursor.fetch_add(1)) < items.size()) {
						uint32_t q_id = items[j].q_id;
						if (lvl_of[j] >= 1) {
							snapshot_search_layer_eps(
							    h, 1, q_id, eps_of[j], h->efc,
							    items[j].w);
							eps_of[j] = items[j].w; // cascade
						} else {
							PQ w;
							snapshot_search_layer_eps(
							    h, 1, q_id, eps_of[j], 1, w);
							double dd;
							uint32_t ii;
							if (w.peek_first(&dd, &ii)) {
								PQ ne2;
								ne2.push(dd, ii);
								eps_of[j] = std::move(ne2);
							}
						}
					}
				};
				std::vector<std::thread> ts;
				int nt = std::max(
				    1, std::min<int>(nthreads, (int)items.size()));
				for (int t = 1; t < nt; t++)
					ts.emplace_back(worker);
				worker();
				for (auto &t : ts)
					t.join();
			}
			std::vector<ApplyItem *> ins;
			for (uint64_t j = 0; j < items.size(); j++)
				if (lvl_of[j] >= 1)
					ins.push_back(&items[j]);
			if (!ins.empty())
				batched_apply_host(h, 1, ins, nthreads);
		}
		// layer 0: every element
		{
			std::atomic<uint64_t> cursor{0};
			auto worker = [&]() {
				uint64_t j;
				while ((j = cursor.fetch_add(1)) < items.size())
					snapshot_search_layer_eps(h, 0, items[j].q_id,
					                          eps_of[j], h->efc,
					                          items[j].w);
			};
			std::vector<std::thread> ts;
			int nt = std::max(1,
			                  std::min<int>(nthreads, (int)items.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(worker);
			worker();
			for (auto &t : ts)
				t.join();
		}
		std::vector<ApplyItem *> all;
		for (auto &it : items)
			all.push_back(&it);
		batched_apply_host(h, 0, all, nthreads);
	}
	hnsw_promote_ep(h);
	h->dirty = true;
	return SDBV_OK;
}

// GPU-accelerated chunked snapshot build, v3 (the
// configs[2] 10M-row build). Bit-identical to the host twin
// sdbv_hnsw_insert_batch_snapshot2 (same batched schedule at EVERY layer,
// same restated distance chains), with all RAM-bound work on the device:
//  - per layer, top-down: one ef=1 multi-query launch carries the greedy
//    descents and one efc launch the insert searches (multi-ep seeding =
//    the layer-above w cascade), against per-layer padded device
//    adjacencies kept in sync by k_adj_scatter deltas;
//  - neighbour selects and prunes: k_pair_mats + k_heur_select (the
//    exact heuristic) at every layer.
// The host keeps the deterministic phase-B edge appends and the queue
// bookkeeping. The round-2 10M trace showed the HOST upper-layer inserts
// of v2 were the remaining wall (~110 s per 1M elements); v3 moves them
// here.
int sdbv_hnsw_insert_batch_snapshot_gpu(sdbv_hnsw *h, const float *pts,
                                        uint64_t n, uint32_t chunk,
                                        int nthreads) {
	using namespace hnsw;
	if (!h || !h->ctx || chunk == 0 || n == 0 || h->efc == 0 ||
	    h->efc > HQ_EF_CAP)
		return SDBV_ERR_BAD_ARG;
	if (h->extend || h->m0 > 64 || h->m > 64 || h->efc + 1 > HSEL_CAP)
		// extend-candidates (or oversized select windows) stay on the
		// host twin — same algorithm, host distances
		return sdbv_hnsw_insert_batch_snapshot2(h, pts, n, chunk, nthreads);
	if (h->finalized) { // writes invalidate the finalized device state
		hnsw_free_device_state(h);
		h->dirty = true;
	}
	if (nthreads <= 0)
		nthreads = (int)std::thread::hardware_concurrency();
	sdbv_ctx *ctx = h->ctx;
	std::lock_guard<std::mutex> ctxlk(ctx->mu);
	uint64_t base = h->next_id;
	std::vector<uint32_t> levels(n);
	for (uint64_t i = 0; i < n; i++)
		levels[i] = next_level(h); // sequential RNG contract, per ordinal
	h->next_id += n;
	h->vecs.reserve(h->vecs.size() + n * h->d);
	for (uint64_t i = 0; i < n; i++)
		hnsw_append_vec(h, pts + i * h->d);
	{
		std::lock_guard<std::mutex> lk(h->global_mu);
		uint32_t max_level = 0;
		for (uint64_t i = 0; i < n; i++)
			max_level = std::max(max_level, levels[i]);
		while (h->layers.size() <= max_level)
			h->layers.push_back(hnsw::Layer{{}, h->m});
		uint64_t ne = h->vecs.size() / h->d;
		for (auto &l : h->layers) {
			if (l.edges.size() < ne)
				l.edges.resize(ne);
			if (l.in_layer.size() < ne)
				l.in_layer.resize(ne, 0);
		}
	}
	const uint64_t nelem = h->vecs.size() / h->d;
	const uint32_t d = h->d;
	const uint32_t efc = h->efc;
	const uint32_t nlayers = (uint32_t)h->layers.size();
	// ---- device state: vectors + per-layer padded adjacencies ----
	for (void **p : {(void **)&h->rm_dev, (void **)&h->norms_dev,
	                 (void **)&h->adj_dev, (void **)&h->deg_dev})
		if (*p) {
			(void)hipFree(*p);
			*p = nullptr;
		}
	HIP_CHECK(ctx, hipMalloc(&h->rm_dev, nelem * d * sizeof(float)));
	HIP_CHECK(ctx, hipMemcpy(h->rm_dev, h->vecs.data(),
	                         nelem * d * sizeof(float),
	                         hipMemcpyHostToDevice));
	if (h->metric == SDBV_METRIC_COSINE) {
		HIP_CHECK(ctx, hipMalloc(&h->norms_dev, nelem * sizeof(double)));
		HIP_CHECK(ctx, hipMemcpy(h->norms_dev, h->norms.data(),
		                         nelem * sizeof(double),
		                         hipMemcpyHostToDevice));
	}
	// layer 0 lives in h->adj_dev/deg_dev; layers >= 1 in build-local
	// arrays (all freed at the end; finalize re-exports the CSR)
	// device adjacency for layers 0 and 1 only: levels >= 2 stay on the
	// classic host path (tiny skeleton layers, progressive for quality)
	const uint32_t ndev_layers = std::min<uint32_t>(nlayers, 2);
	std::vector<uint32_t *> adjL(ndev_layers, nullptr),
	    degL(ndev_layers, nullptr);
	std::vector<uint32_t> strideL(ndev_layers);
	std::vector<uint8_t> has_members(ndev_layers, 0);
	h->dtrack.clear();
	h->dtrack.resize(ndev_layers);
	for (uint32_t l = 0; l < ndev_layers; l++) {
		strideL[l] = (((l == 0 ? h->m0 : h->m) + 8) + 7) & ~7u;
		HIP_CHECK(ctx, hipMalloc(&adjL[l],
		                         nelem * (uint64_t)strideL[l] *
		                             sizeof(uint32_t)));
		HIP_CHECK(ctx, hipMalloc(&degL[l], nelem * sizeof(uint32_t)));
		HIP_CHECK(ctx, hipMemset(degL[l], 0, nelem * sizeof(uint32_t)));
		h->dtrack[l] = std::make_unique<sdbv_hnsw::DirtyTrack>();
		h->dtrack[l]->flag.assign(nelem, 0);
		h->dtrack[l]->list.assign(nelem, 0);
		for (uint64_t i = 0; i < base; i++) { // pre-existing graph
			if (h->layers[l].has((uint32_t)i)) {
				h->mark_dirty(l, (uint32_t)i);
				has_members[l] = 1;
			}
		}
	}
	h->adj_dev = adjL[0];
	h->deg_dev = degL[0];
	h->adj_stride = strideL[0];
	h->adj_nodes = nelem;
	h->dev_rows = nelem;
	const uint64_t vwords = (nelem + 31) / 32;
	{
		uint64_t need = (uint64_t)chunk * vwords * sizeof(uint32_t);
		if (h->vis_cap < need) {
			if (h->vis_dev)
				(void)hipFree(h->vis_dev);
			h->vis_dev = nullptr;
			h->vis_cap = 0;
			HIP_CHECK(ctx, hipMalloc(&h->vis_dev, need));
			h->vis_cap = need;
		}
	}
	// ---- per-launch scratch (capacity = chunk, reused) ----
	float *Qd = nullptr;
	double *qnd = nullptr, *epdd = nullptr, *outd = nullptr;
	uint32_t *epsd = nullptr, *epoffd = nullptr;
	uint32_t *outr = nullptr, *outc = nullptr, *outf = nullptr;
	uint32_t *upd_ids_dev = nullptr, *upd_deg_dev = nullptr,
	         *upd_edges_dev = nullptr;
	uint32_t *listsd = nullptr, *loffd = nullptr, *seld = nullptr,
	         *selcntd = nullptr;
	uint64_t *moffd = nullptr;
	double *matsd = nullptr;
	uint64_t upd_cap = 0, lists_cap = 0, mats_cap = 0, sel_cap = 0,
	         loff_cap = 0;
	auto cleanup = [&] {
		adjL[0] = nullptr; // owned by h->adj_dev (hnsw_free_device_state)
		degL[0] = nullptr;
		for (uint32_t l = 1; l < ndev_layers; l++) {
			if (adjL[l])
				(void)hipFree(adjL[l]);
			if (degL[l])
				(void)hipFree(degL[l]);
		}
		for (void *p : {(void *)Qd, (void *)qnd, (void *)epdd, (void *)epsd,
		                (void *)epoffd, (void *)outr, (void *)outd,
		                (void *)outc, (void *)outf, (void *)upd_ids_dev,
		                (void *)upd_deg_dev, (void *)upd_edges_dev,
		                (void *)listsd, (void *)loffd, (void *)seld,
		                (void *)selcntd, (void *)moffd, (void *)matsd})
			if (p)
				(void)hipFree(p);
		h->dtrack.clear();
	};
#define BGPU_CHECK(call)                                                     \
	do {                                                                     \
		hipError_t err_ = (call);                                            \
		if (err_ != hipSuccess) {                                            \
			ctx->err = std::string("hip: ") + hipGetErrorString(err_);       \
			cleanup();                                                       \
			return SDBV_ERR_HIP;                                             \
		}                                                                    \
	} while (0)
	BGPU_CHECK(hipMalloc(&Qd, (uint64_t)chunk * d * sizeof(float)));
	BGPU_CHECK(hipMalloc(&qnd, chunk * sizeof(double)));
	BGPU_CHECK(hipMalloc(&epdd,
	                     (uint64_t)chunk * (efc + 1) * sizeof(double)));
	BGPU_CHECK(hipMalloc(&epsd,
	                     (uint64_t)chunk * (efc + 1) * sizeof(uint32_t)));
	BGPU_CHECK(hipMalloc(&epoffd, (chunk + 1) * sizeof(uint32_t)));
	BGPU_CHECK(hipMalloc(&outr, (uint64_t)chunk * efc * sizeof(uint32_t)));
	BGPU_CHECK(hipMalloc(&outd, (uint64_t)chunk * efc * sizeof(double)));
	BGPU_CHECK(hipMalloc(&outc, chunk * sizeof(uint32_t)));
	BGPU_CHECK(hipMalloc(&outf, chunk * sizeof(uint32_t)));
	// host staging
	std::vector<float> Qh;
	std::vector<double> qnh, epdh;
	std::vector<uint32_t> epsh, epoffh, outch, outfh, outrh;
	std::vector<double> outdh;
	std::vector<uint32_t> upd_ids, upd_deg, upd_edges;
	std::vector<uint32_t> listsh, loffh, selh, selcnth;
	std::vector<uint64_t> moffh;

	double t_epinit = 0, t_sync = 0, t_kern = 0, t_selA = 0, t_link = 0,
	       t_upperk = 0;
	auto now = [] { return std::chrono::steady_clock::now(); };
	auto secs = [](std::chrono::steady_clock::time_point a,
	               std::chrono::steady_clock::time_point b) {
		return std::chrono::duration<double>(b - a).count();
	};

	auto sync_adj = [&](uint32_t l) -> int {
		auto &D = *h->dtrack[l];
		upd_ids.clear();
		upd_deg.clear();
		uint32_t maxdeg = 0;
		auto &L = h->layers[l];
		uint32_t nd = D.n.load(std::memory_order_relaxed);
		for (uint32_t li = 0; li < nd; li++) {
			uint32_t i = D.list[li];
			uint32_t dg = (uint32_t)L.edges[i].size();
			maxdeg = std::max(maxdeg, dg);
			upd_ids.push_back(i);
			upd_deg.push_back(dg);
		}
		if (maxdeg > strideL[l]) {
			uint32_t ns = (maxdeg + 8 + 7) & ~7u;
			(void)hipFree(adjL[l]);
			adjL[l] = nullptr;
			BGPU_CHECK(hipMalloc(&adjL[l],
			                     nelem * (uint64_t)ns * sizeof(uint32_t)));
			strideL[l] = ns;
			if (l == 0) {
				h->adj_dev = adjL[0];
				h->adj_stride = ns;
			}
			upd_ids.clear();
			upd_deg.clear();
			for (uint64_t i = 0; i < nelem; i++)
				if (!L.edges[i].empty() || D.flag[i]) {
					upd_ids.push_back((uint32_t)i);
					upd_deg.push_back((uint32_t)L.edges[i].size());
				}
		}
		for (uint32_t li = 0; li < nd; li++)
			D.flag[D.list[li]] = 0;
		D.n.store(0, std::memory_order_relaxed);
		uint64_t cnt = upd_ids.size();
		if (cnt == 0)
			return SDBV_OK;
		const uint32_t stride = strideL[l];
		upd_edges.assign(cnt * stride, 0);
		for (uint64_t i = 0; i < cnt; i++) {
			const auto &e = L.edges[upd_ids[i]];
			std::copy(e.begin(), e.end(), upd_edges.begin() + i * stride);
		}
		if (upd_cap < (uint64_t)cnt * stride) {
			for (void **p : {(void **)&upd_ids_dev, (void **)&upd_deg_dev,
			                 (void **)&upd_edges_dev})
				if (*p) {
					(void)hipFree(*p);
					*p = nullptr;
				}
			uint64_t cap = ((uint64_t)cnt * stride * 3) / 2;
			BGPU_CHECK(hipMalloc(&upd_ids_dev, cap * sizeof(uint32_t)));
			BGPU_CHECK(hipMalloc(&upd_deg_dev, cap * sizeof(uint32_t)));
			BGPU_CHECK(hipMalloc(&upd_edges_dev, cap * sizeof(uint32_t)));
			upd_cap = cap;
		}
		BGPU_CHECK(hipMemcpyAsync(upd_ids_dev, upd_ids.data(),
		                          cnt * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(upd_deg_dev, upd_deg.data(),
		                          cnt * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(upd_edges_dev, upd_edges.data(),
		                          cnt * stride * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		uint64_t threads = cnt * stride;
		hipLaunchKernelGGL(k_adj_scatter,
		                   dim3((uint32_t)((threads + 255) / 256)), dim3(256),
		                   0, ctx->stream, upd_ids_dev, upd_deg_dev,
		                   upd_edges_dev, (uint32_t)cnt, stride, adjL[l],
		                   degL[l]);
		return SDBV_OK;
	};

	auto device_select = [&](const std::vector<uint32_t> &lists,
	                         const std::vector<uint32_t> &loff,
	                         uint32_t nlists, uint32_t m_max) -> int {
		moffh.resize(nlists + 1);
		uint64_t mo = 0;
		for (uint32_t i = 0; i < nlists; i++) {
			moffh[i] = mo;
			uint64_t len = loff[i + 1] - loff[i];
			mo += len * len;
		}
		moffh[nlists] = mo;
		if (lists_cap < lists.size()) {
			if (listsd)
				(void)hipFree(listsd);
			listsd = nullptr;
			BGPU_CHECK(hipMalloc(&listsd,
			                     lists.size() * 3 / 2 * sizeof(uint32_t)));
			lists_cap = lists.size() * 3 / 2;
		}
		if (loff_cap < nlists + 1) {
			for (void **p : {(void **)&loffd, (void **)&moffd,
			                 (void **)&selcntd})
				if (*p) {
					(void)hipFree(*p);
					*p = nullptr;
				}
			uint64_t cap = (nlists + 1) * 3 / 2;
			BGPU_CHECK(hipMalloc(&loffd, cap * sizeof(uint32_t)));
			BGPU_CHECK(hipMalloc(&moffd, cap * sizeof(uint64_t)));
			BGPU_CHECK(hipMalloc(&selcntd, cap * sizeof(uint32_t)));
			loff_cap = cap;
		}
		if (mats_cap < mo) {
			if (matsd)
				(void)hipFree(matsd);
			matsd = nullptr;
			BGPU_CHECK(hipMalloc(&matsd, mo * 5 / 4 * sizeof(double)));
			mats_cap = mo * 5 / 4;
		}
		if (sel_cap < (uint64_t)nlists * m_max) {
			if (seld)
				(void)hipFree(seld);
			seld = nullptr;
			BGPU_CHECK(hipMalloc(&seld, (uint64_t)nlists * m_max * 3 / 2 *
			                                sizeof(uint32_t)));
			sel_cap = (uint64_t)nlists * m_max * 3 / 2;
		}
		BGPU_CHECK(hipMemcpyAsync(listsd, lists.data(),
		                          lists.size() * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(loffd, loff.data(),
		                          (nlists + 1) * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(moffd, moffh.data(),
		                          (nlists + 1) * sizeof(uint64_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		hipLaunchKernelGGL(k_pair_mats, dim3(nlists), dim3(256), 0,
		                   ctx->stream, h->rm_dev, h->norms_dev, d,
		                   (int)h->metric, listsd, loffd, moffd, matsd);
		hipLaunchKernelGGL(k_heur_select, dim3(nlists), dim3(64), 0,
		                   ctx->stream, listsd, loffd, moffd, matsd, m_max,
		                   h->keep ? 1 : 0, seld, selcntd);
		selh.resize((uint64_t)nlists * m_max);
		selcnth.resize(nlists);
		BGPU_CHECK(hipMemcpyAsync(selh.data(), seld,
		                          (uint64_t)nlists * m_max *
		                              sizeof(uint32_t),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(selcnth.data(), selcntd,
		                          nlists * sizeof(uint32_t),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipStreamSynchronize(ctx->stream));
		BGPU_CHECK(hipGetLastError());
		return SDBV_OK;
	};

	// launch the persistent-kernel search for a subset of chunk items at
	// layer l: queries/norms/eps packed from item indices; results land in
	// outr/outd/outc/outf at the SUBSET ordinal positions.
	std::vector<ApplyItem> items;
	std::vector<PQ> eps_of;
	std::vector<uint32_t> lvl_of;
	auto launch_search = [&](uint32_t l, const std::vector<uint32_t> &sub,
	                         uint32_t k, uint32_t ef) -> int {
		uint32_t b = (uint32_t)sub.size();
		Qh.resize((uint64_t)b * d);
		qnh.resize(b);
		epoffh.resize(b + 1);
		epsh.clear();
		epdh.clear();
		for (uint32_t j = 0; j < b; j++) {
			uint32_t q_id = items[sub[j]].q_id;
			std::memcpy(Qh.data() + (uint64_t)j * d, vec(h, q_id),
			            d * sizeof(float));
			qnh[j] = h->metric == SDBV_METRIC_COSINE ? h->norms[q_id] : 0;
			epoffh[j] = (uint32_t)epsh.size();
			for (auto &e : eps_of[sub[j]].to_vec()) {
				epsh.push_back(e.second);
				epdh.push_back(e.first);
			}
		}
		epoffh[b] = (uint32_t)epsh.size();
		BGPU_CHECK(hipMemcpyAsync(Qd, Qh.data(),
		                          (uint64_t)b * d * sizeof(float),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(qnd, qnh.data(), b * sizeof(double),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(epsd, epsh.data(),
		                          epsh.size() * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(epdd, epdh.data(),
		                          epdh.size() * sizeof(double),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(epoffd, epoffh.data(),
		                          (b + 1) * sizeof(uint32_t),
		                          hipMemcpyHostToDevice, ctx->stream));
		BGPU_CHECK(hipMemsetAsync(h->vis_dev, 0,
		                          (uint64_t)b * vwords * sizeof(uint32_t),
		                          ctx->stream));
		hipLaunchKernelGGL(k_hnsw_search<1>, dim3(b), dim3(64), 0,
		                   ctx->stream, h->rm_dev, h->norms_dev, d,
		                   (int)h->metric, degL[l], adjL[l], strideL[l], Qd,
		                   qnd, epsd, epdd, epoffd, h->vis_dev, vwords, k,
		                   ef, outr, outd, outc, outf);
		outch.resize(b);
		outfh.resize(b);
		outrh.resize((uint64_t)b * k);
		outdh.resize((uint64_t)b * k);
		BGPU_CHECK(hipMemcpyAsync(outch.data(), outc, b * sizeof(uint32_t),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(outfh.data(), outf, b * sizeof(uint32_t),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(outrh.data(), outr,
		                          (uint64_t)b * k * sizeof(uint32_t),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipMemcpyAsync(outdh.data(), outd,
		                          (uint64_t)b * k * sizeof(double),
		                          hipMemcpyDeviceToHost, ctx->stream));
		BGPU_CHECK(hipStreamSynchronize(ctx->stream));
		BGPU_CHECK(hipGetLastError());
		return SDBV_OK;
	};

	// device select + phase B/C for the insert set at layer l. The w
	// windows were just searched into outrh/outdh (subset order).
	auto apply_layer = [&](uint32_t l, const std::vector<uint32_t> &ins)
	    -> int {
		uint32_t b = (uint32_t)ins.size();
		uint32_t m_max = h->layers[l].m_max;
		listsh.clear();
		loffh.assign(b + 1, 0);
		for (uint32_t j = 0; j < b; j++) {
			loffh[j] = (uint32_t)listsh.size();
			listsh.push_back(items[ins[j]].q_id);
			if (!(outfh[j] & HQ_FLAG_OVERFLOW))
				for (uint32_t i = 0; i < outch[j]; i++)
					listsh.push_back(outrh[(uint64_t)j * efc + i]);
		}
		loffh[b] = (uint32_t)listsh.size();
		int rc = device_select(listsh, loffh, b, m_max);
		if (rc)
			return rc;
		for (uint32_t j = 0; j < b; j++) {
			ApplyItem &it = items[ins[j]];
			if (outfh[j] & HQ_FLAG_OVERFLOW) {
				// exact host fallback (rare)
				PQ w;
				snapshot_search_layer_eps(h, l, it.q_id, eps_of[ins[j]],
				                          efc, w);
				eps_of[ins[j]] = w;
				const float *q_pt = vec(h, it.q_id);
				double qn = h->metric == SDBV_METRIC_COSINE
				                ? h->norms[it.q_id]
				                : 0;
				it.neighbors.clear();
				select_neighbors(h, h->layers[l], it.q_id, q_pt, qn,
				                 std::move(w), it.neighbors, false);
				continue;
			}
			it.neighbors.assign(
			    selh.begin() + (uint64_t)j * m_max,
			    selh.begin() + (uint64_t)j * m_max + selcnth[j]);
		}
		std::vector<ApplyItem *> ptrs;
		ptrs.reserve(b);
		for (uint32_t j = 0; j < b; j++)
			ptrs.push_back(&items[ins[j]]);
		auto tb0 = now();
		auto overfull = batched_apply_phaseB(h, l, ptrs);
		t_link += secs(tb0, now());
		if (!overfull.empty()) {
			listsh.clear();
			loffh.clear();
			std::vector<uint32_t> host_prunes, dev_nodes;
			for (uint32_t e : overfull) {
				const auto &conn = h->layers[l].edges[e];
				if (1 + conn.size() > HSEL_CAP) {
					host_prunes.push_back(e);
					continue;
				}
				dev_nodes.push_back(e);
				loffh.push_back((uint32_t)listsh.size());
				listsh.push_back(e);
				for (uint32_t nid : conn) {
					if (nid < h->elem_present.size() &&
					    !h->elem_present[nid])
						continue;
					listsh.push_back(nid);
				}
			}
			loffh.push_back((uint32_t)listsh.size());
			if (!dev_nodes.empty()) {
				rc = device_select(listsh, loffh,
				                   (uint32_t)dev_nodes.size(), m_max);
				if (rc)
					return rc;
				for (uint32_t li = 0; li < dev_nodes.size(); li++) {
					uint32_t e = dev_nodes[li];
					auto &ee = h->layers[l].edges[e];
					ee.assign(selh.begin() + (uint64_t)li * m_max,
					          selh.begin() + (uint64_t)li * m_max +
					              selcnth[li]);
					h->mark_dirty(l, e);
				}
			}
			if (!host_prunes.empty())
				batched_apply_phaseC_host(h, l, host_prunes, nthreads);
		}
		return SDBV_OK;
	};

	std::vector<std::pair<uint32_t, uint32_t>> upper2; // (q_id, level)
	// warm-up: see the host twin — the first elements of an empty graph
	// insert classically so batching starts on a connected graph
	const uint64_t warm_until = h->enter_point < 0 ? base + 64 : 0;
	for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
		uint64_t c1 = std::min(n, c0 + chunk);
		auto tp0 = now();
		items.clear();
		eps_of.clear();
		lvl_of.clear();
		upper2.clear();
		for (uint64_t i = c0; i < c1; i++) {
			if (h->enter_point < 0 || base + i < warm_until) {
				insert_at(h, (uint32_t)(base + i), levels[i], false);
				for (uint32_t l = 0;
				     l < ndev_layers && l <= levels[i]; l++) {
					h->mark_dirty(l, (uint32_t)(base + i));
					has_members[l] = 1;
				}
				continue;
			}
			if (levels[i] >= 2) {
				// levels >= 2 (0.4% of elements): FULL classic host
				// inserts — progressive at every layer (half-inserted
				// elements must never be search-visible; their classic
				// applies mark the device adjacency via
				// layer_insert_apply's dirty hooks)
				upper2.push_back({(uint32_t)(base + i), levels[i]});
				continue;
			}
			items.push_back(ApplyItem{(uint32_t)(base + i), PQ{}, {}});
			eps_of.emplace_back();
			lvl_of.push_back(levels[i]);
		}
		if (!upper2.empty()) {
			std::atomic<uint64_t> cursor{0};
			auto worker = [&]() {
				uint64_t j;
				while ((j = cursor.fetch_add(1)) < upper2.size())
					insert_at(h, upper2[j].first, upper2[j].second, true);
			};
			std::vector<std::thread> ts;
			int nt = std::max(1,
			                  std::min<int>(nthreads, (int)upper2.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(worker);
			worker();
			for (auto &t : ts)
				t.join();
			for (uint32_t l = 0; l < ndev_layers; l++)
				has_members[l] = 1; // classic inserts joined every layer
		}
		if (items.empty())
			continue;
		// levels <= 1: host greedy descents through layers top..2
		{
			std::atomic<uint64_t> cursor{0};
			auto worker = [&]() {
				uint64_t j;
				while ((j = cursor.fetch_add(1)) < items.size()) {
					uint32_t q_id = items[j].q_id;
					double qn = h->metric == SDBV_METRIC_COSINE
					                ? h->norms[q_id]
					                : 0;
					uint32_t ep;
					double epd;
					descend_to_layer2(h, q_id, qn, &ep, &epd);
					eps_of[j].push(epd, ep);
				}
			};
			std::vector<std::thread> ts;
			int nt = std::max(1,
			                  std::min<int>(nthreads, (int)items.size()));
			for (int t = 1; t < nt; t++)
				ts.emplace_back(worker);
			worker();
			for (auto &t : ts)
				t.join();
		}
		auto tp1 = now();
		t_epinit += secs(tp0, tp1);
		// layer 1 (device): ef=1 descents for level-0 elements, efc
		// searches + batched apply for level >= 1
		if (nlayers >= 2) {
			const uint32_t l = 1;
			std::vector<uint32_t> desc, ins;
			for (uint32_t j = 0; j < (uint32_t)items.size(); j++)
				(lvl_of[j] >= l ? ins : desc).push_back(j);
			auto tu0 = now();
			int rc = sync_adj(l);
			if (rc)
				return rc;
			t_sync += secs(tu0, now());
			if (has_members[l] && !desc.empty()) {
				auto tk = now();
				rc = launch_search(l, desc, 1, 1);
				if (rc)
					return rc;
				t_upperk += secs(tk, now());
				for (uint32_t j = 0; j < desc.size(); j++) {
					if (outch[j] == 0)
						continue; // keep previous eps
					PQ ne2;
					ne2.push(outdh[(uint64_t)j * 1], outrh[j]);
					eps_of[desc[j]] = std::move(ne2);
				}
			}
			if (!ins.empty()) {
				if (has_members[l]) {
					auto tk = now();
					rc = launch_search(l, ins, efc, efc);
					if (rc)
						return rc;
					t_upperk += secs(tk, now());
					// cascade eps = w
					for (uint32_t j = 0; j < ins.size(); j++) {
						if (outfh[j] & HQ_FLAG_OVERFLOW)
							continue; // handled in apply_layer
						PQ ne2;
						for (uint32_t i = 0; i < outch[j]; i++)
							ne2.push(outdh[(uint64_t)j * efc + i],
							         outrh[(uint64_t)j * efc + i]);
						eps_of[ins[j]] = std::move(ne2);
					}
				} else {
					// empty layer: search degenerates to w = eps
					outch.assign(ins.size(), 0);
					outfh.assign(ins.size(), 0);
					outrh.resize(ins.size() * (uint64_t)efc);
					outdh.resize(ins.size() * (uint64_t)efc);
					for (uint32_t j = 0; j < ins.size(); j++) {
						auto v = eps_of[ins[j]].to_vec();
						outch[j] = (uint32_t)std::min<size_t>(v.size(),
						                                      efc);
						for (uint32_t i = 0; i < outch[j]; i++) {
							outrh[(uint64_t)j * efc + i] = v[i].second;
							outdh[(uint64_t)j * efc + i] = v[i].first;
						}
					}
				}
				auto ta = now();
				rc = apply_layer(l, ins);
				if (rc)
					return rc;
				t_selA += secs(ta, now());
				has_members[l] = 1;
			}
		}
		// layer 0: every item
		{
			std::vector<uint32_t> all(items.size());
			for (uint32_t j = 0; j < (uint32_t)items.size(); j++)
				all[j] = j;
			auto tu0 = now();
			int rc = sync_adj(0);
			if (rc)
				return rc;
			t_sync += secs(tu0, now());
			auto tk = now();
			if (has_members[0]) {
				rc = launch_search(0, all, efc, efc);
				if (rc)
					return rc;
			} else {
				outch.assign(all.size(), 0);
				outfh.assign(all.size(), 0);
				outrh.resize(all.size() * (uint64_t)efc);
				outdh.resize(all.size() * (uint64_t)efc);
				for (uint32_t j = 0; j < all.size(); j++) {
					auto v = eps_of[j].to_vec();
					outch[j] = (uint32_t)std::min<size_t>(v.size(), efc);
					for (uint32_t i = 0; i < outch[j]; i++) {
						outrh[(uint64_t)j * efc + i] = v[i].second;
						outdh[(uint64_t)j * efc + i] = v[i].first;
					}
				}
			}
			t_kern += secs(tk, now());
			auto ta = now();
			rc = apply_layer(0, all);
			if (rc)
				return rc;
			t_selA += secs(ta, now());
			has_members[0] = 1;
		}
		if (((c0 / chunk) & 63) == 63)
			fprintf(stderr,
			        "[sdbv build_gpu3] %llu/%llu epinit=%.1f sync=%.1f "
			        "upperk=%.1f kern0=%.1f apply=%.1f link=%.1f\n",
			        (unsigned long long)c1, (unsigned long long)n,
			        t_epinit, t_sync, t_upperk, t_kern, t_selA, t_link);
	}
#undef BGPU_CHECK
	hnsw_promote_ep(h);
	fprintf(stderr,
	        "[sdbv build_gpu3] n=%llu chunk=%u phases: epinit=%.1fs "
	        "sync=%.1fs upper-kernels=%.1fs kernel0=%.1fs "
	        "apply(selA+selC)=%.1fs link=%.1fs\n",
	        (unsigned long long)n, chunk, t_epinit, t_sync, t_upperk,
	        t_kern, t_selA, t_link);
	cleanup();
	h->dirty = true;
	return SDBV_OK;
}


uint64_t sdbv_hnsw_n(sdbv_hnsw *h) { return h ? h->next_id : 0; }
uint32_t sdbv_hnsw_layers(sdbv_hnsw *h) {
	return h ? (uint32_t)h->layers.size() : 0;
}
uint64_t sdbv_hnsw_l0_edge_count(sdbv_hnsw *h) {
	uint64_t c = 0;
	for (auto &e : h->layers[0].edges)
		c += e.size();
	return c;
}
void sdbv_hnsw_l0_export(sdbv_hnsw *h, uint32_t *offsets, uint32_t *edges) {
	uint32_t off = 0;
	for (uint64_t i = 0; i < h->next_id; i++) {
		offsets[i] = off;
		if (i < h->layers[0].edges.size())
			for (uint32_t e : h->layers[0].edges[i])
				edges[off++] = e;
	}
	offsets[h->next_id] = off;
}
/* Full per-layer export (CSR + membership) — lets the bench's cpu_baseline
 * leg import the exact product graph into the oracle searcher. */
uint64_t sdbv_hnsw_layer_edge_count(sdbv_hnsw *h, uint32_t l) {
	if (!h || l >= h->layers.size())
		return 0;
	uint64_t c = 0;
	for (auto &e : h->layers[l].edges)
		c += e.size();
	return c;
}
void sdbv_hnsw_layer_export(sdbv_hnsw *h, uint32_t l, uint32_t *offsets,
                            uint32_t *edges, uint8_t *in_layer) {
	uint32_t off = 0;
	const auto &L = h->layers[l];
	for (uint64_t i = 0; i < h->next_id; i++) {
		offsets[i] = off;
		in_layer[i] = L.has((uint32_t)i) ? 1 : 0;
		if (i < L.edges.size())
			for (uint32_t e : L.edges[i])
				edges[off++] = e;
	}
	offsets[h->next_id] = off;
}
int64_t sdbv_hnsw_enter_point(sdbv_hnsw *h) {
	return h ? h->enter_point : -1;
}
/* Zero-copy view of the host row-major vector store (n x d f32, element id
 * = row): the oracle import reads rows from here instead of a second copy. */
const float *sdbv_hnsw_vecs_ptr(sdbv_hnsw *h) {
	return h ? h->vecs.data() : nullptr;
}

// Frees the per-index device state so finalize can be called again after
// host-graph mutations (apply_pendings re-finalizes a dirty index).
static void hnsw_free_device_state(sdbv_hnsw *h) {
	for (void **p : {(void **)&h->rows_dev, (void **)&h->dout_dev,
	                 (void **)&h->q_dev, (void **)&h->rm_dev,
	                 (void **)&h->offsets_dev, (void **)&h->edges_dev,
	                 (void **)&h->norms_dev, (void **)&h->vis_dev,
	                 (void **)&h->adj_dev, (void **)&h->deg_dev}) {
		if (*p)
			(void)hipFree(*p);
		*p = nullptr;
	}
	if (h->rows_pinned) {
		(void)hipHostFree(h->rows_pinned);
		h->rows_pinned = nullptr;
	}
	if (h->dists_pinned) {
		(void)hipHostFree(h->dists_pinned);
		h->dists_pinned = nullptr;
	}
	h->vis_cap = 0;
	h->adj_stride = 0;
	h->adj_nodes = 0;
	h->dev_rows = 0;
	h->finalized = false;
}

int sdbv_hnsw_finalize(sdbv_hnsw *h, uint64_t table) {
	if (!h || !h->ctx || h->next_id == 0)
		return SDBV_ERR_BAD_ARG;
	hnsw_free_device_state(h);
	int rc = stage_corpus_impl(h->ctx, table, h->vecs.data(), nullptr,
	                           h->next_id, h->d, h->metric, false);
	if (rc)
		return rc;
	sdbv_ctx *ctx = h->ctx;
	// per-hop scratch sized from the ACTUAL max layer-0 degree: a
	// parallel/batched build can leave a node transiently above m0 (the
	// keep-back fold in layer_insert_apply), and a frontier copy larger
	// than the scratch would overflow it (round-1 advisor class of bug)
	h->max_deg = h->m0 + 1;
	for (uint64_t i = 0; i < h->next_id; i++)
		h->max_deg = std::max<uint32_t>(
		    h->max_deg, (uint32_t)h->layers[0].edges[i].size() + 1);
	HIP_CHECK(ctx, hipMalloc(&h->rows_dev, h->max_deg * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipMalloc(&h->dout_dev, h->max_deg * sizeof(double)));
	HIP_CHECK(ctx, hipMalloc(&h->q_dev, h->d * sizeof(float)));
	HIP_CHECK(ctx, hipHostMalloc(&h->rows_pinned,
	                             h->max_deg * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipHostMalloc(&h->dists_pinned,
	                             h->max_deg * sizeof(double)));
	// persistent-kernel graph state: row-major vectors + layer-0 CSR
	uint64_t n = h->next_id;
	HIP_CHECK(ctx, hipMalloc(&h->rm_dev, n * h->d * sizeof(float)));
	HIP_CHECK(ctx, hipMemcpy(h->rm_dev, h->vecs.data(),
	                         n * h->d * sizeof(float),
	                         hipMemcpyHostToDevice));
	{
		// Scrubbed CSR: dangling edges to removed elements are dropped at
		// export, so the device kernels (which have no elements map) see
		// exactly the live graph — equivalent to the reference's
		// get_vector None gate (layer.rs:206).
		std::vector<uint32_t> offsets(n + 1);
		std::vector<uint32_t> edges;
		uint64_t ec = 0;
		for (uint64_t i = 0; i < n; i++) {
			offsets[i] = (uint32_t)ec;
			for (uint32_t e : h->layers[0].edges[i])
				if (h->elem_present[e]) {
					edges.push_back(e);
					ec++;
				}
		}
		offsets[n] = (uint32_t)ec;
		HIP_CHECK(ctx, hipMalloc(&h->offsets_dev, (n + 1) * sizeof(uint32_t)));
		HIP_CHECK(ctx, hipMalloc(&h->edges_dev,
		                         std::max<uint64_t>(ec, 1) * sizeof(uint32_t)));
		HIP_CHECK(ctx, hipMemcpy(h->offsets_dev, offsets.data(),
		                         (n + 1) * sizeof(uint32_t),
		                         hipMemcpyHostToDevice));
		if (ec)
			HIP_CHECK(ctx, hipMemcpy(h->edges_dev, edges.data(),
			                         ec * sizeof(uint32_t),
			                         hipMemcpyHostToDevice));
	}
	if (h->metric == SDBV_METRIC_COSINE) {
		HIP_CHECK(ctx, hipMalloc(&h->norms_dev, n * sizeof(double)));
		HIP_CHECK(ctx, hipMemcpy(h->norms_dev, h->norms.data(),
		                         n * sizeof(double), hipMemcpyHostToDevice));
	}
	h->table = table;
	h->finalized = true;
	h->dirty = false;
	return SDBV_OK;
}

// Batched ef-search on the persistent kernel: one query per workgroup; host
// does the upper-layer descent (search_ep) per query, the kernel runs the
// full layer-0 best-first loop. Results are EXACTLY the reference's
// (to_vec_limit(k) then the builder's (dist total_cmp, id) order). Any query
// whose in-kernel candidate queue overflowed (HQ_FLAG_OVERFLOW, not observed
// on real workloads) is re-run on the exact per-hop path.
int sdbv_hnsw_knn_batch(sdbv_hnsw *h, const float *Q, uint32_t b, uint32_t k,
                        uint32_t ef, uint64_t *out_ids, double *out_dists,
                        uint32_t *out_ns) {
	using namespace hnsw;
	// k is bounded by the in-kernel w window (HQ_EF_CAP), not the scan's
	// MAX_K: the output extraction loops generically over k slots. k <= 64
	// is the GPU-validated regime; larger k (the snapshot build's efc
	// window, round 2) shares the same code path.
	if (!h || !h->finalized || b == 0 || k == 0 || k > HQ_EF_CAP ||
	    ef > HQ_EF_CAP)
		return SDBV_ERR_BAD_ARG;
	if (h->enter_point < 0) {
		for (uint32_t j = 0; j < b; j++)
			out_ns[j] = 0;
		return SDBV_OK;
	}
	sdbv_ctx *ctx = h->ctx;
	std::unique_lock<std::mutex> lk(ctx->mu);
	uint64_t n = h->next_id;

	// host: per-query norms (restated chain) + upper-layer descent
	std::vector<double> qnorms(b);
	std::vector<uint32_t> eps(b);
	std::vector<double> epd(b);
	for (uint32_t j = 0; j < b; j++) {
		const float *q = Q + (uint64_t)j * h->d;
		qnorms[j] = sqrt(host_sumsq_f32(q, h->d));
		uint32_t ep_id = (uint32_t)h->enter_point;
		double ep_dist = dist(h, q, qnorms[j], ep_id);
		for (size_t l = h->layers.size() - 1; l >= 1; l--) {
			PQ cand;
			cand.push(ep_dist, ep_id);
			std::unordered_set<uint32_t> visited{ep_id};
			PQ w = cand;
			search_layer_host(h, h->layers[l], q, qnorms[j], cand, visited, w,
			                  1, false);
			double dd;
			uint32_t ii;
			if (w.peek_first(&dd, &ii)) {
				ep_dist = dd;
				ep_id = ii;
			}
		}
		eps[j] = ep_id;
		epd[j] = ep_dist;
	}

	// device buffers
	uint64_t vwords = (n + 31) / 32;
	uint64_t vis_need = (uint64_t)b * vwords * sizeof(uint32_t);
	if (h->vis_cap < vis_need) {
		if (h->vis_dev)
			(void)hipFree(h->vis_dev);
		h->vis_dev = nullptr;
		h->vis_cap = 0;
		HIP_CHECK(ctx, hipMalloc(&h->vis_dev, vis_need));
		h->vis_cap = vis_need;
	}
	HIP_CHECK(ctx, hipMemsetAsync(h->vis_dev, 0, vis_need, ctx->stream));
	float *Qd = nullptr;
	double *qnd = nullptr, *epdd = nullptr, *outd = nullptr;
	uint32_t *epsd = nullptr, *outr = nullptr, *outc = nullptr, *outf = nullptr;
	HIP_CHECK(ctx, hipMalloc(&Qd, (uint64_t)b * h->d * sizeof(float)));
	HIP_CHECK(ctx, hipMalloc(&qnd, b * sizeof(double)));
	HIP_CHECK(ctx, hipMalloc(&epdd, b * sizeof(double)));
	HIP_CHECK(ctx, hipMalloc(&epsd, b * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipMalloc(&outr, (uint64_t)b * k * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipMalloc(&outd, (uint64_t)b * k * sizeof(double)));
	HIP_CHECK(ctx, hipMalloc(&outc, b * sizeof(uint32_t)));
	HIP_CHECK(ctx, hipMalloc(&outf, b * sizeof(uint32_t)));
	auto cleanup = [&] {
		for (void *p : {(void *)Qd, (void *)qnd, (void *)epdd, (void *)epsd,
		                (void *)outr, (void *)outd, (void *)outc,
		                (void *)outf})
			if (p)
				(void)hipFree(p);
	};
	(void)hipMemcpyAsync(Qd, Q, (uint64_t)b * h->d * sizeof(float),
	               hipMemcpyHostToDevice, ctx->stream);
	(void)hipMemcpyAsync(qnd, qnorms.data(), b * sizeof(double),
	               hipMemcpyHostToDevice, ctx->stream);
	(void)hipMemcpyAsync(epdd, epd.data(), b * sizeof(double),
	               hipMemcpyHostToDevice, ctx->stream);
	(void)hipMemcpyAsync(epsd, eps.data(), b * sizeof(uint32_t),
	               hipMemcpyHostToDevice, ctx->stream);

	auto t0 = std::chrono::steady_clock::now();
	hipLaunchKernelGGL(k_hnsw_search<0>, dim3(b), dim3(64), 0, ctx->stream,
	                   h->rm_dev, h->norms_dev, h->d, (int)h->metric,
	                   h->offsets_dev, h->edges_dev, 0u, Qd, qnd, epsd, epdd,
	                   (const uint32_t *)nullptr,
	                   h->vis_dev, vwords, k, ef, outr, outd, outc, outf);
	std::vector<uint32_t> h_rows((uint64_t)b * k), h_cnt(b), h_flags(b);
	std::vector<double> h_d((uint64_t)b * k);
	(void)hipMemcpyAsync(h_rows.data(), outr, h_rows.size() * sizeof(uint32_t),
	               hipMemcpyDeviceToHost, ctx->stream);
	(void)hipMemcpyAsync(h_d.data(), outd, h_d.size() * sizeof(double),
	               hipMemcpyDeviceToHost, ctx->stream);
	(void)hipMemcpyAsync(h_cnt.data(), outc, b * sizeof(uint32_t),
	               hipMemcpyDeviceToHost, ctx->stream);
	(void)hipMemcpyAsync(h_flags.data(), outf, b * sizeof(uint32_t),
	               hipMemcpyDeviceToHost, ctx->stream);
	if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
	    hipGetLastError() != hipSuccess) {
		ctx->err = "k_hnsw_search failed";
		cleanup();
		return SDBV_ERR_HIP;
	}
	ctx->stats.last_scan_kernel_ms =
	    std::chrono::duration<double, std::milli>(
	        std::chrono::steady_clock::now() - t0)
	        .count();
	ctx->stats.last_rows_scanned = n;
	cleanup();

	uint32_t overflowed = 0;
	for (uint32_t j = 0; j < b; j++)
		if (h_flags[j] & 1u)
			overflowed++;

	// final (dist total_cmp, id) order per query (knn.rs:363)
	for (uint32_t j = 0; j < b; j++) {
		if (h_flags[j] & 1u)
			continue; // re-run below on the exact per-hop path
		uint32_t m = h_cnt[j];
		std::vector<std::pair<std::pair<uint64_t, uint32_t>, double>> fin(m);
		for (uint32_t i = 0; i < m; i++) {
			double dd = h_d[(uint64_t)j * k + i];
			fin[i] = {{total_key(dd), h_rows[(uint64_t)j * k + i]}, dd};
		}
		std::sort(fin.begin(), fin.end());
		out_ns[j] = m;
		for (uint32_t i = 0; i < m; i++) {
			out_ids[(uint64_t)j * k + i] = fin[i].first.second;
			out_dists[(uint64_t)j * k + i] = fin[i].second;
		}
	}
	if (overflowed) {
		// exact fallback for overflowed queries (still the GPU gather path;
		// sdbv_hnsw_knn takes the ctx mutex itself)
		lk.unlock();
		for (uint32_t j = 0; j < b; j++)
			if (h_flags[j] & 1u) {
				int rc = sdbv_hnsw_knn(h, Q + (uint64_t)j * h->d, k, ef,
				                       out_ids + (uint64_t)j * k,
				                       out_dists + (uint64_t)j * k,
				                       &out_ns[j]);
				if (rc)
					return rc;
			}
	}
	return SDBV_OK;
}

// knn_search (hnsw/index.rs:270-335 without the host-kept parts): host
// upper-layer descent, then the layer-0 ef-search where each hop's
// neighbour distances come from the GPU gather kernel (the north_star's
// "batched gather + distance" design). Exact queue semantics preserved:
// distances are queue-independent, so batching them per hop does not change
// the reference's accept/update order.
int sdbv_hnsw_knn(sdbv_hnsw *h, const float *q, uint32_t k, uint32_t ef,
                  uint64_t *out_ids, double *out_dists, uint32_t *out_n) {
	using namespace hnsw;
	if (!h || !h->finalized)
		return SDBV_ERR_BAD_ARG;
	if (h->enter_point < 0) {
		*out_n = 0;
		return SDBV_OK;
	}
	sdbv_ctx *ctx = h->ctx;
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(h->table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;

	double q_norm_d = 0;
	float q_sumsq = 0;
	{
		float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		uint32_t i = 0;
		for (; i + 8 <= h->d; i += 8)
			for (uint32_t tt = 0; tt < 8; tt++)
				p[tt] += q[i + tt] * q[i + tt];
		q_sumsq = 0;
		q_sumsq += ((p[0] + p[4]) + (p[1] + p[5]));
		q_sumsq += ((p[2] + p[6]) + (p[3] + p[7]));
		for (; i < h->d; i++)
			q_sumsq += q[i] * q[i];
		q_norm_d = sqrt((double)q_sumsq);
	}

	// upper layers: greedy descent, host distances (tiny)
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q, q_norm_d, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q, q_norm_d, cand, visited, w, 1,
		                  false);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}

	// layer 0: ef-search with GPU batched neighbour expansion
	HIP_CHECK(ctx, hipMemcpyAsync(h->q_dev, q, h->d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	const Layer &l0 = h->layers[0];
	PQ candidates, w;
	candidates.push(ep_dist, ep_id);
	w.push(ep_dist, ep_id);
	std::vector<bool> visited(h->next_id, false);
	visited[ep_id] = true;
	double fq = w.peek_last_dist(DBL_MAX);
	std::vector<uint32_t> frontier;
	std::vector<double> fdists(h->max_deg); // actual max degree
	double cd;
	uint32_t doc;
	double gpu_ms = 0;
	uint64_t gathered = 0;
	while (candidates.pop_first(&cd, &doc)) {
		if (cd > fq)
			break;
		frontier.clear();
		for (uint32_t e : l0.edges[doc])
			if (!visited[e]) {
				visited[e] = true;
				// elements.get_vector -> None (dangling edge to a
				// removed element): visited-marked then skipped
				if (!h->elem_present[e])
					continue;
				frontier.push_back(e);
			}
		if (frontier.empty())
			continue;
		auto hop_t0 = std::chrono::steady_clock::now();
		// ONE gather+distance launch for this hop's neighbours
		std::memcpy(h->rows_pinned, frontier.data(),
		            frontier.size() * sizeof(uint32_t));
		HIP_CHECK(ctx, hipMemcpyAsync(h->rows_dev, h->rows_pinned,
		                              frontier.size() * sizeof(uint32_t),
		                              hipMemcpyHostToDevice, ctx->stream));
		if (t.metric == SDBV_METRIC_COSINE)
			hipLaunchKernelGGL(k_gather_dist<0>, dim3((uint32_t)frontier.size()),
			                   dim3(64), 0, ctx->stream, t.cm, t.norms,
			                   t.n_pad, t.d, h->rows_dev,
			                   (uint32_t)frontier.size(), h->q_dev, q_norm_d,
			                   h->dout_dev);
		else
			hipLaunchKernelGGL(k_gather_dist<1>, dim3((uint32_t)frontier.size()),
			                   dim3(64), 0, ctx->stream, t.cm, t.norms,
			                   t.n_pad, t.d, h->rows_dev,
			                   (uint32_t)frontier.size(), h->q_dev, q_norm_d,
			                   h->dout_dev);
		HIP_CHECK(ctx, hipMemcpyAsync(h->dists_pinned, h->dout_dev,
		                              frontier.size() * sizeof(double),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		std::memcpy(fdists.data(), h->dists_pinned,
		            frontier.size() * sizeof(double));
		gpu_ms += std::chrono::duration<double, std::milli>(
		              std::chrono::steady_clock::now() - hop_t0)
		              .count();
		gathered += frontier.size();
		// sequential accept/update in edge order (layer.rs:195-218)
		for (size_t i = 0; i < frontier.size(); i++) {
			double ed = fdists[i];
			uint32_t e = frontier[i];
			if (ed < fq || w.n < ef) {
				candidates.push(ed, e);
				w.push(ed, e);
				if (w.n > ef)
					w.pop_last();
				fq = w.peek_last_dist(DBL_MAX);
			}
		}
	}

	ctx->stats.last_scan_kernel_ms = gpu_ms; // gather sections (incl. copies)
	ctx->stats.last_merge_kernel_ms = 0;
	ctx->stats.last_rows_scanned = gathered;

	// to_vec_limit(k) in (dist, FIFO) order (knn.rs:92-104), then the
	// KnnResultBuilder (dist, id) final ordering (knn.rs:363)
	auto v = w.to_vec();
	size_t m = std::min<size_t>(k, v.size());
	std::vector<std::pair<std::pair<uint64_t, uint32_t>, double>> fin(m);
	for (size_t i = 0; i < m; i++)
		fin[i] = {{total_key(v[i].first), v[i].second}, v[i].first};
	std::sort(fin.begin(), fin.end());
	*out_n = (uint32_t)m;
	for (size_t i = 0; i < m; i++) {
		out_ids[i] = fin[i].first.second;
		out_dists[i] = fin[i].second;
	}
	return SDBV_OK;
}

int sdbv_hnsw_remove(sdbv_hnsw *h, uint64_t e_id) {
	if (!h || h->finalized)
		return SDBV_ERR_BAD_ARG;
	return hnsw::hnsw_remove(h, (uint32_t)e_id) ? 1 : 0;
}

// Host-side knn_search (same algorithm as the GPU per-hop path with host
// distances — the code path the build's efc-searches exercise). No device
// needed: lets CPU tests and quality audits search any host graph.
int sdbv_hnsw_knn_host(sdbv_hnsw *h, const float *q, uint32_t k, uint32_t ef,
                       uint64_t *out_ids, double *out_dists,
                       uint32_t *out_n) {
	using namespace hnsw;
	if (!h || !q || k == 0)
		return SDBV_ERR_BAD_ARG;
	if (h->enter_point < 0) {
		*out_n = 0;
		return SDBV_OK;
	}
	double q_norm = h->metric == SDBV_METRIC_COSINE
	                    ? sqrt(host_sumsq_f32(q, h->d))
	                    : 0;
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q, q_norm, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q, q_norm, cand, visited, w, 1,
		                  false);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}
	PQ cand, w;
	cand.push(ep_dist, ep_id);
	w.push(ep_dist, ep_id);
	std::unordered_set<uint32_t> visited{ep_id};
	search_layer_host(h, h->layers[0], q, q_norm, cand, visited, w, ef,
	                  false);
	auto v = w.to_vec();
	size_t m = std::min<size_t>(k, v.size());
	std::vector<std::pair<std::pair<uint64_t, uint32_t>, double>> fin(m);
	for (size_t i = 0; i < m; i++)
		fin[i] = {{total_key(v[i].first), v[i].second}, v[i].first};
	std::sort(fin.begin(), fin.end());
	*out_n = (uint32_t)m;
	for (size_t i = 0; i < m; i++) {
		out_ids[i] = fin[i].first.second;
		out_dists[i] = fin[i].second;
	}
	return SDBV_OK;
}

// Test hooks: drive the DoublePriorityQueue restatement directly so tests
// can replay the reference's own test_double_priority_queue sequence
// (knn.rs:735-790) against this implementation.
void *sdbv_test_pq_new() { return new hnsw::PQ(); }
void sdbv_test_pq_free(void *q) { delete (hnsw::PQ *)q; }
uint64_t sdbv_test_pq_len(void *q) { return ((hnsw::PQ *)q)->n; }
void sdbv_test_pq_push(void *q, double d, uint64_t id) {
	((hnsw::PQ *)q)->push(d, (uint32_t)id);
}
int sdbv_test_pq_peek_first(void *q, double *d, uint64_t *id) {
	uint32_t i;
	if (!((hnsw::PQ *)q)->peek_first(d, &i))
		return 0;
	*id = i;
	return 1;
}
int sdbv_test_pq_peek_last_dist(void *q, double *d) {
	auto *pq = (hnsw::PQ *)q;
	if (pq->n == 0)
		return 0;
	*d = pq->peek_last_dist(0);
	return 1;
}
int sdbv_test_pq_pop_first(void *q, double *d, uint64_t *id) {
	uint32_t i;
	if (!((hnsw::PQ *)q)->pop_first(d, &i))
		return 0;
	*id = i;
	return 1;
}
int sdbv_test_pq_pop_last(void *q, double *d, uint64_t *id) {
	auto *pq = (hnsw::PQ *)q;
	if (pq->n == 0)
		return 0;
	*d = pq->v.back().d;
	*id = pq->v.back().id;
	pq->pop_last();
	return 1;
}

} // extern "C"

// ===========================================================================
// Index layer — the operator surface of HnswIndex (hnsw/index.rs) with the
// parts the reference keeps behind the KV transaction held in host memory:
// the Hp pendings queue, the Hv vector->docs entries (VecDocs + Ids64), and
// the hi/hd record-key<->doc-id maps (HnswDocs). Record keys are opaque u64
// handles supplied by the host binding (INTEGRATION.md "record-key
// handles"). Searches run the pendings overlay on the host and the graph
// search on the GPU per-hop path once the index is finalized (re-finalizing
// automatically after writes); a host-only index (ctx == NULL) searches the
// host graph — that is the CPU-testable path, not a product fallback: a
// GPU-bound index always has a ctx.
// ===========================================================================

namespace vdocs {

// knn.rs:163-326 Ids64 — doc-id set with size-dependent representation.
// Vec1..Vec8 keep INSERTION order; the 9th insert collapses to Bits
// (iteration ascending); dropping back to exactly 8 keeps ascending order.
// insert/remove return "a new variant was produced" — the contract VecDocs
// persists on (Bits in-place mutations are dropped by the caller,
// docs.rs:374-382/:437-447; restated as-is).
struct Ids64 {
	std::vector<uint64_t> v;
	bool bits = false;
	size_t len() const { return v.size(); }
	bool empty() const { return v.empty(); }
	bool contains(uint64_t d) const {
		return std::find(v.begin(), v.end(), d) != v.end();
	}
	bool insert_ret_variant(uint64_t d) {
		if (contains(d))
			return false;
		if (!bits) {
			v.push_back(d);
			if (v.size() > 8) {
				std::sort(v.begin(), v.end());
				bits = true;
			}
			return true;
		}
		v.insert(std::lower_bound(v.begin(), v.end(), d), d);
		return false;
	}
	bool remove_ret_variant(uint64_t d, Ids64 *out) {
		if (bits) {
			auto it = std::lower_bound(v.begin(), v.end(), d);
			bool had = (it != v.end() && *it == d);
			if (had)
				v.erase(it);
			if (!had || v.size() != 8)
				return false;
			out->v = v;
			out->bits = false;
			return true;
		}
		switch (v.size()) {
		case 0:
			return false;
		case 1:
			if (v[0] == d) {
				out->v.clear();
				out->bits = false;
				return true;
			}
			return false;
		case 2:
			// knn.rs:266-268: first element != d becomes One — for a
			// non-member d this drops the second element (restated as-is)
			for (uint64_t x : v)
				if (x != d) {
					out->v = {x};
					out->bits = false;
					return true;
				}
			return false;
		default: {
			std::vector<uint64_t> f;
			for (uint64_t x : v)
				if (x != d)
					f.push_back(x);
			if (f.size() == v.size() - 1) {
				out->v = std::move(f);
				out->bits = false;
				return true;
			}
			return false;
		}
		}
	}
};

// knn.rs:363-437 KnnResultBuilder over VectorId (kind 0 = DocId < kind 1 =
// RecordKey, the enum's derived Ord).
struct Vid {
	uint8_t kind;
	uint64_t id;
	bool operator<(const Vid &o) const {
		if (kind != o.kind)
			return kind < o.kind;
		return id < o.id;
	}
};
struct Builder {
	size_t knn;
	struct Ent {
		uint64_t key;
		Vid vid;
		double dist;
		bool operator<(const Ent &o) const {
			if (key != o.key)
				return key < o.key;
			return vid < o.vid;
		}
	};
	std::set<Ent> pl;
	std::map<Vid, size_t> count;
	explicit Builder(size_t k) : knn(k) {}
	// knn.rs:386-394: plain f64 `>` against the current worst
	bool check_add(double submitted) const {
		if (pl.size() >= knn && !pl.empty() &&
		    submitted > std::prev(pl.end())->dist)
			return false;
		return true;
	}
	// knn.rs:410-433: returns true + *evicted when an id fell out of the
	// result entirely (count hit 0) — the filter-cache expiry signal.
	bool add_ret_evicted(double dist, Vid vid, Vid *evicted) {
		pl.insert(Ent{hnsw::total_key(dist), vid, dist});
		count[vid]++; // incremented even on duplicate set inserts
		if (pl.size() <= knn)
			return false;
		auto last = std::prev(pl.end());
		Vid ev = last->vid;
		pl.erase(last);
		auto it = count.find(ev);
		if (it != count.end()) {
			if (it->second <= 1) {
				count.erase(it);
				if (evicted)
					*evicted = ev;
				return true;
			}
			it->second--;
		}
		return false;
	}
	void add(double dist, Vid vid) { add_ret_evicted(dist, vid, nullptr); }
	void add_graph(double dist, const Ids64 &docs) {
		for (uint64_t doc : docs.v)
			add(dist, Vid{0, doc});
	}
};

} // namespace vdocs

struct sdbv_index {
	sdbv_hnsw *h;
	uint64_t table;
	struct ED {
		uint32_t e_id;
		vdocs::Ids64 docs;
	};
	// Hv entries: serialized vector bytes -> (element, docs)
	std::unordered_map<std::string, ED> vd;
	std::unordered_map<uint32_t, const std::string *> by_elem;
	// HnswDocs: hi/hd maps + recycled allocation (docs.rs:20-135)
	std::map<uint64_t, uint64_t> key2doc, doc2key;
	std::set<uint64_t> available;
	uint64_t next_doc_id = 0;
	// Hp pendings in appending order (index.rs:131-174)
	struct Pending {
		uint8_t kind; // 0 DocId, 1 RecordKey
		uint64_t id;
		std::vector<float> olds, news;
	};
	std::vector<Pending> pendings;
	// the reference's RwLock<HnswFlavor> (index.rs:55): one mutex here
	std::mutex mu;
};

namespace hnsw {
// layer.rs:320-338 are_all_docs_in_pending: an element with no VecDocs
// entry, or whose every doc is pending, counts as all-pending.
static bool idx_all_docs_pending(const IdxPend *p, uint32_t e_id) {
	if (!p->pending || p->pending->empty())
		return false;
	auto it = p->ix->by_elem.find(e_id);
	if (it != p->ix->by_elem.end()) {
		for (uint64_t doc : p->ix->vd.at(*it->second).docs.v)
			if (!p->pending->count(doc))
				return false;
	}
	return true;
}
} // namespace hnsw

// Distance of the query against a raw (not yet indexed) vector — the
// pendings overlay's Distance::calculate (idx/trees/vector.rs:660-672),
// same restated chain as the element path.
static double idx_dist_raw(const sdbv_hnsw *h, const float *q, double q_norm,
                           const float *v) {
	if (h->metric == SDBV_METRIC_COSINE) {
		double dot = hnsw::host_dot_f32(q, v, h->d);
		double v_norm = sqrt(hnsw::host_sumsq_f32(v, h->d));
		return 1.0 - dot / (q_norm * v_norm);
	}
	float acc = 0;
	for (uint32_t i = 0; i < h->d; i++) {
		float diff = q[i] - v[i];
		acc += diff * diff;
	}
	return sqrt((double)acc);
}

// docs.rs:64-90 resolve / :78-90 next_doc_id (smallest recycled id first).
static uint64_t idx_docs_resolve(sdbv_index *ix, uint64_t record_key) {
	auto it = ix->key2doc.find(record_key);
	if (it != ix->key2doc.end())
		return it->second;
	uint64_t doc_id;
	if (!ix->available.empty()) {
		doc_id = *ix->available.begin();
		ix->available.erase(ix->available.begin());
	} else {
		doc_id = ix->next_doc_id++;
	}
	ix->key2doc[record_key] = doc_id;
	ix->doc2key[doc_id] = record_key;
	return doc_id;
}

// docs.rs:113-135 HnswDocs::remove (recycle the id).
static void idx_docs_remove(sdbv_index *ix, uint64_t doc_id) {
	auto it = ix->doc2key.find(doc_id);
	if (it == ix->doc2key.end())
		return;
	ix->key2doc.erase(it->second);
	ix->doc2key.erase(it);
	ix->available.insert(doc_id);
}

// docs.rs:363-393 VecDocs::insert.
static int idx_vd_insert(sdbv_index *ix, const float *v, uint64_t doc_id) {
	std::string key((const char *)v, (size_t)ix->h->d * 4);
	auto it = ix->vd.find(key);
	if (it == ix->vd.end()) {
		uint32_t e_id = (uint32_t)ix->h->next_id;
		int rc = sdbv_hnsw_insert(ix->h, v);
		if (rc != SDBV_OK)
			return rc; // never silent: a dropped insert corrupts VecDocs
		auto r = ix->vd.emplace(std::move(key), sdbv_index::ED{e_id, {}});
		r.first->second.docs.v = {doc_id};
		ix->by_elem[e_id] = &r.first->first;
	} else {
		sdbv_index::ED ed = it->second; // owned copy, like tx.get
		if (ed.docs.insert_ret_variant(doc_id))
			it->second = ed; // persisted only on a new variant
	}
	return SDBV_OK;
}

// docs.rs:424-449 VecDocs::remove.
static void idx_vd_remove(sdbv_index *ix, const float *v, uint64_t doc_id) {
	std::string key((const char *)v, (size_t)ix->h->d * 4);
	auto it = ix->vd.find(key);
	if (it == ix->vd.end())
		return;
	sdbv_index::ED ed = it->second;
	vdocs::Ids64 new_docs;
	if (ed.docs.remove_ret_variant(doc_id, &new_docs)) {
		if (new_docs.empty()) {
			uint32_t e_id = ed.e_id;
			ix->by_elem.erase(e_id);
			ix->vd.erase(it);
			hnsw::hnsw_remove(ix->h, e_id);
		} else {
			ed.docs = new_docs;
			it->second = ed;
		}
	}
	// else: no new variant — the mutation is dropped (docs.rs:437-447)
}

// Host full graph search with pendings (knn_search, mod.rs:459-482 +
// search_ep :521-548): used for a host-only index (CPU tests).
static uint32_t idx_graph_search_host(sdbv_index *ix, const float *q,
                                      uint32_t k, uint32_t ef,
                                      const hnsw::IdxPend *pend,
                                      std::vector<std::pair<double, uint32_t>>
                                          &out) {
	using namespace hnsw;
	sdbv_hnsw *h = ix->h;
	if (h->enter_point < 0)
		return 0;
	double q_norm = h->metric == SDBV_METRIC_COSINE
	                    ? sqrt(host_sumsq_f32(q, h->d))
	                    : 0;
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q, q_norm, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q, q_norm, cand, visited, w, 1,
		                  false, pend);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}
	PQ cand;
	cand.push(ep_dist, ep_id);
	std::unordered_set<uint32_t> visited{ep_id};
	PQ w = cand;
	search_layer_host(h, h->layers[0], q, q_norm, cand, visited, w, ef,
	                  false, pend);
	auto v = w.to_vec(); // to_vec_limit(k), knn.rs:92-104
	uint32_t n = (uint32_t)std::min<size_t>(k, v.size());
	for (uint32_t i = 0; i < n; i++)
		out.push_back({v[i].first, v[i].second});
	return n;
}

// GPU per-hop graph search with pendings: the sdbv_hnsw_knn layer-0 loop
// (host queue + k_gather_dist batched expansion) with the pending gate on
// the candidates push. Caller holds ix->mu; takes ctx->mu itself.
static int idx_graph_search_gpu(sdbv_index *ix, const float *q, uint32_t k,
                                uint32_t ef, const hnsw::IdxPend *pend,
                                std::vector<std::pair<double, uint32_t>> &out,
                                uint32_t *out_n) {
	using namespace hnsw;
	sdbv_hnsw *h = ix->h;
	*out_n = 0;
	if (h->enter_point < 0)
		return SDBV_OK;
	sdbv_ctx *ctx = h->ctx;
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(h->table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	double q_norm = h->metric == SDBV_METRIC_COSINE
	                    ? sqrt(host_sumsq_f32(q, h->d))
	                    : 0;
	// upper layers: host descent (tiny)
	uint32_t ep_id = (uint32_t)h->enter_point;
	double ep_dist = dist(h, q, q_norm, ep_id);
	for (size_t l = h->layers.size() - 1; l >= 1; l--) {
		PQ cand;
		cand.push(ep_dist, ep_id);
		std::unordered_set<uint32_t> visited{ep_id};
		PQ w = cand;
		search_layer_host(h, h->layers[l], q, q_norm, cand, visited, w, 1,
		                  false, pend);
		double dd;
		uint32_t ii;
		if (w.peek_first(&dd, &ii)) {
			ep_dist = dd;
			ep_id = ii;
		}
	}
	// layer 0: ef-search, one gather+distance launch per hop
	HIP_CHECK(ctx, hipMemcpyAsync(h->q_dev, q, h->d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	const Layer &l0 = h->layers[0];
	PQ candidates, w;
	candidates.push(ep_dist, ep_id);
	w.push(ep_dist, ep_id);
	std::vector<bool> visited(h->next_id, false);
	visited[ep_id] = true;
	double fq = w.peek_last_dist(DBL_MAX);
	std::vector<uint32_t> frontier;
	std::vector<double> fdists(h->max_deg); // actual max degree
	double cd;
	uint32_t doc;
	while (candidates.pop_first(&cd, &doc)) {
		if (cd > fq)
			break;
		frontier.clear();
		for (uint32_t e : l0.edges[doc])
			if (!visited[e]) {
				visited[e] = true;
				if (!h->elem_present[e])
					continue;
				frontier.push_back(e);
			}
		if (frontier.empty())
			continue;
		std::memcpy(h->rows_pinned, frontier.data(),
		            frontier.size() * sizeof(uint32_t));
		HIP_CHECK(ctx, hipMemcpyAsync(h->rows_dev, h->rows_pinned,
		                              frontier.size() * sizeof(uint32_t),
		                              hipMemcpyHostToDevice, ctx->stream));
		if (t.metric == SDBV_METRIC_COSINE)
			hipLaunchKernelGGL(k_gather_dist<0>,
			                   dim3((uint32_t)frontier.size()), dim3(64), 0,
			                   ctx->stream, t.cm, t.norms, t.n_pad, t.d,
			                   h->rows_dev, (uint32_t)frontier.size(),
			                   h->q_dev, q_norm, h->dout_dev);
		else
			hipLaunchKernelGGL(k_gather_dist<1>,
			                   dim3((uint32_t)frontier.size()), dim3(64), 0,
			                   ctx->stream, t.cm, t.norms, t.n_pad, t.d,
			                   h->rows_dev, (uint32_t)frontier.size(),
			                   h->q_dev, q_norm, h->dout_dev);
		HIP_CHECK(ctx, hipMemcpyAsync(h->dists_pinned, h->dout_dev,
		                              frontier.size() * sizeof(double),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		std::memcpy(fdists.data(), h->dists_pinned,
		            frontier.size() * sizeof(double));
		// sequential accept in edge order (layer.rs:195-218) with the
		// pending gate on candidates only (:209-212)
		for (size_t i = 0; i < frontier.size(); i++) {
			double ed = fdists[i];
			uint32_t e = frontier[i];
			if (ed < fq || w.n < ef) {
				if (!pend || !idx_all_docs_pending(pend, e))
					candidates.push(ed, e);
				w.push(ed, e);
				if (w.n > ef)
					w.pop_last();
				fq = w.peek_last_dist(DBL_MAX);
			}
		}
	}
	auto v = w.to_vec();
	uint32_t n = (uint32_t)std::min<size_t>(k, v.size());
	for (uint32_t i = 0; i < n; i++)
		out.push_back({v[i].first, v[i].second});
	*out_n = n;
	return SDBV_OK;
}

// ===========================================================================
// KV codec + cold-start staging pipeline: the
// reference's on-disk HNSW state — He element vectors (key/index/he.rs),
// Hn per-node edge lists (hn.rs), Hs graph state (hs.rs), Hv vector->docs
// entries (hv.rs) — parsed/emitted byte-exactly so a dumped surrealdb
// index bulk-loads straight into the host graph + device SoA with no
// re-insertion. Key layout (storekey, pinned by the reference's own key
// tests): `/*<ns u32 BE>*<db u32 BE>*<tb>\0+<ix u32 BE>!h<e|n|s|v>` +
// per-key fields (element u64 BE; layer u16 BE + node u64 BE; escaped
// revisioned vector). Embedded slices escape 0x00 -> 0x01 0x00 and
// 0x01 -> 0x01 0x01 with a 0x00 terminator (derived from the hv.rs
// golden bytes). Values use the `revision` crate 0.17.0 wire format
// (dependency pinned by Cargo.lock, source not vendored): varint revision
// tag + varint enum variant + varint lengths + fixed little-endian
// primitives — pinned by the hv.rs golden vectors at small sizes; beyond
// the single-byte range (values >= 251) the varints use bincode-style
// markers (0xFB + u16 LE, 0xFC + u32 LE, 0xFD + u64 LE), pinned by the
// catalog compat fixtures' 900/3600/86400 durations.
// ===========================================================================

namespace kvc {

// bincode-style unsigned varint (revision 0.17.0): < 251 one byte;
// 0xfb + u16 LE; 0xfc + u32 LE; 0xfd + u64 LE.
static void put_varint(std::vector<uint8_t> &b, uint64_t v) {
	if (v < 251) {
		b.push_back((uint8_t)v);
	} else if (v <= 0xFFFF) {
		b.push_back(0xFB);
		b.push_back((uint8_t)v);
		b.push_back((uint8_t)(v >> 8));
	} else if (v <= 0xFFFFFFFFull) {
		b.push_back(0xFC);
		for (int i = 0; i < 4; i++)
			b.push_back((uint8_t)(v >> (8 * i)));
	} else {
		b.push_back(0xFD);
		for (int i = 0; i < 8; i++)
			b.push_back((uint8_t)(v >> (8 * i)));
	}
}
static bool get_varint(const uint8_t *&p, const uint8_t *end, uint64_t *v) {
	if (p >= end)
		return false;
	uint8_t c = *p++;
	int extra;
	if (c < 251) {
		*v = c;
		return true;
	} else if (c == 0xFB) {
		extra = 2;
	} else if (c == 0xFC) {
		extra = 4;
	} else if (c == 0xFD) {
		extra = 8;
	} else {
		return false; // 0xFE (u128) unsupported
	}
	if (end - p < extra)
		return false;
	uint64_t out = 0;
	for (int i = 0; i < extra; i++)
		out |= (uint64_t)(*p++) << (8 * i);
	*v = out;
	return true;
}
template <typename T> static void put_le(std::vector<uint8_t> &b, T v) {
	uint8_t tmp[sizeof(T)];
	std::memcpy(tmp, &v, sizeof(T));
	b.insert(b.end(), tmp, tmp + sizeof(T));
}
template <typename T>
static bool get_le(const uint8_t *&p, const uint8_t *end, T *v) {
	if ((size_t)(end - p) < sizeof(T))
		return false;
	std::memcpy(v, p, sizeof(T));
	p += sizeof(T);
	return true;
}
template <typename T> static void put_be(std::vector<uint8_t> &b, T v) {
	for (int i = (int)sizeof(T) - 1; i >= 0; i--)
		b.push_back((uint8_t)(v >> (8 * i)));
}
template <typename T>
static bool get_be(const uint8_t *&p, const uint8_t *end, T *v) {
	if ((size_t)(end - p) < sizeof(T))
		return false;
	T out = 0;
	for (size_t i = 0; i < sizeof(T); i++)
		out = (out << 8) | *p++;
	*v = out;
	return true;
}

// storekey escaped-slice codec (embedded dynamic fields in keys)
static void put_escaped(std::vector<uint8_t> &b, const uint8_t *s, size_t n) {
	for (size_t i = 0; i < n; i++) {
		if (s[i] == 0x00 || s[i] == 0x01) {
			b.push_back(0x01);
			b.push_back(s[i]);
		} else {
			b.push_back(s[i]);
		}
	}
	b.push_back(0x00);
}
static bool get_escaped(const uint8_t *&p, const uint8_t *end,
                        std::vector<uint8_t> &out) {
	while (p < end) {
		uint8_t c = *p++;
		if (c == 0x00)
			return true; // terminator
		if (c == 0x01) {
			if (p >= end)
				return false;
			out.push_back(*p++);
		} else {
			out.push_back(c);
		}
	}
	return false;
}

// revisioned SerializedVector (idx/trees/vector.rs:33-41; F64=0 F32=1
// I64=2 I32=3 I16=4), F32 payloads only on the encode side (the HNSW
// default vector type, define.rs:1107).
static void enc_vec_f32(std::vector<uint8_t> &b, const float *v, uint32_t d) {
	put_varint(b, 1); // revision
	put_varint(b, 1); // variant F32
	put_varint(b, d);
	for (uint32_t i = 0; i < d; i++)
		put_le(b, v[i]);
}
static bool dec_vec_f32_cursor(const uint8_t *&p, const uint8_t *end,
                               std::vector<float> &out) {
	uint64_t rev, variant, len;
	if (!get_varint(p, end, &rev) || rev != 1)
		return false;
	if (!get_varint(p, end, &variant))
		return false;
	if (!get_varint(p, end, &len))
		return false;
	// bound before reserving: every element needs >= 4 payload bytes
	if (len > (uint64_t)(end - p) / 4 + 1)
		return false;
	out.clear();
	out.reserve(len);
	for (uint64_t i = 0; i < len; i++) {
		switch (variant) {
		case 1: { // F32
			float f;
			if (!get_le(p, end, &f))
				return false;
			out.push_back(f);
			break;
		}
		default:
			return false; // F64/I* corpora are not staged as f32 blindly
		}
	}
	return true;
}
static bool dec_vec_f32(const uint8_t *p, const uint8_t *end,
                        std::vector<float> &out) {
	return dec_vec_f32_cursor(p, end, out);
}

// graph.rs:104-113 node_to_val: u16 BE edge count + u64 BE edge ids.
static void enc_node(std::vector<uint8_t> &b,
                     const std::vector<uint32_t> &edges) {
	put_be(b, (uint16_t)edges.size());
	for (uint32_t e : edges)
		put_be(b, (uint64_t)e);
}
static bool dec_node(const uint8_t *p, const uint8_t *end,
                     std::vector<uint32_t> &out) {
	uint16_t n;
	if (!get_be(p, end, &n))
		return false;
	out.clear();
	out.reserve(n);
	for (uint16_t i = 0; i < n; i++) {
		uint64_t e;
		if (!get_be(p, end, &e))
			return false;
		out.push_back((uint32_t)e);
	}
	return true;
}

// revisioned HnswState (hnsw/mod.rs:61-71): Option<ElementId> enter_point
// (u8 tag 0/1 + u64 LE), next_element_id u64 LE, layer0 LayerState
// {version u64 LE, chunks u32 LE}, layers Vec<LayerState>.
struct HnswStateKV {
	bool has_ep = false;
	uint64_t enter_point = 0;
	uint64_t next_element_id = 0;
	uint64_t n_upper_layers = 0; // layers.len()
};
static void enc_state(std::vector<uint8_t> &b, const HnswStateKV &s) {
	put_varint(b, 1); // revision
	b.push_back(s.has_ep ? 1 : 0); // Option tag
	if (s.has_ep)
		put_varint(b, s.enter_point); // ElementId: unsigned -> varint
	put_varint(b, s.next_element_id);
	put_varint(b, 1);            // layer0 LayerState revision
	put_varint(b, 0);            // layer0.version (not tracked here)
	put_varint(b, 0);            // layer0.chunks == 0 (post-Hl format)
	put_varint(b, s.n_upper_layers);
	for (uint64_t i = 0; i < s.n_upper_layers; i++) {
		put_varint(b, 1); // LayerState revision
		put_varint(b, 0);
		put_varint(b, 0);
	}
}
static bool dec_state(const uint8_t *p, const uint8_t *end, HnswStateKV *s) {
	uint64_t rev;
	if (!get_varint(p, end, &rev) || rev != 1)
		return false;
	if (p >= end)
		return false;
	uint8_t tag = *p++;
	s->has_ep = tag != 0;
	if (s->has_ep && !get_varint(p, end, &s->enter_point))
		return false;
	if (!get_varint(p, end, &s->next_element_id))
		return false;
	uint64_t lrev, version, chunks;
	if (!get_varint(p, end, &lrev) || lrev != 1 ||
	    !get_varint(p, end, &version) || !get_varint(p, end, &chunks))
		return false; // layer0 state
	if (chunks != 0)
		return false; // legacy Hl chunks unsupported (post-migration only)
	if (!get_varint(p, end, &s->n_upper_layers))
		return false;
	for (uint64_t i = 0; i < s->n_upper_layers; i++)
		if (!get_varint(p, end, &lrev) || lrev != 1 ||
		    !get_varint(p, end, &version) ||
		    !get_varint(p, end, &chunks) || chunks != 0)
			return false;
	return true;
}

// revisioned ElementDocs (docs.rs:164-177): e_id varint + Ids64 (variant
// varint: Empty=0 One=1 Vec2=2..Vec8=8 Bits=9; doc ids as unsigned
// varints like every unsigned field). The reference's Bits variant is a
// serialized RoaringTreemap — not implemented here, so encode REFUSES a
// bits-mode set (callers return SDBV_ERR_UNSUPPORTED rather than emit a
// record a real surrealdb could not deserialize) and decode rejects
// variant 9.
static bool enc_element_docs(std::vector<uint8_t> &b, uint64_t e_id,
                             const vdocs::Ids64 &docs) {
	size_t n = docs.v.size();
	if (docs.bits || n > 8)
		return false; // Bits (roaring) — refuse, never emit malformed
	put_varint(b, 1);     // revision
	put_varint(b, e_id);  // ElementId: unsigned -> varint
	put_varint(b, 1);     // Ids64 revision
	put_varint(b, n);
	for (uint64_t d : docs.v)
		put_varint(b, d); // DocId: unsigned -> varint
	return true;
}
static bool dec_element_docs(const uint8_t *p, const uint8_t *end,
                             uint64_t *e_id, vdocs::Ids64 *docs) {
	uint64_t rev, variant;
	if (!get_varint(p, end, &rev) || rev != 1)
		return false;
	if (!get_varint(p, end, e_id))
		return false;
	if (!get_varint(p, end, &rev) || rev != 1)
		return false;
	if (!get_varint(p, end, &variant))
		return false;
	docs->v.clear();
	docs->bits = false;
	if (variant == 0)
		return true;
	if (variant > 8)
		return false; // Bits / roaring not supported in this revision
	for (uint64_t i = 0; i < variant; i++) {
		uint64_t d;
		if (!get_varint(p, end, &d))
			return false;
		docs->v.push_back(d);
	}
	return true;
}

// revisioned VectorPendingUpdate (hnsw/mod.rs:93-116): VectorId enum
// (DocId(u64 varint) = 0 | RecordKey(RecordIdKey) = 1; RecordIdKey
// revisioned enum — only Number(i64, fixed LE) maps onto the u64
// record-key handles of this boundary, other key kinds are the host's to
// apply) + old/new Vec<SerializedVector>.
struct PendingKV {
	uint8_t kind; // 0 DocId, 1 RecordKey(Number handle)
	uint64_t id;
	std::vector<float> olds, news; // n*d concatenated
};
static bool dec_vec_list(const uint8_t *&p, const uint8_t *end, uint32_t d,
                         std::vector<float> &out) {
	uint64_t n;
	if (!get_varint(p, end, &n))
		return false;
	out.clear();
	std::vector<float> one;
	for (uint64_t i = 0; i < n; i++) {
		if (!dec_vec_f32_cursor(p, end, one) || one.size() != d)
			return false;
		out.insert(out.end(), one.begin(), one.end());
	}
	return true;
}
static bool dec_pending(const uint8_t *p, const uint8_t *end, uint32_t d,
                        PendingKV *out) {
	uint64_t rev, variant;
	if (!get_varint(p, end, &rev) || rev != 1)
		return false; // VectorPendingUpdate revision
	if (!get_varint(p, end, &rev) || rev != 1)
		return false; // VectorId revision
	if (!get_varint(p, end, &variant))
		return false;
	if (variant == 0) { // DocId(u64)
		out->kind = 0;
		if (!get_varint(p, end, &out->id))
			return false;
	} else if (variant == 1) { // RecordKey(RecordIdKey)
		uint64_t krev, kvar;
		if (!get_varint(p, end, &krev) || krev != 1)
			return false;
		if (!get_varint(p, end, &kvar))
			return false;
		if (kvar != 0)
			return false; // only Number keys map to u64 handles here
		int64_t num;
		if (!get_le(p, end, &num))
			return false; // i64: signed -> fixed LE
		out->kind = 1;
		out->id = (uint64_t)num;
	} else {
		return false;
	}
	if (!dec_vec_list(p, end, d, out->olds))
		return false;
	if (!dec_vec_list(p, end, d, out->news))
		return false;
	return true;
}
static void enc_pending(std::vector<uint8_t> &b, uint32_t d,
                        const PendingKV &pk) {
	put_varint(b, 1); // VectorPendingUpdate revision
	put_varint(b, 1); // VectorId revision
	put_varint(b, pk.kind);
	if (pk.kind == 0) {
		put_varint(b, pk.id);
	} else {
		put_varint(b, 1);          // RecordIdKey revision
		put_varint(b, 0);          // Number variant
		put_le(b, (int64_t)pk.id); // signed fixed LE
	}
	put_varint(b, pk.olds.size() / d);
	for (size_t i = 0; i * d < pk.olds.size(); i++)
		enc_vec_f32(b, pk.olds.data() + i * d, d);
	put_varint(b, pk.news.size() / d);
	for (size_t i = 0; i * d < pk.news.size(); i++)
		enc_vec_f32(b, pk.news.data() + i * d, d);
}

// Key prefix `/*<ns>*<db>*<tb>\0+<ix>!h` + kind char.
static void key_prefix(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                       const char *tb, uint32_t ix) {
	b.push_back('/');
	b.push_back('*');
	put_be(b, ns);
	b.push_back('*');
	put_be(b, db);
	b.push_back('*');
	b.insert(b.end(), tb, tb + strlen(tb));
	b.push_back(0);
	b.push_back('+');
	put_be(b, ix);
	b.push_back('!');
	b.push_back('h');
}
static void key_he(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                   const char *tb, uint32_t ix, uint64_t element_id) {
	key_prefix(b, ns, db, tb, ix);
	b.push_back('e');
	put_be(b, element_id);
}
static void key_hn(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                   const char *tb, uint32_t ix, uint16_t layer,
                   uint64_t node) {
	key_prefix(b, ns, db, tb, ix);
	b.push_back('n');
	put_be(b, layer);
	put_be(b, node);
}
static void key_hs(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                   const char *tb, uint32_t ix) {
	key_prefix(b, ns, db, tb, ix);
	b.push_back('s');
}
static void key_hp(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                   const char *tb, uint32_t ix, uint64_t appending_id) {
	key_prefix(b, ns, db, tb, ix);
	b.push_back('p');
	put_be(b, appending_id);
}
static void key_hv(std::vector<uint8_t> &b, uint32_t ns, uint32_t db,
                   const char *tb, uint32_t ix, const float *v, uint32_t d) {
	key_prefix(b, ns, db, tb, ix);
	b.push_back('v');
	std::vector<uint8_t> ser;
	enc_vec_f32(ser, v, d);
	put_escaped(b, ser.data(), ser.size());
}

// Parses a key: positions the kind char + the remainder. Returns 0 on a
// well-formed `!h?` key, else -1.
struct ParsedKey {
	char kind;
	const uint8_t *rest;
	const uint8_t *end;
};
static int parse_key(const uint8_t *k, size_t n, ParsedKey *out) {
	const uint8_t *p = k, *end = k + n;
	if (end - p < 12 || *p++ != '/' || *p++ != '*')
		return -1;
	p += 4; // ns
	if (p >= end || *p++ != '*')
		return -1;
	p += 4; // db
	if (p >= end || *p++ != '*')
		return -1;
	while (p < end && *p != 0)
		p++; // tb
	if (p >= end)
		return -1;
	p++; // NUL
	if (p >= end || *p++ != '+')
		return -1;
	p += 4; // ix
	if (end - p < 3 || *p++ != '!' || *p++ != 'h')
		return -1;
	out->kind = (char)*p++;
	out->rest = p;
	out->end = end;
	return 0;
}

} // namespace kvc

// ---------------------------------------------------------------------------
// Filtered KNN (hnsw/filter.rs + layer.rs:110-318): the WHERE-condition
// evaluation (is_record_truthy — KV fetch + expression compute) stays on
// the host side as a callback; the library keeps the FilterCache semantics
// (one evaluation per VectorId while cached, expired on builder eviction)
// and the accept/expand gating. Callback must be deterministic per call.
// ---------------------------------------------------------------------------

typedef int (*sdbv_truthy_cb)(void *user, uint8_t kind, uint64_t id);
typedef void (*sdbv_expire_cb)(void *user, uint8_t kind, uint64_t id);

namespace vdocs {

struct Filter {
	sdbv_truthy_cb cb;
	sdbv_expire_cb ex;
	void *user;
	std::map<std::pair<uint8_t, uint64_t>, bool> cache; // filter.rs:22
	bool truthy(uint8_t kind, uint64_t id) {
		auto key = std::make_pair(kind, id);
		auto it = cache.find(key);
		if (it != cache.end())
			return it->second;
		bool t = cb(user, kind, id) != 0;
		cache[key] = t;
		return t;
	}
	void expire(uint8_t kind, uint64_t id) { // filter.rs:141-144
		cache.erase({kind, id});
		if (ex)
			ex(user, kind, id);
	}
	bool any_doc_truthy(const Ids64 &docs) { // filter.rs:53-66
		for (uint64_t d : docs.v)
			if (truthy(0, d))
				return true;
		return false;
	}
};

} // namespace vdocs

// layer.rs:308-318 check_all_docs_in_pending (plain Ids64 variant).
static bool idx_check_all_docs_in_pending(const vdocs::Ids64 &docs,
                                          const std::set<uint64_t> *pending) {
	if (!pending || pending->empty())
		return false;
	for (uint64_t d : docs.v)
		if (!pending->count(d))
			return false;
	return true;
}

// layer.rs:278-306 add_if_truthy: docs looked up BY VECTOR.
static bool idx_add_if_truthy(sdbv_index *ix, uint32_t ef, hnsw::PQ &w,
                              const float *e_pt, double e_dist, uint32_t e_id,
                              vdocs::Filter &filter,
                              const std::set<uint64_t> *pending) {
	std::string key((const char *)e_pt, (size_t)ix->h->d * 4);
	auto it = ix->vd.find(key);
	if (it == ix->vd.end())
		return false;
	const vdocs::Ids64 &docs = it->second.docs;
	if (idx_check_all_docs_in_pending(docs, pending))
		return false;
	if (filter.any_doc_truthy(docs)) {
		w.push(e_dist, e_id);
		if (w.n > ef)
			w.pop_last();
		return true;
	}
	return false;
}

// layer.rs:226-275 search_with_filter, host distances (host-only index).
static void idx_search_l0_filter_host(sdbv_index *ix, const float *q,
                                      double q_norm, hnsw::PQ &candidates,
                                      std::vector<bool> &visited, hnsw::PQ &w,
                                      uint32_t ef, vdocs::Filter &filter,
                                      const std::set<uint64_t> *pending) {
	using namespace hnsw;
	sdbv_hnsw *h = ix->h;
	const Layer &l0 = h->layers[0];
	double f_dist = w.peek_last_dist(DBL_MAX);
	double cd;
	uint32_t doc;
	while (candidates.pop_first(&cd, &doc)) {
		if (cd > f_dist)
			break;
		for (uint32_t e : l0.edges[doc]) {
			if (visited[e])
				continue;
			visited[e] = true;
			if (!h->elem_present[e])
				continue;
			double ed = dist(h, q, q_norm, e);
			if (ed < f_dist || w.n < ef) {
				candidates.push(ed, e);
				if (idx_add_if_truthy(ix, ef, w, vec(h, e), ed, e, filter,
				                      pending))
					f_dist = w.peek_last_dist(DBL_MAX);
			}
		}
	}
}

// Same loop with the per-hop GPU gather for distances (finalized index).
// Caller holds ix->mu; takes ctx->mu itself.
static int idx_search_l0_filter_gpu(sdbv_index *ix, const float *q,
                                    double q_norm, hnsw::PQ &candidates,
                                    std::vector<bool> &visited, hnsw::PQ &w,
                                    uint32_t ef, vdocs::Filter &filter,
                                    const std::set<uint64_t> *pending) {
	using namespace hnsw;
	sdbv_hnsw *h = ix->h;
	sdbv_ctx *ctx = h->ctx;
	std::lock_guard<std::mutex> lk(ctx->mu);
	auto it = ctx->tables.find(h->table);
	if (it == ctx->tables.end())
		return SDBV_ERR_NO_TABLE;
	Table &t = it->second;
	HIP_CHECK(ctx, hipMemcpyAsync(h->q_dev, q, h->d * sizeof(float),
	                              hipMemcpyHostToDevice, ctx->stream));
	const Layer &l0 = h->layers[0];
	double f_dist = w.peek_last_dist(DBL_MAX);
	std::vector<uint32_t> frontier;
	std::vector<double> fdists(h->max_deg); // actual max degree
	double cd;
	uint32_t doc;
	while (candidates.pop_first(&cd, &doc)) {
		if (cd > f_dist)
			break;
		frontier.clear();
		for (uint32_t e : l0.edges[doc])
			if (!visited[e]) {
				visited[e] = true;
				if (!h->elem_present[e])
					continue;
				frontier.push_back(e);
			}
		if (frontier.empty())
			continue;
		std::memcpy(h->rows_pinned, frontier.data(),
		            frontier.size() * sizeof(uint32_t));
		HIP_CHECK(ctx, hipMemcpyAsync(h->rows_dev, h->rows_pinned,
		                              frontier.size() * sizeof(uint32_t),
		                              hipMemcpyHostToDevice, ctx->stream));
		if (t.metric == SDBV_METRIC_COSINE)
			hipLaunchKernelGGL(k_gather_dist<0>,
			                   dim3((uint32_t)frontier.size()), dim3(64), 0,
			                   ctx->stream, t.cm, t.norms, t.n_pad, t.d,
			                   h->rows_dev, (uint32_t)frontier.size(),
			                   h->q_dev, q_norm, h->dout_dev);
		else
			hipLaunchKernelGGL(k_gather_dist<1>,
			                   dim3((uint32_t)frontier.size()), dim3(64), 0,
			                   ctx->stream, t.cm, t.norms, t.n_pad, t.d,
			                   h->rows_dev, (uint32_t)frontier.size(),
			                   h->q_dev, q_norm, h->dout_dev);
		HIP_CHECK(ctx, hipMemcpyAsync(h->dists_pinned, h->dout_dev,
		                              frontier.size() * sizeof(double),
		                              hipMemcpyDeviceToHost, ctx->stream));
		HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		std::memcpy(fdists.data(), h->dists_pinned,
		            frontier.size() * sizeof(double));
		for (size_t i = 0; i < frontier.size(); i++) {
			double ed = fdists[i];
			uint32_t e = frontier[i];
			if (ed < f_dist || w.n < ef) {
				candidates.push(ed, e);
				if (idx_add_if_truthy(ix, ef, w, vec(h, e), ed, e, filter,
				                      pending))
					f_dist = w.peek_last_dist(DBL_MAX);
			}
		}
	}
	return SDBV_OK;
}

extern "C" {

int sdbv_index_create(sdbv_ctx *ctx, uint64_t table, uint32_t d,
                      uint8_t metric, uint32_t m, uint32_t m0, uint32_t efc,
                      int extend, int keep, uint64_t seed, double ml,
                      sdbv_index **out) {
	sdbv_hnsw *h = nullptr;
	int rc = sdbv_hnsw_create(ctx, d, metric, m, m0, efc, extend, keep, seed,
	                          ml, &h);
	if (rc)
		return rc;
	auto *ix = new sdbv_index();
	ix->h = h;
	ix->table = table;
	*out = ix;
	return SDBV_OK;
}

void sdbv_index_destroy(sdbv_index *ix) {
	if (!ix)
		return;
	sdbv_hnsw_destroy(ix->h);
	delete ix;
}

sdbv_hnsw *sdbv_index_hnsw(sdbv_index *ix) { return ix ? ix->h : nullptr; }

// Level-RNG state carry-over (an EXTENSION record): the reference draws
// insert levels from an entropy-seeded SmallRng (hnsw/mod.rs:263-266), so
// the sequence restarts arbitrarily on every process start and ANY state
// is reference-conformant. For this framework's determinism convention
// (same seed => same graph) a host may persist the state across cold
// starts and restore it after load.
uint64_t sdbv_index_level_rng(sdbv_index *ix) {
	return ix ? ix->h->rng_state : 0;
}
void sdbv_index_set_level_rng(sdbv_index *ix, uint64_t state) {
	if (ix)
		ix->h->rng_state = state;
}
uint64_t sdbv_index_doc_count(sdbv_index *ix) { return ix->doc2key.size(); }
uint64_t sdbv_index_pending_count(sdbv_index *ix) {
	return ix->pendings.size();
}

// HnswIndex::index (index.rs:138-186): resolve the id kind via the hi map
// and append one VectorPendingUpdate (old/new = n*d f32 each).
int sdbv_index_enqueue(sdbv_index *ix, uint64_t record_key, const float *olds,
                       uint32_t n_old, const float *news, uint32_t n_new) {
	if (!ix)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	sdbv_index::Pending p;
	auto it = ix->key2doc.find(record_key);
	if (it != ix->key2doc.end()) {
		p.kind = 0;
		p.id = it->second;
	} else {
		p.kind = 1;
		p.id = record_key;
	}
	uint32_t d = ix->h->d;
	p.olds.assign(olds, olds + (size_t)n_old * d);
	p.news.assign(news, news + (size_t)n_new * d);
	ix->pendings.push_back(std::move(p));
	return SDBV_OK;
}

// index_pendings + index_pending (index.rs:188-257): drain in appending
// order; old-vector removals only for DocId pendings; empty new_vectors
// deletes the doc mapping; RecordKey ids resolve (allocate) at apply time.
int sdbv_index_apply_pendings(sdbv_index *ix, uint64_t *out_count) {
	if (!ix)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	uint64_t count = 0;
	uint32_t d = ix->h->d;
	for (auto &p : ix->pendings) {
		if (p.kind == 0) {
			for (size_t i = 0; i * d < p.olds.size(); i++)
				idx_vd_remove(ix, p.olds.data() + i * d, p.id);
			if (p.news.empty())
				idx_docs_remove(ix, p.id);
		}
		if (!p.news.empty()) {
			uint64_t doc_id =
			    (p.kind == 0) ? p.id : idx_docs_resolve(ix, p.id);
			for (size_t i = 0; i * d < p.news.size(); i++) {
				int rc = idx_vd_insert(ix, p.news.data() + i * d, doc_id);
				if (rc != SDBV_OK)
					return rc;
			}
		}
		count++;
	}
	ix->pendings.clear();
	if (out_count)
		*out_count = count;
	return SDBV_OK;
}

// knn_search (index.rs:270-335 without record materialisation):
// search_pendings overlay + graph search (GPU per-hop once finalized,
// auto-refinalizing after writes) + VecDocs doc expansion through one
// KnnResultBuilder. Out arrays sized k; *out_n = entries returned. Entries
// ascending (dist total_cmp, VectorId); kind 0 = DocId, 1 = RecordKey.
int sdbv_index_knn(sdbv_index *ix, const float *q, uint32_t k, uint32_t ef,
                   uint8_t *out_kinds, uint64_t *out_ids, double *out_dists,
                   uint32_t *out_n) {
	if (!ix || !q || k == 0)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	sdbv_hnsw *h = ix->h;
	vdocs::Builder builder(k);
	// search_pendings (index.rs:366-421)
	std::set<uint64_t> all_existing;
	std::map<vdocs::Vid, const std::vector<float> *> non_deleted;
	for (auto &p : ix->pendings) {
		if (p.kind == 0)
			all_existing.insert(p.id);
		vdocs::Vid vid{p.kind, p.id};
		if (p.news.empty())
			non_deleted.erase(vid);
		else
			non_deleted[vid] = &p.news;
	}
	if (!(all_existing.empty() && non_deleted.empty())) {
		double q_norm = h->metric == SDBV_METRIC_COSINE
		                    ? sqrt(hnsw::host_sumsq_f32(q, h->d))
		                    : 0;
		for (auto &e : non_deleted) {
			const std::vector<float> &vecs = *e.second;
			for (size_t i = 0; i * h->d < vecs.size(); i++) {
				double dd =
				    idx_dist_raw(h, q, q_norm, vecs.data() + i * h->d);
				if (builder.check_add(dd))
					builder.add(dd, e.first);
			}
		}
	}
	hnsw::IdxPend pend{&all_existing, ix};
	const hnsw::IdxPend *pp = all_existing.empty() ? nullptr : &pend;
	// graph search: GPU per-hop when a device context exists (finalizing
	// on first use / after writes), host path otherwise
	std::vector<std::pair<double, uint32_t>> neighbors;
	if (h->ctx && h->next_id > 0) {
		if (h->dirty || !h->finalized) {
			int rc = sdbv_hnsw_finalize(h, ix->table);
			if (rc)
				return rc;
		}
		uint32_t ng = 0;
		int rc = idx_graph_search_gpu(ix, q, k, ef, pp, neighbors, &ng);
		if (rc)
			return rc;
	} else {
		idx_graph_search_host(ix, q, k, ef, pp, neighbors);
	}
	// add_graph_results (index.rs:454-483)
	for (auto &nb : neighbors) {
		if (!builder.check_add(nb.first))
			continue;
		auto it = ix->by_elem.find(nb.second);
		if (it == ix->by_elem.end())
			continue; // get_vector/get_docs -> None
		builder.add_graph(nb.first, ix->vd.at(*it->second).docs);
	}
	uint32_t n = 0;
	for (const auto &e : builder.pl) {
		out_kinds[n] = e.vid.kind;
		out_ids[n] = e.vid.id;
		out_dists[n] = e.dist;
		n++;
	}
	*out_n = n;
	return SDBV_OK;
}

// knn_search with cond_filter (index.rs:270-335 + knn_search_with_filter
// mod.rs:484-515 + search_single_with_filter layer.rs:110-149): same flow
// as sdbv_index_knn but candidates expand unconditionally and w is gated
// by add_if_truthy (>=1 truthy doc, not all-pending). NOTE the reference
// seeds add_if_truthy with SEARCH.PT as the entry point's vector
// (layer.rs:125-135) — the entry point enters w only if the QUERY VECTOR
// itself is an indexed vector with a truthy doc; restated as-is.
int sdbv_index_knn_filtered(sdbv_index *ix, const float *q, uint32_t k,
                            uint32_t ef, sdbv_truthy_cb truthy,
                            sdbv_expire_cb expire, void *user,
                            uint8_t *out_kinds, uint64_t *out_ids,
                            double *out_dists, uint32_t *out_n) {
	using namespace hnsw;
	if (!ix || !q || k == 0 || !truthy)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	sdbv_hnsw *h = ix->h;
	vdocs::Builder builder(k);
	vdocs::Filter filter{truthy, expire, user, {}};
	// search_pendings with the filter (index.rs:400-421)
	std::set<uint64_t> all_existing;
	std::map<vdocs::Vid, const std::vector<float> *> non_deleted;
	for (auto &p : ix->pendings) {
		if (p.kind == 0)
			all_existing.insert(p.id);
		vdocs::Vid vid{p.kind, p.id};
		if (p.news.empty())
			non_deleted.erase(vid);
		else
			non_deleted[vid] = &p.news;
	}
	if (!(all_existing.empty() && non_deleted.empty())) {
		double q_norm = h->metric == SDBV_METRIC_COSINE
		                    ? sqrt(host_sumsq_f32(q, h->d))
		                    : 0;
		for (auto &e : non_deleted) {
			if (!filter.truthy(e.first.kind, e.first.id))
				continue;
			const std::vector<float> &vecs = *e.second;
			for (size_t i = 0; i * h->d < vecs.size(); i++) {
				double dd =
				    idx_dist_raw(h, q, q_norm, vecs.data() + i * h->d);
				if (builder.check_add(dd)) {
					vdocs::Vid ev;
					if (builder.add_ret_evicted(dd, e.first, &ev))
						filter.expire(ev.kind, ev.id);
				}
			}
		}
	}
	const std::set<uint64_t> *pp =
	    all_existing.empty() ? nullptr : &all_existing;
	IdxPend pend{&all_existing, ix};
	const IdxPend *ep_pend = all_existing.empty() ? nullptr : &pend;
	// knn_search_with_filter (mod.rs:484-515)
	std::vector<std::pair<double, uint32_t>> neighbors;
	if (h->next_id > 0 && h->enter_point >= 0) {
		bool use_gpu = h->ctx != nullptr;
		if (use_gpu && (h->dirty || !h->finalized)) {
			int rc = sdbv_hnsw_finalize(h, ix->table);
			if (rc)
				return rc;
		}
		double q_norm = h->metric == SDBV_METRIC_COSINE
		                    ? sqrt(host_sumsq_f32(q, h->d))
		                    : 0;
		// search_ep: plain upper-layer descent with pending (mod.rs:520-548)
		uint32_t ep_id = (uint32_t)h->enter_point;
		double ep_dist = dist(h, q, q_norm, ep_id);
		for (size_t l = h->layers.size() - 1; l >= 1; l--) {
			PQ cand;
			cand.push(ep_dist, ep_id);
			std::unordered_set<uint32_t> visited{ep_id};
			PQ w = cand;
			search_layer_host(h, h->layers[l], q, q_norm, cand, visited, w,
			                  1, false, ep_pend);
			double dd;
			uint32_t ii;
			if (w.peek_first(&dd, &ii)) {
				ep_dist = dd;
				ep_id = ii;
			}
		}
		// search_single_with_filter (layer.rs:110-149; the search.pt seed)
		PQ candidates, w;
		candidates.push(ep_dist, ep_id);
		std::vector<bool> visited(h->next_id, false);
		visited[ep_id] = true;
		idx_add_if_truthy(ix, ef, w, q, ep_dist, ep_id, filter, pp);
		if (use_gpu) {
			int rc = idx_search_l0_filter_gpu(ix, q, q_norm, candidates,
			                                  visited, w, ef, filter, pp);
			if (rc)
				return rc;
		} else {
			idx_search_l0_filter_host(ix, q, q_norm, candidates, visited, w,
			                          ef, filter, pp);
		}
		auto v = w.to_vec();
		size_t m = std::min<size_t>(k, v.size());
		for (size_t i = 0; i < m; i++)
			neighbors.push_back({v[i].first, v[i].second});
	}
	// add_graph_results with eviction expiry (index.rs:353-359, :454-483)
	for (auto &nb : neighbors) {
		if (!builder.check_add(nb.first))
			continue;
		auto it = ix->by_elem.find(nb.second);
		if (it == ix->by_elem.end())
			continue;
		for (uint64_t docid : ix->vd.at(*it->second).docs.v) {
			vdocs::Vid ev;
			if (builder.add_ret_evicted(nb.first, vdocs::Vid{0, docid}, &ev))
				filter.expire(ev.kind, ev.id);
		}
	}
	uint32_t n = 0;
	for (const auto &e : builder.pl) {
		out_kinds[n] = e.vid.kind;
		out_ids[n] = e.vid.id;
		out_dists[n] = e.dist;
		n++;
	}
	*out_n = n;
	return SDBV_OK;
}

// ---- KV cold-start loader (He/Hn/Hs/Hv stream -> host graph + index) ----

struct sdbv_kvload {
	sdbv_ctx *ctx;
	uint32_t d;
	uint8_t metric;
	uint32_t m, m0, efc;
	int extend, keep;
	uint64_t seed;
	double ml;
	bool has_state = false;
	kvc::HnswStateKV state;
	std::map<uint64_t, std::vector<float>> elems;          // He
	std::map<std::pair<uint16_t, uint64_t>, std::vector<uint32_t>> nodes; // Hn
	struct HvEnt {
		std::vector<float> vec;
		uint64_t e_id;
		vdocs::Ids64 docs;
	};
	std::vector<HvEnt> hv; // Hv
	std::map<uint64_t, kvc::PendingKV> hp; // Hp by appending id
};

int sdbv_kvload_new(sdbv_ctx *ctx, uint32_t d, uint8_t metric, uint32_t m,
                    uint32_t m0, uint32_t efc, int extend, int keep,
                    uint64_t seed, double ml, sdbv_kvload **out) {
	if (d == 0 || (d % 4) != 0 || metric > SDBV_METRIC_EUCLIDEAN)
		return SDBV_ERR_BAD_ARG;
	auto *L = new sdbv_kvload();
	L->ctx = ctx;
	L->d = d;
	L->metric = metric;
	L->m = m;
	L->m0 = m0;
	L->efc = efc;
	L->extend = extend;
	L->keep = keep;
	L->seed = seed;
	L->ml = ml;
	*out = L;
	return SDBV_OK;
}

void sdbv_kvload_abort(sdbv_kvload *L) { delete L; }

// Feed one (key, value) pair from the index's KV range scan. Unknown `!h?`
// kinds (hd/hi/hp/hh records — host-kept) are skipped, not errors.
int sdbv_kvload_feed(sdbv_kvload *L, const uint8_t *key, uint64_t klen,
                     const uint8_t *val, uint64_t vlen) {
	if (!L || !key)
		return SDBV_ERR_BAD_ARG;
	kvc::ParsedKey pk;
	if (kvc::parse_key(key, klen, &pk) != 0)
		return SDBV_ERR_BAD_ARG;
	const uint8_t *p = pk.rest, *end = pk.end;
	switch (pk.kind) {
	case 'e': { // He: element id (key) -> SerializedVector (value)
		uint64_t e_id;
		if (!kvc::get_be(p, end, &e_id))
			return SDBV_ERR_BAD_ARG;
		std::vector<float> v;
		if (!kvc::dec_vec_f32(val, val + vlen, v) || v.size() != L->d)
			return SDBV_ERR_UNSUPPORTED;
		L->elems[e_id] = std::move(v);
		return SDBV_OK;
	}
	case 'n': { // Hn: (layer, node) -> edge list
		uint16_t layer;
		uint64_t node;
		if (!kvc::get_be(p, end, &layer) || !kvc::get_be(p, end, &node))
			return SDBV_ERR_BAD_ARG;
		std::vector<uint32_t> edges;
		if (!kvc::dec_node(val, val + vlen, edges))
			return SDBV_ERR_BAD_ARG;
		L->nodes[{layer, node}] = std::move(edges);
		return SDBV_OK;
	}
	case 's': { // Hs: graph state
		if (!kvc::dec_state(val, val + vlen, &L->state))
			return SDBV_ERR_UNSUPPORTED;
		L->has_state = true;
		return SDBV_OK;
	}
	case 'v': { // Hv: escaped vector (key) -> ElementDocs (value)
		std::vector<uint8_t> ser;
		if (!kvc::get_escaped(p, end, ser))
			return SDBV_ERR_BAD_ARG;
		sdbv_kvload::HvEnt ent;
		if (!kvc::dec_vec_f32(ser.data(), ser.data() + ser.size(),
		                      ent.vec) ||
		    ent.vec.size() != L->d)
			return SDBV_ERR_UNSUPPORTED;
		if (!kvc::dec_element_docs(val, val + vlen, &ent.e_id, &ent.docs))
			return SDBV_ERR_UNSUPPORTED;
		L->hv.push_back(std::move(ent));
		return SDBV_OK;
	}
	case 'p': { // Hp: appending id (key) -> VectorPendingUpdate (value)
		uint64_t aid;
		if (!kvc::get_be(p, end, &aid))
			return SDBV_ERR_BAD_ARG;
		kvc::PendingKV pk;
		if (!kvc::dec_pending(val, val + vlen, L->d, &pk))
			return SDBV_ERR_UNSUPPORTED;
		L->hp[aid] = std::move(pk);
		return SDBV_OK;
	}
	default:
		return SDBV_OK; // hd/hi/hh etc.: host-kept, skipped
	}
}

// Builds the host graph from the fed He/Hn/Hs pairs (HnswFlavor::new +
// check_state + HnswLayer::load, layer.rs:504-563 — post-Hl format only).
static int kvload_build_graph(sdbv_kvload *L, sdbv_hnsw **out) {
	if (!L->has_state)
		return SDBV_ERR_BAD_ARG; // an existing index always has Hs
	sdbv_hnsw *h = nullptr;
	int rc = sdbv_hnsw_create(L->ctx, L->d, L->metric, L->m, L->m0, L->efc,
	                          L->extend, L->keep, L->seed, L->ml, &h);
	if (rc)
		return rc;
	uint64_t n = L->state.next_element_id;
	// Untrusted Hs fields bound the allocations below (n*d floats, one
	// n-sized edge vector per layer): reject absurd values up front like
	// the 2^32 doc-id guard, instead of letting bad_alloc abort through
	// the extern "C" boundary.
	if (n > (1ull << 32) || L->state.n_upper_layers > 64) {
		sdbv_hnsw_destroy(h);
		return SDBV_ERR_UNSUPPORTED;
	}
	h->next_id = n;
	h->vecs.assign((size_t)n * L->d, 0.0f);
	h->elem_present.assign(n, 0);
	if (L->metric == SDBV_METRIC_COSINE)
		h->norms.assign(n, 0.0);
	for (auto &e : L->elems) {
		if (e.first >= n) {
			sdbv_hnsw_destroy(h);
			return SDBV_ERR_BAD_ARG;
		}
		std::memcpy(h->vecs.data() + e.first * L->d, e.second.data(),
		            (size_t)L->d * 4);
		h->elem_present[e.first] = 1;
		if (L->metric == SDBV_METRIC_COSINE)
			h->norms[e.first] =
			    sqrt(hnsw::host_sumsq_f32(e.second.data(), L->d));
	}
	uint64_t n_layers = 1 + L->state.n_upper_layers;
	h->layers.clear();
	for (uint64_t l = 0; l < n_layers; l++)
		h->layers.push_back(
		    hnsw::Layer{std::vector<std::vector<uint32_t>>(n),
		                l == 0 ? L->m0 : L->m});
	for (auto &l : h->layers)
		l.in_layer.assign(n, 0);
	for (auto &nd : L->nodes) {
		uint16_t layer = nd.first.first;
		uint64_t node = nd.first.second;
		if (layer >= h->layers.size() || node >= n) {
			sdbv_hnsw_destroy(h);
			return SDBV_ERR_BAD_ARG;
		}
		for (uint32_t e : nd.second)
			if (e >= n) {
				sdbv_hnsw_destroy(h);
				return SDBV_ERR_BAD_ARG;
			}
		// Degree above the declared layer cap is ACCEPTED, like the
		// reference's own loader (layer.rs load reads edge lists with no
		// cap check): it arises legitimately from parameter-mismatched
		// dumps and from this repo's threaded builds (keep-back
		// relaxation). Safe since finalize sizes every per-hop scratch
		// from the ACTUAL max degree (the round-1 advisor's overflow is
		// closed by sizing, its alternative remedy); dec_node already
		// bounds a single node at 65535 edges.
		h->layers[layer].edges[node] = nd.second;
		h->layers[layer].in_layer[node] = 1;
	}
	h->enter_point = L->state.has_ep ? (int64_t)L->state.enter_point : -1;
	h->dirty = true;
	*out = h;
	return SDBV_OK;
}

int sdbv_kvload_finish_hnsw(sdbv_kvload *L, sdbv_hnsw **out) {
	if (!L || !out)
		return SDBV_ERR_BAD_ARG;
	int rc = kvload_build_graph(L, out);
	delete L;
	return rc;
}

int sdbv_kvload_finish_index(sdbv_kvload *L, uint64_t table,
                             sdbv_index **out) {
	if (!L || !out)
		return SDBV_ERR_BAD_ARG;
	sdbv_hnsw *h = nullptr;
	int rc = kvload_build_graph(L, &h);
	if (rc) {
		delete L;
		return rc;
	}
	auto *ix = new sdbv_index();
	ix->h = h;
	ix->table = table;
	uint64_t max_doc = 0;
	bool any_doc = false;
	for (auto &ent : L->hv) {
		std::string key((const char *)ent.vec.data(), (size_t)L->d * 4);
		auto r = ix->vd.emplace(std::move(key),
		                        sdbv_index::ED{(uint32_t)ent.e_id, ent.docs});
		if (r.second)
			ix->by_elem[(uint32_t)ent.e_id] = &r.first->first;
		for (uint64_t d : ent.docs.v) {
			any_doc = true;
			if (d > max_doc)
				max_doc = d;
		}
	}
	// HnswDocsState (hd root) stays host-side, but the allocator is
	// reconstructed EXACTLY up to allocation equivalence. Doc ids
	// allocate densely (docs.rs:78-90), so the reference's persisted
	// state is always {available = [0, next) \ bound, next}; min-first
	// draws make any trailing run of `available` foldable into `next`
	// without changing a single future allocation. Hence: seed
	// available with every id up to the highest Hv-referenced one (Hv
	// references include RECYCLED zombies — the dropped-old-removal
	// quirk — which the reference also holds in `available`), and let
	// sdbv_index_bind_doc_key carve out the live (hi/hd-bound) ids.
	ix->next_doc_id = any_doc ? max_doc + 1 : 0;
	if (ix->next_doc_id > (1ull << 32)) { // corrupt input guard: doc ids
		delete ix;                         // are dense, so this is absurd
		return SDBV_ERR_UNSUPPORTED;
	}
	for (uint64_t dd = 0; dd < ix->next_doc_id; dd++)
		ix->available.insert(dd);
	// outstanding Hp pendings, in appending order (the reference drains
	// the Hp range in key order, index.rs:195-205)
	for (auto &e : L->hp) {
		sdbv_index::Pending p;
		p.kind = e.second.kind;
		p.id = e.second.id;
		p.olds = std::move(e.second.olds);
		p.news = std::move(e.second.news);
		ix->pendings.push_back(std::move(p));
	}
	delete L;
	*out = ix;
	return SDBV_OK;
}

// Export the doc-id <-> record-key-handle map (the host's hi/hd state —
// what it persists so a cold start can re-bind). Returns the entry count;
// writes up to `cap` pairs.
uint64_t sdbv_index_doc_keys(sdbv_index *ix, uint64_t *out_docs,
                             uint64_t *out_keys, uint64_t cap) {
	if (!ix)
		return 0;
	std::lock_guard<std::mutex> lk(ix->mu);
	uint64_t i = 0;
	for (auto &e : ix->doc2key) {
		if (i < cap) {
			out_docs[i] = e.first;
			out_keys[i] = e.second;
		}
		i++;
	}
	return (uint64_t)ix->doc2key.size();
}

// Re-binds one record-key handle to a doc id (the host's hi/hd entries)
// after a cold-start load.
int sdbv_index_bind_doc_key(sdbv_index *ix, uint64_t doc_id,
                            uint64_t record_key) {
	if (!ix)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	ix->key2doc[record_key] = doc_id;
	ix->doc2key[doc_id] = record_key;
	// keep the reconstructed allocator consistent: a bound id is live
	ix->available.erase(doc_id);
	if (doc_id >= ix->next_doc_id) {
		if (doc_id - ix->next_doc_id > (1ull << 32))
			return SDBV_ERR_BAD_ARG; // dense ids: absurd gap = corrupt
		for (uint64_t dd = ix->next_doc_id; dd < doc_id; dd++)
			ix->available.insert(dd);
		ix->next_doc_id = doc_id + 1;
	}
	return SDBV_OK;
}

// ---- KV dump (round-trip + migration tooling) ----

typedef int (*sdbv_kv_write_cb)(void *user, const uint8_t *key, uint64_t klen,
                                const uint8_t *val, uint64_t vlen);

int sdbv_hnsw_dump_kv(sdbv_hnsw *h, uint32_t ns, uint32_t db, const char *tb,
                      uint32_t ix_id, sdbv_kv_write_cb write, void *user) {
	if (!h || !tb || !write)
		return SDBV_ERR_BAD_ARG;
	std::vector<uint8_t> k, v;
	// Hs
	kvc::HnswStateKV st;
	st.has_ep = h->enter_point >= 0;
	st.enter_point = st.has_ep ? (uint64_t)h->enter_point : 0;
	st.next_element_id = h->next_id;
	st.n_upper_layers = h->layers.size() - 1;
	k.clear();
	v.clear();
	kvc::key_hs(k, ns, db, tb, ix_id);
	kvc::enc_state(v, st);
	if (write(user, k.data(), k.size(), v.data(), v.size()))
		return SDBV_ERR_BAD_ARG;
	// He per present element
	for (uint64_t e = 0; e < h->next_id; e++) {
		if (!h->elem_present[e])
			continue;
		k.clear();
		v.clear();
		kvc::key_he(k, ns, db, tb, ix_id, e);
		kvc::enc_vec_f32(v, h->vecs.data() + e * h->d, h->d);
		if (write(user, k.data(), k.size(), v.data(), v.size()))
			return SDBV_ERR_BAD_ARG;
	}
	// Hn per layer member
	for (size_t l = 0; l < h->layers.size(); l++) {
		const hnsw::Layer &layer = h->layers[l];
		for (uint64_t node = 0; node < layer.edges.size(); node++) {
			if (!layer.has((uint32_t)node))
				continue;
			k.clear();
			v.clear();
			kvc::key_hn(k, ns, db, tb, ix_id, (uint16_t)l, node);
			kvc::enc_node(v, layer.edges[node]);
			if (write(user, k.data(), k.size(), v.data(), v.size()))
				return SDBV_ERR_BAD_ARG;
		}
	}
	return SDBV_OK;
}

int sdbv_index_dump_kv(sdbv_index *ix, uint32_t ns, uint32_t db,
                       const char *tb, uint32_t ix_id, sdbv_kv_write_cb write,
                       void *user) {
	if (!ix)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	int rc = sdbv_hnsw_dump_kv(ix->h, ns, db, tb, ix_id, write, user);
	if (rc)
		return rc;
	std::vector<uint8_t> k, v;
	for (auto &e : ix->vd) {
		k.clear();
		v.clear();
		kvc::key_hv(k, ns, db, tb, ix_id, (const float *)e.first.data(),
		            ix->h->d);
		if (!kvc::enc_element_docs(v, e.second.e_id, e.second.docs))
			return SDBV_ERR_UNSUPPORTED; // Ids64 in Bits (roaring) mode
		if (write(user, k.data(), k.size(), v.data(), v.size()))
			return SDBV_ERR_BAD_ARG;
	}
	// outstanding pendings as Hp pairs (RecordKey handles dump as
	// RecordIdKey::Number — see INTEGRATION.md "record-key handles")
	uint64_t aid = 0;
	for (auto &p : ix->pendings) {
		kvc::PendingKV pk;
		pk.kind = p.kind;
		pk.id = p.id;
		pk.olds = p.olds;
		pk.news = p.news;
		k.clear();
		v.clear();
		kvc::key_hp(k, ns, db, tb, ix_id, aid++);
		kvc::enc_pending(v, ix->h->d, pk);
		if (write(user, k.data(), k.size(), v.data(), v.size()))
			return SDBV_ERR_BAD_ARG;
	}
	return SDBV_OK;
}

// check_hnsw_properties (mod.rs:561-570 + the reference index tests'
// element count): present elements == expected == Hv entries, layer edge
// invariants (counts, no self-edges, in-range targets).
int sdbv_index_check_props(sdbv_index *ix, uint64_t expected_count) {
	if (!ix)
		return SDBV_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lk(ix->mu);
	sdbv_hnsw *h = ix->h;
	uint64_t present = 0;
	for (uint8_t p : h->elem_present)
		present += p;
	if (present != expected_count)
		return -10;
	if (present != ix->vd.size())
		return -11;
	for (size_t li = 0; li < h->layers.size(); li++) {
		auto &layer = h->layers[li];
		for (size_t id = 0; id < layer.edges.size(); id++) {
			if (!layer.has((uint32_t)id)) {
				if (!layer.edges[id].empty()) {
					if (getenv("SDBV_DEBUG"))
						fprintf(stderr,
						        "check_props: layer %zu node %zu not "
						        "member, %zu edges (present=%d)\n",
						        li, id, layer.edges[id].size(),
						        id < h->elem_present.size()
						            ? (int)h->elem_present[id]
						            : -1);
					return -12;
				}
				continue;
			}
			if (layer.edges[id].size() > layer.m_max)
				return -13;
			// layer.rs check_props: every graph node is a LIVE element
			// (edge targets may dangle, nodes may not)
			if (id >= h->elem_present.size() || !h->elem_present[id])
				return -15;
			for (uint32_t e : layer.edges[id])
				if (e == id || e >= h->next_id)
					return -14;
		}
	}
	return 0;
}

} // extern "C"
