// The non-personalised and memory-based baselines of the rank-eval protocol (mamdr_item_cooc, mamdr_history_scores,
// mamdr_rank_scores, mamdr_topk_scores; include/mamdr_hip.h): item co-occurrence counts of user histories, ItemKNN scores
// from them, and ranks / top-K lists from ANY dense score matrix under the retrieval family's key.  No reference
// counterpart: the reference never ranks.
//
// A history is a CSR over users (hist_off int64 [n_user + 1], hist_pos int32 [nnz]).  Every reader clamps both ends of a
// user's range into [0, nnz] (an end below its start is an empty range) and skips a position outside [0, m): a broken CSR
// gives wrong numbers, never an access outside the arrays.
//
// k_item_cooc     the sparse form: one workgroup of 4 waves per user, one integer atomic per ORDERED pair of its history
//                 (sum of L^2 adds).  Wave w owns the history entries a = h[w], h[w + 4], ..: the row of C is wave-uniform,
//                 and the lanes walk the history as columns b = h[lane], h[lane + 64], .. -- one wave-instruction's adds
//                 land along ONE row of C, in ascending columns; both loops stride, so a history longer than the workgroup
//                 still produces all L^2 pairs.  The diagonal pair (a, a) is the item's user count.
// k_item_roots    root[a] = sqrtf(float(C[a][a])): m square roots once per call instead of one per (query, entry, column).
// k_hist_scores   one workgroup of 256 lanes per (query, tile of 256 V columns), V = 4 with 16-byte loads where every row
//                 of C and of the scores is 16-byte aligned, V = 1 otherwise.  A lane owns its V output elements for the
//                 whole walk over the history: entry j (wave-uniform) brings row j of C, consecutive lanes reading
//                 consecutive columns, and every element makes ONE fp32 add per entry in history order -- one reduction
//                 order, no cross-lane sum, no atomics.  sim = float(C[c][j]) / (root[c] * root[j] + shrink): a product, a
//                 sum and an IEEE division, separately rounded (the file is compiled without fma contraction and with
//                 correctly rounded division and square root).  Both variants run the same operations per element.
// k_rank_scores   one workgroup per (query, tile of 1,024 candidate positions): four keys per lane in registers (0 for an
//                 excluded position), then per target of the query popcount(ballot(key > target key)), one integer atomic
//                 per wave and target; the live count the same way.  The target's key is the key of the candidate position
//                 that holds its id (binary search in d_cand): no position, rank -1.
// k_topk_scores   one workgroup per query walks the candidates 256 at a time; a tile that holds a key above the running
//                 K-th joins the 256 best so far in LDS and the 512 are sorted (bitonic, descending).  The first k of the
//                 set's sorted keys are a function of the set: no trace of the tiles.
// Keys are rec_key's (rec_device.h) on the score with -0.0 taken as +0.0 -- a bit test, as the tower calls' `logit += 0.f`
// -- so the two selection kernels use no floating-point arithmetic at all.  Integer atomics only.
#include "rec_device.h"

namespace mamdr {
namespace {

constexpr int BASE_THREADS = 256;
constexpr int RANK_ITEMS = 4;                    // candidate positions per lane of k_rank_scores
constexpr int TOPK_TILE = 256;                   // candidates per step of k_topk_scores
static_assert(BASE_MAX_K <= TOPK_TILE, "the running list holds the longest list");

typedef __attribute__((ext_vector_type(4))) unsigned int base_u32x4;
typedef __attribute__((ext_vector_type(4))) float base_f32x4;

// user u's range of hist_pos, both ends inside [0, nnz]
__device__ __forceinline__ void hist_range(const HistArgs& a, int64_t u, int64_t& lo, int64_t& hi) {
    lo = a.hist_off[u];
    hi = a.hist_off[u + 1];
    lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
    hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
}

__global__ __launch_bounds__(BASE_THREADS) void k_item_cooc(const HistArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t lo, hi;
    hist_range(a, blockIdx.x, lo, hi);
    for (int64_t i = lo + w; i < hi; i += BASE_THREADS / 64) {          // (wave-uniform)
        const int row = a.hist_pos[i];
        if (row < 0 || row >= a.m) continue;
        uint32_t* dst = a.cooc + (size_t)row * a.m;
        for (int64_t j = lo + lane; j < hi; j += 64) {
            const int col = a.hist_pos[j];
            if (col >= 0 && col < a.m) atomicAdd(dst + col, 1u);
        }
    }
}

__global__ __launch_bounds__(BASE_THREADS) void k_item_roots(const HistArgs a) {
    const int c = blockIdx.x * BASE_THREADS + threadIdx.x;
    if (c < a.m) a.root[c] = sqrtf((float)a.cooc[(size_t)c * a.m + c]);
}

__device__ __forceinline__ float hist_sim(uint32_t cnt, int c, int j, float rc, float rj, float shrink) {
    if (cnt == 0u || c == j) return 0.f;
    return (float)cnt / (rc * rj + shrink);
}

template <int V>
__global__ __launch_bounds__(BASE_THREADS) void k_hist_scores(const HistArgs a, int tiles) {
    const int q = blockIdx.x / tiles, tile = blockIdx.x - q * tiles;
    const int c0 = (tile * BASE_THREADS + threadIdx.x) * V;            // my first column
    if (c0 >= a.m) return;
    const int u = a.query[q];
    int64_t lo = 0, hi = 0;
    if (u >= 0 && u < a.n_user) hist_range(a, u, lo, hi);
    float rc[V], acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        rc[v] = c0 + v < a.m ? a.root[c0 + v] : 0.f;                    // (V = 4: m is a multiple of 4, every lane is whole)
        acc[v] = 0.f;
    }
    for (int64_t i = lo; i < hi; ++i) {                                 // (block-uniform)
        const int j = a.hist_pos[i];
        if (j < 0 || j >= a.m) continue;
        const float rj = a.root[j];
        const uint32_t* row = a.cooc + (size_t)j * a.m + c0;
        uint32_t cnt[V];
        if constexpr (V == 4) {
            const base_u32x4 x = *reinterpret_cast<const base_u32x4*>(row);
#pragma unroll
            for (int v = 0; v < V; ++v) cnt[v] = x[v];
        } else {
            cnt[0] = row[0];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = acc[v] + hist_sim(cnt[v], c0 + v, j, rc[v], rj, a.shrink);
    }
    float* out = a.scores + (size_t)q * a.m + c0;
    if constexpr (V == 4) {
        *reinterpret_cast<base_f32x4*>(out) = base_f32x4{acc[0], acc[1], acc[2], acc[3]};
    } else {
        out[0] = acc[0];
    }
}

// ---- ranks and top-K lists from a score matrix
__device__ __forceinline__ int score_id(const ScoreRankArgs& a, int p) { return a.cand ? a.cand[p] : p; }

// the key of candidate position p for query q (the position's id given)
__device__ __forceinline__ u64 score_key(const ScoreRankArgs& a, int q, int p, int id) {
    uint32_t b = __float_as_uint(a.scores[(size_t)q * a.row_stride + p]);
    if (b == 0x80000000u) b = 0u;                                       // -0 counts as +0
    return rec_key(__uint_as_float(b), id);
}

// is `id` in query q's exclusion list (ascending ids)
__device__ __forceinline__ bool score_excluded(const ScoreRankArgs& a, int q, int id) {
    if (!a.excl_off) return false;
    const int64_t end = a.excl_off[q + 1];
    int64_t lo = a.excl_off[q], hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.excl_ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < end && a.excl_ids[lo] == id;
}

// the candidate position that holds `id`, or -1
__device__ __forceinline__ int score_position(const ScoreRankArgs& a, int id) {
    if (!a.cand) return id >= 0 && id < a.n_cand ? id : -1;
    int lo = 0, hi = a.n_cand;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cand[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < a.n_cand && a.cand[lo] == id ? lo : -1;
}

__global__ __launch_bounds__(BASE_THREADS) void k_rank_scores(const ScoreRankArgs a, int tiles) {
    const int q = blockIdx.x / tiles, tile = blockIdx.x - q * tiles;
    const int lane = threadIdx.x & 63;
    u64 key[RANK_ITEMS];
    int n_live = 0;
#pragma unroll
    for (int i = 0; i < RANK_ITEMS; ++i) {
        const int64_t p = ((int64_t)tile * RANK_ITEMS + i) * BASE_THREADS + threadIdx.x;
        key[i] = 0ull;
        if (p < a.n_cand) {
            const int id = score_id(a, (int)p);
            if (!score_excluded(a, q, id)) {
                key[i] = score_key(a, q, (int)p, id);
                ++n_live;
            }
        }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) n_live += __shfl_xor(n_live, x, 64);
    if (lane == 0 && n_live) atomicAdd(a.live_out + q, n_live);
    int64_t t0 = a.tgt_off[q], t1 = a.tgt_off[q + 1];
    t0 = t0 < 0 ? 0 : (t0 > a.n_tgt ? a.n_tgt : t0);
    t1 = t1 < t0 ? t0 : (t1 > a.n_tgt ? a.n_tgt : t1);
    for (int64_t t = t0; t < t1; ++t) {                                 // (block-uniform)
        const int id = a.tgt_ids[t];
        const int pt = score_position(a, id);
        if (pt < 0) {                                                   // not among the candidates
            if (tile == 0 && threadIdx.x == 0) {
                a.rank_out[t] = -1;
                if (a.score_out) a.score_out[t] = 0.f;
            }
            continue;
        }
        const u64 tkey = score_key(a, q, pt, id);
        int above = 0;
#pragma unroll
        for (int i = 0; i < RANK_ITEMS; ++i) above += __popcll(__ballot(key[i] > tkey));
        if (lane == 0 && above) atomicAdd(a.rank_out + t, above);
        if (a.score_out && tile == 0 && threadIdx.x == 0) a.score_out[t] = a.scores[(size_t)q * a.row_stride + pt];
    }
}

__global__ __launch_bounds__(BASE_THREADS) void k_topk_scores(const ScoreRankArgs a) {
    __shared__ u64 buf[2 * TOPK_TILE];            // [0, 256): the best so far, sorted descending; [256, 512): the tile
    const int t = threadIdx.x, q = blockIdx.x;
    buf[t] = 0ull;
    __syncthreads();
    for (int64_t base = 0; base < a.n_cand; base += TOPK_TILE) {
        const int64_t p = base + t;
        u64 key = 0ull;
        if (p < a.n_cand) {
            const int id = score_id(a, (int)p);
            if (!score_excluded(a, q, id)) key = score_key(a, q, (int)p, id);
        }
        const u64 kth = buf[a.k - 1];
        if (!__syncthreads_or(key > kth)) continue;
        buf[TOPK_TILE + t] = key;
        __syncthreads();
        for (int k = 2; k <= 2 * TOPK_TILE; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int i = 2 * t - (t & (j - 1)), o = i + j;         // the t-th pair (i, i ^ j) with i < o
                const u64 x = buf[i], y = buf[o];
                if (((i & k) == 0) ? x < y : x > y) {
                    buf[i] = y;
                    buf[o] = x;
                }
                __syncthreads();
            }
        }
    }
    if (t < a.k) {
        const u64 key = buf[t];
        a.ids_out[(size_t)q * a.k + t] = key ? (int32_t)~(uint32_t)key : -1;
        a.topk_out[(size_t)q * a.k + t] = key ? rec_key_logit(key) : 0.f;
    }
}

}  // namespace

void launch_item_cooc(const HistArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_item_cooc, dim3((unsigned)a.n_user), dim3(BASE_THREADS), 0, s, a);
}
void launch_hist_scores(const HistArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_item_roots, dim3((unsigned)((a.m + BASE_THREADS - 1) / BASE_THREADS)), dim3(BASE_THREADS), 0, s, a);
    const int per = BASE_THREADS * (a.vec4 ? 4 : 1), tiles = (a.m + per - 1) / per;
    const dim3 grid((unsigned)((int64_t)a.n_query * tiles));
    if (a.vec4) MAMDR_LAUNCH(k_hist_scores<4>, grid, dim3(BASE_THREADS), 0, s, a, tiles);
    else MAMDR_LAUNCH(k_hist_scores<1>, grid, dim3(BASE_THREADS), 0, s, a, tiles);
}
void launch_rank_scores(const ScoreRankArgs& a, hipStream_t s) {
    const int per = BASE_THREADS * RANK_ITEMS, tiles = (a.n_cand + per - 1) / per;
    MAMDR_LAUNCH(k_rank_scores, dim3((unsigned)((int64_t)a.n_query * tiles)), dim3(BASE_THREADS), 0, s, a, tiles);
}
void launch_topk_scores(const ScoreRankArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_topk_scores, dim3((unsigned)a.n_query), dim3(BASE_THREADS), 0, s, a);
}

}  // namespace mamdr
