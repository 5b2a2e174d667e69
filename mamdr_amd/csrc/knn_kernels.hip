// Exact cosine nearest neighbours of table rows (mamdr_row_neighbours; include/mamdr_hip.h): a query set x candidate set
// cosine matrix on the fp32 matrix cores with the per-query top-K selection fused behind it.  No reference counterpart.
//
// The cosine is list_gram.h's: ls_fma8 fixes the dot product's fma chain (one chain over the columns, whatever tile holds
// the pair), ls_cos the quotient.  A pair's cosine is therefore the bits k_list_sim forms for the two-entry list [q, c].
//
// k_knn_norms     squared norms with the chain's bits: a wave contracts 32 rows with themselves through ls_fma8 and keeps
//                 the diagonal (32 x the flops of an fmaf loop, on N E instead of N^2 E of them: the MFMA diagonal itself,
//                 not an argument about it).  An id outside [0, n_rows) gets 0.
// k_knn_tile      a workgroup of 4 waves owns KNN_QBLOCK = 64 queries (blockIdx.x) and every gridDim.y-th tile of the
//                 pass's candidates (blockIdx.y: the split).
//   LDS           the 64 query rows, gathered once ([64][emb_dim + 4] floats: 16-byte rows, 4 mod 32 banks); one tile of
//                 64 candidate rows, LS_CHUNK columns at a time ([64][LS_LD]); the 64 running lists ([64][128] keys, sorted
//                 descending, 0 = no entry) -- 146 KiB at emb_dim 256.
//   contraction   wave w owns the 32 x 32 tile (queries 32 (w >> 1) .., candidates 32 (w & 1) ..).  The next stage's rows
//                 are loaded into registers before the MFMAs of the current one, so the loads fly under the matrix cores.
//   selection     the cosines become rec_key(cos, id) in registers (0 where the pair is not eligible).  Only a tile that
//                 holds a key above some query's running K-th (__syncthreads_or) is folded in: the keys' high words
//                 go to LDS by (query, column) (over the candidate tile: it has been read), and wave w inserts, for queries
//                 w, w + 4, .., each staged key into the sorted list it holds in registers (two entries per lane, one
//                 lane shift per key).  Behind the first tiles a key passes with probability about K / (candidates seen).
//                 Integers only from the key on; no atomics at all.
//   passes        the lists live in the workspace between the passes of a call and between this kernel and the merge.
// k_knn_merge     one workgroup per query: the splits' lists through k_rec_merge's 256-key bitonic sort, then the first k
//                 entries as (id, raw cosine); id -1 / sim 0 behind a short list.
//
// Determinism: the first k entries of a list after any number of tiles are the k largest keys of the set it has seen -- a
// function of the set (what stands behind them are keys of that set too, which passed an earlier K-th: they can only lose
// in the merge).  Keys are distinct (distinct ids), so neither the order of the tiles, of d_cand, of the splits nor of the
// passes, nor where a query stands in its block, leaves a trace in the outputs.
#include "list_gram.h"
#include "rec_device.h"

namespace mamdr {
namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_NORM_WAVES = 4;      // waves of a k_knn_norms workgroup: 32 rows each
static_assert(KNN_QBLOCK == 64 && KNN_TILE == 64, "2 x 2 MFMA tiles of 32 x 32, one per wave");
static_assert(KNN_MAX_K == 128, "two list entries per lane");
static_assert(KNN_QBLOCK * KNN_TILE * sizeof(uint32_t) <= KNN_TILE * LS_LD * sizeof(float), "the staged keys fit the tile");

// the row id of entry p of an id list (null: entry p is row p), or -1 when it lies outside [0, n_rows)
__device__ __forceinline__ int knn_row(const int32_t* ids, int64_t p, int64_t n_rows) {
    const int64_t id = ids ? (int64_t)ids[p] : p;
    return id >= 0 && id < n_rows ? (int)id : -1;
}

// out[p] = the squared norm of row ids[first + p] (p < n): the diagonal of the rows' own Gram tile
__global__ __launch_bounds__(KNN_NORM_WAVES * 64) void k_knn_norms(const float* rows, int64_t n_rows, int emb_dim,
                                                                     const int32_t* ids, int64_t first, int n, float* out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t p = ((int64_t)blockIdx.x * KNN_NORM_WAVES + w) * 32 + r;
    const int row = p < n ? knn_row(ids, first + p, n_rows) : -1;
    const float* src = rows + (int64_t)(row < 0 ? 0 : row) * emb_dim + 4 * h;
    ls_f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    for (int c = 0; c < emb_dim; c += 8) {
        ls_f32x4 x = ls_f32x4{0.f, 0.f, 0.f, 0.f};
        if (row >= 0) x = *reinterpret_cast<const ls_f32x4*>(src + c);
        ls_fma8(x, x, acc);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g)
        if (ls_acc_row(g, h) == r && p < n) out[p] = acc[g];
}

// one stage of the walk: LS_CHUNK (or emb_dim = 32) columns of one candidate tile, four float4 per thread
struct KnnStage {
    ls_f32x4 v[4];
};
__device__ __forceinline__ void knn_load(const KnnArgs& a, int tile, int c0, int sh4, KnnStage& st) {
    const int tid = threadIdx.x, cw4 = 1 << sh4, items = KNN_TILE << sh4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = u * KNN_THREADS + tid;
        const int row = i >> sh4, c4 = i & (cw4 - 1);
        const int64_t pos = (int64_t)tile * KNN_TILE + row;
        st.v[u] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < items && pos < a.n_chunk) {
            const int id = knn_row(a.cand, a.c_base + pos, a.n_rows);
            if (id >= 0) st.v[u] = *reinterpret_cast<const ls_f32x4*>(a.rows + (int64_t)id * a.emb_dim + c0 + 4 * c4);
        }
    }
}
__device__ __forceinline__ void knn_store(float* ctile, int sh4, const KnnStage& st) {
    const int tid = threadIdx.x, cw4 = 1 << sh4, items = KNN_TILE << sh4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = u * KNN_THREADS + tid;
        const int row = i >> sh4, c4 = i & (cw4 - 1);
        if (i < items) *reinterpret_cast<ls_f32x4*>(ctile + row * LS_LD + 4 * c4) = st.v[u];
    }
}

__device__ __forceinline__ u64 knn_shfl(u64 v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 knn_shfl_up1(u64 v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1), hi = __shfl_up((uint32_t)(v >> 32), 1);
    return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(KNN_THREADS) void k_knn_tile(const KnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
    __shared__ u64 s_thr[KNN_QBLOCK];              // the query's running K-th key
    __shared__ float s_nq[KNN_QBLOCK];
    __shared__ int s_qid[KNN_QBLOCK];              // the query's row id, -1: not a query
    __shared__ int s_cid[KNN_TILE];                // the tile's candidate ids
    const int E = a.emb_dim, QLD = E + 4;
    float* qrows = reinterpret_cast<float*>(knn_smem);                       // [64][QLD]
    float* ctile = qrows + KNN_QBLOCK * QLD;                                 // [64][LS_LD]
    uint32_t* pend = reinterpret_cast<uint32_t*>(ctile);                     // [64][64] staged keys' high words, over the tile
    u64* lists = reinterpret_cast<u64*>(ctile + KNN_TILE * LS_LD);           // [64][128]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qi = w >> 1, cj = w & 1;
    const int64_t q0 = (int64_t)blockIdx.x * KNN_QBLOCK;
    u64* best = a.best + ((q0 * a.splits + blockIdx.y) * KNN_MAX_K);         // list of query j: best[j * splits * 128 ..]
    const size_t best_ld = (size_t)a.splits * KNN_MAX_K;

    // the queries: ids, squared norms, rows, running lists
    if (tid < KNN_QBLOCK) {
        const int64_t qp = q0 + tid;
        const int id = qp < a.n_query ? knn_row(a.query, qp, a.n_rows) : -1;
        s_qid[tid] = id;
        s_nq[tid] = id >= 0 ? a.qn2[qp] : 0.f;
    }
    __syncthreads();
    {
        const int e4 = E >> 2;
        for (int i = tid; i < KNN_QBLOCK * e4; i += KNN_THREADS) {
            const int row = i / e4, c4 = i - row * e4;
            const int id = s_qid[row];
            ls_f32x4 v = ls_f32x4{0.f, 0.f, 0.f, 0.f};
            if (id >= 0) v = *reinterpret_cast<const ls_f32x4*>(a.rows + (int64_t)id * E + 4 * c4);
            *reinterpret_cast<ls_f32x4*>(qrows + row * QLD + 4 * c4) = v;
        }
        for (int i = tid; i < KNN_QBLOCK * KNN_MAX_K; i += KNN_THREADS) {
            const int row = i >> 7, j = i & (KNN_MAX_K - 1);
            lists[i] = a.first_chunk ? 0ull : best[row * best_ld + j];
        }
    }
    __syncthreads();
    if (tid < KNN_QBLOCK) s_thr[tid] = lists[tid * KNN_MAX_K + a.k - 1];
    // (published by the first stage's barriers)

    // the walk: this split's tiles, a chunk of columns per stage
    const int cw = E < LS_CHUNK ? E : LS_CHUNK, n_cc = E / cw, sh4 = cw == 32 ? 3 : 4;
    const int tiles = (a.n_chunk + KNN_TILE - 1) / KNN_TILE;
    const int my_tiles = (int)blockIdx.y < tiles ? (tiles - 1 - (int)blockIdx.y) / a.splits + 1 : 0;
    const int stages = my_tiles * n_cc;
    ls_f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    KnnStage st;
    if (stages) knn_load(a, blockIdx.y, 0, sh4, st);
    int ti = 0, cc = 0;                                    // the stage's tile (of mine) and chunk of columns
    for (int s = 0; s < stages; ++s) {
        const int tile = blockIdx.y + ti * a.splits;
        __syncthreads();                                   // the tile's last readers are done
        knn_store(ctile, sh4, st);
        __syncthreads();
        if (s + 1 < stages) {
            const bool wrap = cc + 1 == n_cc;
            knn_load(a, wrap ? tile + a.splits : tile, wrap ? 0 : (cc + 1) * cw, sh4, st);
        }
        const float* xq = qrows + (32 * qi + r) * QLD + cc * cw + 4 * h;
        const float* yc = ctile + (32 * cj + r) * LS_LD + 4 * h;
        for (int c = 0; c < cw; c += 8)
            ls_fma8(*reinterpret_cast<const ls_f32x4*>(xq + c), *reinterpret_cast<const ls_f32x4*>(yc + c), acc);
        if (++cc < n_cc) continue;
        cc = 0;
        ++ti;

        // the tile's keys
        const int64_t pos = (int64_t)tile * KNN_TILE + 32 * cj + r;
        const int cid = pos < a.n_chunk ? knn_row(a.cand, a.c_base + pos, a.n_rows) : -1;
        const float nb = cid >= 0 ? a.cn2[pos] : 0.f;
        const float sb = sqrtf(nb);
        uint32_t hi[16];
        bool any = false;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = 32 * qi + ls_acc_row(g, h);
            const int qid = s_qid[row];
            const float cosv = ls_cos(acc[g], s_nq[row], nb, sb);
            const bool ok = cid >= 0 && qid >= 0 && !(a.exclude_self && cid == qid);
            const u64 key = ok ? rec_key(cosv, cid) : 0ull;
            const bool pass = key > s_thr[row];
            hi[g] = pass ? (uint32_t)(key >> 32) : 0u;     // (a key's high word is at least 1)
            any |= pass;
            acc[g] = 0.f;
        }
        if (!__syncthreads_or(any)) continue;              // (and every wave has read the tile)

        // fold the tile in
        if (qi == 0 && h == 0) s_cid[32 * cj + r] = cid;
#pragma unroll
        for (int g = 0; g < 16; ++g) pend[(32 * qi + ls_acc_row(g, h)) * KNN_TILE + 32 * cj + r] = hi[g];
        __syncthreads();
        for (int q = w; q < KNN_QBLOCK; q += 4) {
            const uint32_t khi = pend[q * KNN_TILE + lane];
            unsigned long long mask = __ballot(khi != 0u);
            if (!mask) continue;                           // (wave-uniform)
            const u64 key = ((u64)khi << 32) | (u64)(~(uint32_t)s_cid[lane]);
            u64 a0 = lists[q * KNN_MAX_K + 2 * lane], a1 = lists[q * KNN_MAX_K + 2 * lane + 1];   // entries 2 l, 2 l + 1
            while (mask) {
                const int b = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u64 x = knn_shfl(key, b);
                u64 prev = knn_shfl_up1(a1);               // entry 2 l - 1
                if (lane == 0) prev = ~0ull;
                const u64 n0 = a0 > x ? a0 : (prev > x ? x : prev);
                const u64 n1 = a1 > x ? a1 : (a0 > x ? x : a0);
                a0 = n0;
                a1 = n1;
            }
            lists[q * KNN_MAX_K + 2 * lane] = a0;
            lists[q * KNN_MAX_K + 2 * lane + 1] = a1;
            if (lane == ((a.k - 1) >> 1)) s_thr[q] = ((a.k - 1) & 1) ? a1 : a0;
        }
        // (the next stage's first barrier frees the staged keys and publishes the lists' K-th keys)
    }
    __syncthreads();
    for (int i = tid; i < KNN_QBLOCK * KNN_MAX_K; i += KNN_THREADS) {
        const int row = i >> 7, j = i & (KNN_MAX_K - 1);
        best[row * best_ld + j] = lists[i];
    }
}

// one workgroup per query: its splits' lists -> the first k of their union, as (id, cosine)
__global__ __launch_bounds__(KNN_THREADS) void k_knn_merge(const KnnArgs a) {
    __shared__ u64 buf[2 * KNN_MAX_K];
    const int t = threadIdx.x, q = blockIdx.x;
    const u64* list = a.best + (size_t)q * a.splits * KNN_MAX_K;
    buf[t] = t < KNN_MAX_K ? list[t] : 0ull;
    __syncthreads();
    for (int s = 1; s < a.splits; ++s) {
        const u64 key = t < KNN_MAX_K ? list[(size_t)s * KNN_MAX_K + t] : 0ull;
        const u64 kth = buf[a.k - 1];
        if (!__syncthreads_or(key > kth)) continue;
        if (t < KNN_MAX_K) buf[KNN_MAX_K + t] = key;
        __syncthreads();
        for (int k = 2; k <= 2 * KNN_MAX_K; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int o = t ^ j;
                if (o > t) {
                    const u64 x = buf[t], y = buf[o];
                    if (((t & k) == 0) ? x < y : x > y) {
                        buf[t] = y;
                        buf[o] = x;
                    }
                }
                __syncthreads();
            }
        }
    }
    if (t < a.k) {
        const u64 key = buf[t];
        a.ids_out[(size_t)q * a.k + t] = key ? (int32_t)~(uint32_t)key : -1;
        a.sim_out[(size_t)q * a.k + t] = key ? rec_key_logit(key) : 0.f;
    }
}

size_t knn_tile_lds(int emb_dim) {
    return ((size_t)KNN_QBLOCK * (emb_dim + 4) + (size_t)KNN_TILE * LS_LD) * sizeof(float) +
           (size_t)KNN_QBLOCK * KNN_MAX_K * sizeof(u64);
}

}  // namespace

void launch_knn_query_norms(const KnnArgs& a, hipStream_t s) {
    const int per = KNN_NORM_WAVES * 32;
    MAMDR_LAUNCH(k_knn_norms, dim3((a.n_query + per - 1) / per), dim3(KNN_NORM_WAVES * 64), 0, s, a.rows, a.n_rows, a.emb_dim,
                 a.query, (int64_t)0, a.n_query, a.qn2);
}
void launch_knn_cand_norms(const KnnArgs& a, hipStream_t s) {
    const int per = KNN_NORM_WAVES * 32;
    MAMDR_LAUNCH(k_knn_norms, dim3((a.n_chunk + per - 1) / per), dim3(KNN_NORM_WAVES * 64), 0, s, a.rows, a.n_rows, a.emb_dim,
                 a.cand, a.c_base, a.n_chunk, a.cn2);
}
bool launch_knn_tile(const KnnArgs& a, hipStream_t s) {
    static const bool raised = hipFuncSetAttribute(reinterpret_cast<const void*>(k_knn_tile),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_tile_lds(256)) == hipSuccess;
    if (!raised) return false;
    const unsigned blocks = (unsigned)((a.n_query + KNN_QBLOCK - 1) / KNN_QBLOCK);
    MAMDR_LAUNCH(k_knn_tile, dim3(blocks, (unsigned)a.splits), dim3(KNN_THREADS), knn_tile_lds(a.emb_dim), s, a);
    return true;
}
void launch_knn_merge(const KnnArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_knn_merge, dim3((unsigned)a.n_query), dim3(KNN_THREADS), 0, s, a);
}

}  // namespace mamdr
