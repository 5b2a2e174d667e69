// The cosines of a list's item rows, as far as k_list_sim (list_kernels.hip) and k_list_div (diversify_kernels.hip) share
// them: steps 1 - 3 at the head of list_kernels.hip and the cosine's own quotient.  One definition each, so the fp32 cosine
// of a pair is the same bits in both calls, whichever variant and tile computes it.  The contraction's step (ls_fma8) and the
// quotient (ls_cos) are also what knn_kernels.hip forms its query x candidate cosines with: the same bits again.
//
// MFMA maps (32x32x2 f32): A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C/D register g of lane l is
// (row = (g & 3) + 8 (g >> 2) + 4 (l >> 5), col = l & 31).
#pragma once
#include "mamdr_kernels.h"

namespace mamdr {
namespace {

typedef float ls_f32x16 __attribute__((ext_vector_type(16)));
typedef float ls_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LS_CHUNK = 64;               // columns of a row in LDS at a time (32 when emb_dim is 32)
constexpr int LS_LD = LS_CHUNK + 4;        // floats per LDS row: 16-byte rows, 4 mod 64 -> the ds_read_b128 lane groups spread over the banks
constexpr int LS_TILES = 10;               // upper-triangle 32 x 32 tiles of a 128 x 128 Gram
constexpr int LS_SLOTS = 3;                // tiles per wave of the 4-wave variant, at most: t = w, w + 4, w + 8
static_assert(LIST_SIM_MAX_K == 128, "four 32-row tiles");

__constant__ const signed char LS_TI[LS_TILES] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
__constant__ const signed char LS_TJ[LS_TILES] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};

// rows a workgroup of WAVES waves holds, tiles a wave owns
template <int WAVES>
struct LsShape {
    static constexpr int THREADS = WAVES * 64;
    static constexpr int ROWS = WAVES == 1 ? 32 : LIST_SIM_MAX_K;
    static constexpr int SLOTS = WAVES == 1 ? 1 : LS_SLOTS;
};

// a wave's Gram tiles: tile s is rows 32 ti[s] .., columns 32 tj[s] .. (live[s] is wave-uniform)
template <int WAVES>
struct LsTiles {
    int ti[LsShape<WAVES>::SLOTS], tj[LsShape<WAVES>::SLOTS];
    bool live[LsShape<WAVES>::SLOTS];
    ls_f32x16 acc[LsShape<WAVES>::SLOTS];
};

// row of C/D register g of a lane of half h, inside its tile
__device__ __forceinline__ int ls_acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// the contraction's one step: columns c .. c + 7 of a row pair, x / y the float4 at [row][c + 4 h] of the A / B side.  MFMA j
// multiplies the column pair (c + j, c + 4 + j): every dot product of the family (ls_gram here, knn_kernels.hip) is one fp32
// fma chain over the columns in the order c + j, c + 4 + j (c ascending by 8, j = 0 .. 3).
__device__ __forceinline__ void ls_fma8(const ls_f32x4 x, const ls_f32x4 y, ls_f32x16& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], y[j], acc, 0, 0, 0);
}

// 1. the valid entries (0 <= id < n_rows) of list q, compacted in list order (entry t on thread t: waves 0 and 1 hold them
// all) -> L; `slot` is this thread's entry's place among them, or -1.  s_row[0 .. L) is written; the caller's barrier
// publishes it.
template <int WAVES>
__device__ __forceinline__ int ls_compact(const int32_t* ids, int k, int64_t n_rows, int64_t q, int* s_row, int* s_cnt, int& slot) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int id = tid < k ? ids[q * k + tid] : -1;
    const bool ok = tid < k && id >= 0 && (int64_t)id < n_rows;
    const unsigned long long mask = __ballot(ok);
    if (lane == 0 && w < 2) s_cnt[w] = __popcll(mask);
    __syncthreads();
    const int L = s_cnt[0] + (WAVES > 1 ? s_cnt[1] : 0);
    slot = ok ? (w == 1 ? s_cnt[0] : 0) + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
    if (ok) s_row[slot] = id;
    return L;
}

// 2. + 3. the Gram tiles of rows s_row[0 .. L) (L >= 2, published), a chunk of columns at a time through `tile`
// (ROWS x LS_LD floats), and the squared norms s_n2[0 .. 32 ceil(L / 32)) from the diagonal tiles' own diagonal.  Ends
// behind a barrier: s_n2 is published and `tile` is free.
template <int WAVES>
__device__ __forceinline__ void ls_gram(const float* rows, int emb_dim, int L, const int* s_row, float* tile, float* s_n2,
                                        LsTiles<WAVES>& out) {
    LsTiles<WAVES> T;                               // (a local, handed over at the end: the accumulators stay in AGPRs)
    constexpr int THREADS = LsShape<WAVES>::THREADS, SLOTS = LsShape<WAVES>::SLOTS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n_t = (L + 31) >> 5, Lp = n_t * 32;   // live row tiles, rows in LDS

    // this wave's tiles
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int t = w + 4 * s;
        T.live[s] = t < LS_TILES && LS_TJ[t < LS_TILES ? t : 0] < n_t;
        T.ti[s] = T.live[s] ? LS_TI[t] : 0;
        T.tj[s] = T.live[s] ? LS_TJ[t] : 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) T.acc[s][g] = 0.f;
    }

    // 2. the Gram tiles, a chunk of columns at a time
    const int cw = emb_dim < LS_CHUNK ? emb_dim : LS_CHUNK;        // 32 or 64
    const int sh4 = cw == 32 ? 3 : 4, cw4 = 1 << sh4, items = Lp << sh4;      // float4 per row, per chunk
    const int r = lane & 31, h = lane >> 5;
    for (int c0 = 0; c0 < emb_dim; c0 += cw) {
        if (c0) __syncthreads();                                   // (the previous chunk has been read)
        for (int base = 0; base < items; base += 4 * THREADS) {
            ls_f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * THREADS + tid;
                const int row = i >> sh4, c4 = i & (cw4 - 1);
                v[u] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
                if (i < items && row < L)
                    v[u] = *reinterpret_cast<const ls_f32x4*>(rows + (int64_t)s_row[row] * emb_dim + c0 + 4 * c4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * THREADS + tid;
                const int row = i >> sh4, c4 = i & (cw4 - 1);
                if (i < items) *reinterpret_cast<ls_f32x4*>(tile + row * LS_LD + 4 * c4) = v[u];
            }
        }
        __syncthreads();
        for (int c = 0; c < cw; c += 8) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if (!T.live[s]) continue;                          // (wave-uniform)
                const ls_f32x4 x = *reinterpret_cast<const ls_f32x4*>(tile + (32 * T.ti[s] + r) * LS_LD + c + 4 * h);
                const ls_f32x4 y = *reinterpret_cast<const ls_f32x4*>(tile + (32 * T.tj[s] + r) * LS_LD + c + 4 * h);
                ls_fma8(x, y, T.acc[s]);
            }
        }
    }

    // 3. the squared norms: the diagonal tiles' own diagonal
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (!T.live[s] || T.ti[s] != T.tj[s]) continue;
#pragma unroll
        for (int g = 0; g < 16; ++g)
            if (ls_acc_row(g, h) == r) s_n2[32 * T.ti[s] + r] = T.acc[s][g];
    }
    __syncthreads();
    out = T;
}

// the cosine of the pair (a earlier, b later): g their dot product, na / nb their squared norms, sb = sqrtf(nb)
__device__ __forceinline__ float ls_cos(float g, float na, float nb, float sb) {
    float cosv = 0.f;
    if (na != 0.f && nb != 0.f) cosv = (g / sqrtf(na)) / sb;
    return cosv;
}

}  // namespace
}  // namespace mamdr
