// What top-K lists are made of (mamdr_id_counts, mamdr_list_similarity; include/mamdr_hip.h).  No reference counterpart: the
// reference's pipeline ends at loss and AUC and never looks at a list.
//
// k_id_counts     counts[i] = #{j : ids[j] == i (and label[j] != 0 where a label column is given)}: a grid-stride loop of
//                 integer atomics.  An id outside [0, n_bins) counts nowhere.  Integer additions commute: the same bits
//                 whatever order the workgroups run in.
//
// k_list_sim<W>   one workgroup of W waves per list: W = 1 for k <= 32 (one 32 x 32 Gram tile), W = 4 beyond (up to 128 rows,
//                 the upper-triangle tiles (ti <= tj) dealt to the waves in the fixed order of LS_TI / LS_TJ: tile t belongs
//                 to wave t mod 4).
//   1. the list's valid entries (0 <= id < n_rows) are compacted in list order: L of them; padding leaves no trace.
//   2. the L rows stream through LDS LS_CHUNK columns at a time with 16-byte loads (rows L .. the next multiple of 32 are
//      zeros).  Per group of 8 columns c .. c + 7, lane l (r = l & 31, h = l >> 5) reads the float4 at [32 ti + r][c + 4 h]
//      (and the same of tile tj) and feeds element j = 0 .. 3 to v_mfma_f32_32x32x2_f32 as A / B: step j multiplies the
//      column pair (c + j, c + 4 + j).  A dot product is therefore ONE fp32 fma chain over the columns in the fixed order
//      c + j, c + 4 + j (c ascending by 8, j = 0 .. 3), whatever tile, wave or variant computes it.
//   3. the squared norms are the diagonal of the diagonal tiles; cos = (g / sqrtf(n_a)) / sqrtf(n_b) with IEEE sqrt and
//      division, exactly 0 when either squared norm is 0.
//   4. every lane adds its tile's cosines (a < b < L) in fp64 in register order, the 64 lanes meet in a fixed xor butterfly
//      (32, 16, 8, 4, 2, 1), and thread 0 adds the live tiles' sums to +0.0 in tile order.
// Every order above depends on the list's own valid entries alone: a list's two results are the same bits from run to run,
// wherever the list sits in the call, whatever its neighbours hold and whichever variant runs it.  No floating-point atomics.
//
// Steps 1 - 3 and the cosine's quotient live in list_gram.h, which k_list_div (diversify_kernels.hip) shares: its cosines are
// these bits.
#include "list_gram.h"

namespace mamdr {
namespace {

constexpr int IDC_THREADS = 256;
constexpr int IDC_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(IDC_THREADS) void k_id_counts(const IdCountArgs a) {
    const int64_t step = (int64_t)gridDim.x * IDC_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * IDC_THREADS + threadIdx.x; j < a.n; j += step) {
        const int64_t id = a.ids[j];
        if (id < 0 || id >= a.n_bins) continue;
        if (a.label && !(a.label[j] != 0.f)) continue;
        atomicAdd(a.counts + id, 1u);
    }
}

__device__ __forceinline__ double ls_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_list_sim(const ListSimArgs a) {
    constexpr int ROWS = LsShape<WAVES>::ROWS, SLOTS = LsShape<WAVES>::SLOTS;
    __shared__ __attribute__((aligned(16))) float tile[ROWS * LS_LD];
    __shared__ int s_row[ROWS];
    __shared__ float s_n2[ROWS];
    __shared__ double s_tsum[LS_TILES];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q = blockIdx.x;

    // 1. the valid entries, in list order
    int slot;
    const int L = ls_compact<WAVES>(a.ids, a.k, a.n_rows, q, s_row, s_cnt, slot);
    if (L < 2) {                                    // (uniform: no pair, nothing to read)
        if (tid == 0) {
            a.sim_sum[q] = 0.0;
            a.pairs[q] = 0;
        }
        return;
    }
    __syncthreads();
    const int n_t = (L + 31) >> 5;                  // live row tiles

    // 2. + 3. the Gram tiles and the squared norms
    LsTiles<WAVES> T;
    ls_gram<WAVES>(a.rows, a.emb_dim, L, s_row, tile, s_n2, T);
    const int r = lane & 31, h = lane >> 5;

    // 4. cosines of the pairs a < b < L, added in fp64
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (!T.live[s]) continue;
        const int col = 32 * T.tj[s] + r;
        const float nb = s_n2[col];
        const float sb = sqrtf(nb);
        double sum = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = 32 * T.ti[s] + ls_acc_row(g, h);
            const float na = s_n2[row];                             // (row < 32 n_t: written, or a zero row's zero)
            const float cosv = ls_cos(T.acc[s][g], na, nb, sb);
            if (row < col && col < L) sum += (double)cosv;
        }
        sum = ls_wave_sum(sum);
        if (lane == 0) s_tsum[w + 4 * s] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int t = 0; t < (WAVES == 1 ? 1 : LS_TILES); ++t)
            if (LS_TJ[t] < n_t) total += s_tsum[t];
        a.sim_sum[q] = total;
        a.pairs[q] = L * (L - 1) / 2;
    }
}

}  // namespace

void launch_id_counts(const IdCountArgs& a, hipStream_t s) {
    int64_t blocks = (a.n + IDC_THREADS - 1) / IDC_THREADS;
    if (blocks > IDC_MAX_BLOCKS) blocks = IDC_MAX_BLOCKS;
    MAMDR_LAUNCH(k_id_counts, dim3((unsigned)blocks), dim3(IDC_THREADS), 0, s, a);
}

void launch_list_sim(const ListSimArgs& a, hipStream_t s) {
    if (a.k <= 32) MAMDR_LAUNCH(k_list_sim<1>, dim3((unsigned)a.n_list), dim3(64), 0, s, a);
    else MAMDR_LAUNCH(k_list_sim<4>, dim3((unsigned)a.n_list), dim3(256), 0, s, a);
}

}  // namespace mamdr
