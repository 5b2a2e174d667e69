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
// MFMA maps (32x32x2 f32): A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C/D register g of lane l is
// (row = (g & 3) + 8 (g >> 2) + 4 (l >> 5), col = l & 31).
#include "mamdr_kernels.h"

namespace mamdr {
namespace {

typedef float ls_f32x16 __attribute__((ext_vector_type(16)));
typedef float ls_f32x4 __attribute__((ext_vector_type(4)));

constexpr int IDC_THREADS = 256;
constexpr int IDC_MAX_BLOCKS = 2048;

constexpr int LS_CHUNK = 64;               // columns of a row in LDS at a time (32 when emb_dim is 32)
constexpr int LS_LD = LS_CHUNK + 4;        // floats per LDS row: 16-byte rows, 4 mod 64 -> the ds_read_b128 lane groups spread over the banks
constexpr int LS_TILES = 10;               // upper-triangle 32 x 32 tiles of a 128 x 128 Gram
constexpr int LS_SLOTS = 3;                // tiles per wave of the 4-wave variant, at most: t = w, w + 4, w + 8
static_assert(LIST_SIM_MAX_K == 128, "four 32-row tiles");

__constant__ const signed char LS_TI[LS_TILES] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3};
__constant__ const signed char LS_TJ[LS_TILES] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};

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
    constexpr int THREADS = WAVES * 64;
    constexpr int ROWS = WAVES == 1 ? 32 : LIST_SIM_MAX_K;
    constexpr int SLOTS = WAVES == 1 ? 1 : LS_SLOTS;
    __shared__ __attribute__((aligned(16))) float tile[ROWS * LS_LD];
    __shared__ int s_row[ROWS];
    __shared__ float s_n2[ROWS];
    __shared__ double s_tsum[LS_TILES];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q = blockIdx.x;

    // 1. the valid entries, in list order (entry t on thread t: waves 0 and 1 hold them all)
    const int id = tid < a.k ? a.ids[q * a.k + tid] : -1;
    const bool ok = tid < a.k && id >= 0 && (int64_t)id < a.n_rows;
    const unsigned long long mask = __ballot(ok);
    if (lane == 0 && w < 2) s_cnt[w] = __popcll(mask);
    __syncthreads();
    const int L = s_cnt[0] + (WAVES > 1 ? s_cnt[1] : 0);
    if (ok) s_row[(w == 1 ? s_cnt[0] : 0) + __popcll(mask & ((1ull << lane) - 1ull))] = id;
    if (L < 2) {                                    // (uniform: no pair, nothing to read)
        if (tid == 0) {
            a.sim_sum[q] = 0.0;
            a.pairs[q] = 0;
        }
        return;
    }
    __syncthreads();
    const int n_t = (L + 31) >> 5, Lp = n_t * 32;   // live row tiles, rows in LDS

    // this wave's tiles
    int ti[SLOTS], tj[SLOTS];
    bool live[SLOTS];
    ls_f32x16 acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int t = w + 4 * s;
        live[s] = t < LS_TILES && LS_TJ[t < LS_TILES ? t : 0] < n_t;
        ti[s] = live[s] ? LS_TI[t] : 0;
        tj[s] = live[s] ? LS_TJ[t] : 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[s][g] = 0.f;
    }

    // 2. the Gram tiles, a chunk of columns at a time
    const int cw = a.emb_dim < LS_CHUNK ? a.emb_dim : LS_CHUNK;    // 32 or 64
    const int sh4 = cw == 32 ? 3 : 4, cw4 = 1 << sh4, items = Lp << sh4;      // float4 per row, per chunk
    const int r = lane & 31, h = lane >> 5;
    for (int c0 = 0; c0 < a.emb_dim; c0 += cw) {
        if (c0) __syncthreads();                                   // (the previous chunk has been read)
        for (int base = 0; base < items; base += 4 * THREADS) {
            ls_f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = base + u * THREADS + tid;
                const int row = i >> sh4, c4 = i & (cw4 - 1);
                v[u] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
                if (i < items && row < L)
                    v[u] = *reinterpret_cast<const ls_f32x4*>(a.rows + (int64_t)s_row[row] * a.emb_dim + c0 + 4 * c4);
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
                if (!live[s]) continue;                            // (wave-uniform)
                const ls_f32x4 x = *reinterpret_cast<const ls_f32x4*>(tile + (32 * ti[s] + r) * LS_LD + c + 4 * h);
                const ls_f32x4 y = *reinterpret_cast<const ls_f32x4*>(tile + (32 * tj[s] + r) * LS_LD + c + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[j], y[j], acc[s], 0, 0, 0);
            }
        }
    }

    // 3. the squared norms: the diagonal tiles' own diagonal
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (!live[s] || ti[s] != tj[s]) continue;
#pragma unroll
        for (int g = 0; g < 16; ++g)
            if ((g & 3) + 8 * (g >> 2) + 4 * h == r) s_n2[32 * ti[s] + r] = acc[s][g];
    }
    __syncthreads();

    // 4. cosines of the pairs a < b < L, added in fp64
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        if (!live[s]) continue;
        const int col = 32 * tj[s] + r;
        const float nb = s_n2[col];
        const float sb = sqrtf(nb);
        double sum = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = 32 * ti[s] + (g & 3) + 8 * (g >> 2) + 4 * h;
            const float na = s_n2[row];                             // (row < Lp: written, or a zero row's zero)
            float cosv = 0.f;
            if (na != 0.f && nb != 0.f) cosv = (acc[s][g] / sqrtf(na)) / sb;
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
