// Gram matrices of up to 32 flat fp32 vectors over column ranges, in fp64 (mamdr_gram, include/mamdr_hip.h).  No reference
// counterpart: the reference never measures how much its domains' gradients conflict.
//
// Definition.  out[r][i][j] = sum over k in range r of (double) v_i[k] * (double) v_j[k].  An fp32 x fp32 product has 48
// significant bits and is exact in fp64; only the additions round.
//
// Two launches per batch of up to GRAM_MAX_RANGES ranges, the kernel boundary is the hand-off:
//   k_gram_slab     one workgroup per slab of MAMDR_GRAM_SLAB columns of one range (slabs are cut from the RANGE's first
//                   column, not from the vector's).  The slab streams through LDS GRAM_KC columns at a time as fp32, one
//                   column per thread and fill, with 4-byte loads (a range may start at any element).  Wave w takes the
//                   column quads w, w + 4, ... of every chunk: lane l converts v[l & 15][4 quad + (l >> 4)] (and the same
//                   of row 16 + (l & 15)) to fp64 and feeds it to v_mfma_f64_16x16x4_f64 as BOTH operands -- for a Gram
//                   block the A and the B fragment are the same register.  Three accumulators: rows 0..15 x 0..15,
//                   0..15 x 16..31, 16..31 x 16..31 (one when n_vec <= 16).  The four waves' accumulators meet in LDS and
//                   are added in wave order; the slab's partial goes to the workspace, (i, j) and (j, i) from the SAME
//                   value (the diagonal blocks are read on i <= j only).
//   k_gram_finish   thread e of range r adds element e of the range's partials in ascending slab order.
//
// Determinism.  Which lane multiplies which column, which wave and which MFMA takes it and the order of every addition
// depend on the column's index within its range alone: not on the stride, the buffers' addresses or alignment, the other
// ranges of the call or the grid.  Rows n_vec..31 and the columns behind a short last chunk are zeros in LDS; a zero
// product leaves a sum that started at +0 as it is.  No atomics.  NaN and Inf propagate as IEEE: they reach the results
// of their own vector's row and column only (the padding rows' results are never stored).
//
// f64 MFMA layout (it differs from the f32 maps the other kernels use): A[row = l & 15][k = l >> 4], B[k = l >> 4][col =
// l & 15], one f64 per lane; C/D register g of lane l is (row = (l >> 4) + 4 g, col = l & 15).
#include "mamdr_kernels.h"

namespace mamdr {
namespace {

typedef double gram_f64x4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_THREADS = 256;
constexpr int GRAM_WAVES = GRAM_THREADS / 64;
constexpr int GRAM_KC = GRAM_THREADS;          // columns per LDS chunk: one per thread and fill
constexpr int GRAM_LD = GRAM_KC + 4;           // floats per LDS row: 4 mod 32, so the 16 rows x 4 columns a wave reads spread over the banks
static_assert(GRAM_SLAB % GRAM_KC == 0, "a slab is whole chunks");
static_assert(GRAM_MAX_VEC == 32, "two 16-row MFMA blocks");
static_assert(32 * GRAM_LD * sizeof(float) >= 3 * GRAM_WAVES * 256 * sizeof(double), "the waves' partials reuse the tile");

__device__ __forceinline__ gram_f64x4 gram_mfma(double a, double b, gram_f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the range of the launch that slab `b` belongs to: first[r] <= b < first[r + 1] (empty ranges own no slab)
__device__ __forceinline__ int gram_range_of(const GramArgs& a, int64_t b) {
    int r = 0;
    while (r + 1 < a.n_range && b >= a.first[r + 1]) ++r;
    return r;
}

template <bool HI>
__global__ __launch_bounds__(GRAM_THREADS) void k_gram_slab(const GramArgs a) {
    __shared__ double buf[32 * GRAM_LD / 2];
    float* tile = reinterpret_cast<float*>(buf);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = gram_range_of(a, (int64_t)blockIdx.x);
    const int64_t k0 = ((int64_t)blockIdx.x - a.first[r]) * GRAM_SLAB;        // within the range
    const int64_t left = a.count[r] - k0;
    const int cnt = (int)(left < GRAM_SLAB ? left : GRAM_SLAB);               // columns of this slab (>= 1)
    const float* base = a.vecs + a.off[r] + k0;
    constexpr int ROWS = HI ? 32 : 16;
    const int row = lane & 15, q = lane >> 4;
    gram_f64x4 acc_ll = {0.0, 0.0, 0.0, 0.0}, acc_lh = {0.0, 0.0, 0.0, 0.0}, acc_hh = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < cnt; c0 += GRAM_KC) {
        const bool in = c0 + tid < cnt;
        __syncthreads();                                // (the previous chunk has been read)
#pragma unroll
        for (int v0 = 0; v0 < ROWS; v0 += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = (in && v0 + u < a.n_vec) ? base[(int64_t)(v0 + u) * a.stride + c0 + tid] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) tile[(v0 + u) * GRAM_LD + tid] = t[u];
        }
        __syncthreads();
        const int quads = (min(cnt - c0, GRAM_KC) + 3) >> 2;      // (quads behind the slab's end hold zeros only)
        for (int qd = w; qd < quads; qd += GRAM_WAVES) {
            const double lo = (double)tile[row * GRAM_LD + 4 * qd + q];
            acc_ll = gram_mfma(lo, lo, acc_ll);
            if (HI) {
                const double hi = (double)tile[(row + 16) * GRAM_LD + 4 * qd + q];
                acc_lh = gram_mfma(lo, hi, acc_lh);
                acc_hh = gram_mfma(hi, hi, acc_hh);
            }
        }
    }
    __syncthreads();
    double* red = buf;                                  // [block][wave][register g * 64 + lane]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        red[(0 * GRAM_WAVES + w) * 256 + g * 64 + lane] = acc_ll[g];
        if (HI) {
            red[(1 * GRAM_WAVES + w) * 256 + g * 64 + lane] = acc_lh[g];
            red[(2 * GRAM_WAVES + w) * 256 + g * 64 + lane] = acc_hh[g];
        }
    }
    __syncthreads();
    // thread tid owns C/D element (register g = tid >> 6, lane l = tid & 63) of every block
    const int i = (lane >> 4) + 4 * w, j = lane & 15, n = a.n_vec;
    double* P = a.work + (a.work_first + (int64_t)blockIdx.x) * (n * n);
    double s[3];
#pragma unroll
    for (int b = 0; b < (HI ? 3 : 1); ++b) {
        s[b] = red[(b * GRAM_WAVES + 0) * 256 + tid];
#pragma unroll
        for (int ww = 1; ww < GRAM_WAVES; ++ww) s[b] += red[(b * GRAM_WAVES + ww) * 256 + tid];
    }
    if (i <= j && j < n) {
        P[i * n + j] = s[0];
        P[j * n + i] = s[0];
    }
    if (HI) {
        if (i < n && j + 16 < n) {
            P[i * n + j + 16] = s[1];
            P[(j + 16) * n + i] = s[1];
        }
        if (i <= j && j + 16 < n) {
            P[(i + 16) * n + j + 16] = s[2];
            P[(j + 16) * n + i + 16] = s[2];
        }
    }
}

__global__ __launch_bounds__(64) void k_gram_finish(const GramArgs a) {
    const int r = blockIdx.x, dd = a.n_vec * a.n_vec;
    const int e = blockIdx.y * 64 + threadIdx.x;
    if (e >= dd) return;
    const int64_t n_slab = a.first[r + 1] - a.first[r];
    const double* P = a.work + (a.work_first + a.first[r]) * dd + e;
    double s = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < n_slab; ++t) s += P[t * dd];
    a.out[(a.out_first + r) * dd + e] = s;
}

}  // namespace

void launch_gram(const GramArgs& a, hipStream_t s) {
    const int64_t slabs = a.first[a.n_range];
    if (slabs > 0) {
        if (a.n_vec > 16) MAMDR_LAUNCH(k_gram_slab<true>, dim3((unsigned)slabs), dim3(GRAM_THREADS), 0, s, a);
        else MAMDR_LAUNCH(k_gram_slab<false>, dim3((unsigned)slabs), dim3(GRAM_THREADS), 0, s, a);
    }
    MAMDR_LAUNCH(k_gram_finish, dim3((unsigned)a.n_range, (unsigned)((a.n_vec * a.n_vec + 63) / 64)), dim3(64), 0, s, a);
}

}  // namespace mamdr
