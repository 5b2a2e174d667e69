// Generic-layer engine, device side 1 / 5: the dense contractions (64 x 64 and 32 x 32 tiles, single and grouped).
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
#pragma once
#include "mamdr_kernels.h"

namespace {
using namespace mamdr;

constexpr int GT = 64;      // output tile (rows and columns)
constexpr int GK = 16;      // reduction depth per staged tile
constexpr int GLD = 68;     // LDS row stride (floats): the two half-waves of an operand read hit disjoint banks

// ------------------------------------------------------------------ dense contractions
// MODE 0:  C[M x N] = A[M x K] . B[K x N]        + bias, relu, dropout           (layer forward)
// MODE 1:  C[M x N] = A[M x K] . B[N x K]^T      x the gate of gate_y, += C        (d input = dz . W^T)
// MODE 2:  C[M x N] = A[K x M]^T . B[K x N]                                        (dW = in^T . dz, K = batch rows)
// M, N multiples of 64, K a multiple of 16 (MODE 2: M may end inside its last tile, see m_rows).  64x64 tile per workgroup, 4 waves own its 32x32 quadrants
// (`32x32x2`, A / B fragments read from LDS as one float per lane: [k][m] images, conflict-free).
struct GemmArgs {
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    int K;
    const float* bias; int relu;
    uint32_t drop_key, drop_thresh; float keep_scale; int n_cols; int use_dropout;
    const float* gate_y; int gate_ld; float gate_scale; int accumulate;
    // forward only: + sum_{j < n_xe} xe[row][j] * we[j][col] before the bias (PNN: the inner products feed the last three
    // rows of the first kernel, whose 384 + 3 rows are no multiple of the tile depth)
    const float* xe; int xe_ld; const float* we; int n_xe;
    // MODE 2 only: blockIdx.z owns K rows [z K, (z + 1) K) of A and B and writes its partial product at C + z zstride
    size_t zstride;
    // MODE 2 only: rows of C that exist (0: every tile is whole).  A first layer on 3 E input columns has M = 96 at E = 32:
    // the last tile reads 64 columns of A (its neighbours in the workspace, whatever they hold -- row m of C depends on
    // column m of A alone) and stores the rows below m_rows only
    int m_rows;
};
constexpr int MAX_GROUP = 32;
struct GroupTab {
    int n, tiles_y;
    int64_t a_off[MAX_GROUP], b_off[MAX_GROUP], c_off[MAX_GROUP];      // floats added to A / B / C
    int64_t bias_off[MAX_GROUP];                                       // ... to bias (MODE 0) or to the bias gradient (finish)
    int64_t gate_off[MAX_GROUP];                                       // ... to gate_y (MODE 1)
    uint32_t drop_key[MAX_GROUP];
};
template <int MODE>
__device__ __forceinline__ void gemm_tile(const GemmArgs& a, const int bx, const int by, const int bz) {
    __shared__ __attribute__((aligned(16))) float As[2][GK * GLD];
    __shared__ __attribute__((aligned(16))) float Bs[2][GK * GLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = by * GT, n0 = bx * GT;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    constexpr bool A_KC = MODE != 2;        // A's reduction index is the contiguous one in memory
    constexpr bool B_KC = MODE == 1;
    const int r4 = tid >> 2, k4 = (tid & 3) * 4;        // k-contiguous operand: row r4 of the tile, 4 k's
    const int kr = tid >> 4, c4 = (tid & 15) * 4;       // otherwise: k row kr, 4 columns
    f32x4 ra, rb;
    const float *A = a.A, *B = a.B;
    float* C = a.C;
    if (MODE == 2) {
        A += (size_t)bz * a.K * a.lda;
        B += (size_t)bz * a.K * a.ldb;
        C += (size_t)bz * a.zstride;
    }
    const int nkt = a.K / GK;
    auto gload = [&](int kt) {
        const int k0 = kt * GK;
        ra = A_KC ? *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + r4) * a.lda + k0 + k4)
                  : *reinterpret_cast<const f32x4*>(A + (size_t)(k0 + kr) * a.lda + m0 + c4);
        rb = B_KC ? *reinterpret_cast<const f32x4*>(B + (size_t)(n0 + r4) * a.ldb + k0 + k4)
                  : *reinterpret_cast<const f32x4*>(B + (size_t)(k0 + kr) * a.ldb + n0 + c4);
    };
    auto lstore = [&](int buf) {
        if (A_KC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) As[buf][(k4 + j) * GLD + r4] = ra[j];
        } else {
            *reinterpret_cast<f32x4*>(&As[buf][kr * GLD + c4]) = ra;
        }
        if (B_KC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) Bs[buf][(k4 + j) * GLD + r4] = rb[j];
        } else {
            *reinterpret_cast<f32x4*>(&Bs[buf][kr * GLD + c4]) = rb;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    gload(0);
    lstore(0);
    __syncthreads();
    const int kk = lane >> 5, c = lane & 31;
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nkt) gload(kt + 1);
        const float* ap = &As[buf][kk * GLD + wm + c];
        const float* bp = &Bs[buf][kk * GLD + wn + c];
#pragma unroll
        for (int i = 0; i < GK / 2; ++i) acc = MAMDR_MFMA32(ap[2 * i * GLD], bp[2 * i * GLD], acc);
        if (kt + 1 < nkt) lstore(buf ^ 1);
        __syncthreads();
    }
    // D layout of 32x32x2: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wn + c;
    const float bias = (MODE == 0 && a.bias) ? a.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * kk;
        if (MODE == 2 && a.m_rows && row >= a.m_rows) continue;
        float v = acc[r];
        if (MODE == 0) {
            for (int j = 0; j < a.n_xe; ++j) v = fmaf(a.xe[(size_t)row * a.xe_ld + j], a.we[(size_t)j * a.n_cols + col], v);
            v += bias;
            if (a.relu) v = fmaxf(v, 0.f);
            if (a.use_dropout) {
                const uint32_t u = mamdr_dropout_u32(a.drop_key, (uint32_t)row * (uint32_t)a.n_cols + (uint32_t)col);
                v = u >= a.drop_thresh ? v * a.keep_scale : 0.f;
            }
        } else if (MODE == 1) {
            if (a.gate_y) v = a.gate_y[(size_t)row * a.gate_ld + col] > 0.f ? v * a.gate_scale : 0.f;
            if (a.accumulate) v += C[(size_t)row * a.ldc + col];
        }
        C[(size_t)row * a.ldc + col] = v;
    }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_graph_gemm(const GemmArgs a) {
    gemm_tile<MODE>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// ---- the same contraction for a GROUP of problems of one shape in ONE launch: the experts a task mixes share their input
// and their layer shapes (deep_mtl_ctr.py:31-49: num_experts / specific + shared experts, every one DNN(hidden_dim)), so a
// layer of all of them is one grid -- 12 experts x 64 tiles instead of 12 launches of 64 workgroups on 256 CUs.
// MODE 0 / 1: blockIdx.z = the problem; MODE 2: blockIdx.y = problem x row tile (blockIdx.z stays the split of the rows).
// apply_member: member gi's offsets on the shared description (MODE 0: its bias and dropout key, MODE 1: its producer's gate)
template <int MODE>
__device__ __forceinline__ void apply_member(GemmArgs& a, const GroupTab& t, const int gi) {
    a.A += t.a_off[gi];
    a.B += t.b_off[gi];
    a.C += t.c_off[gi];
    if (MODE == 0) {
        a.bias += t.bias_off[gi];
        a.drop_key = t.drop_key[gi];
    }
    if (MODE == 1 && a.gate_y) a.gate_y += t.gate_off[gi];
}
template <int MODE>
__global__ __launch_bounds__(256) void k_graph_gemm_group(GemmArgs a, const GroupTab t) {
    int gi, by = blockIdx.y, bz = blockIdx.z;
    if (MODE == 2) {
        gi = (int)blockIdx.y / t.tiles_y;
        by = (int)blockIdx.y - gi * t.tiles_y;
    } else {
        gi = blockIdx.z;
        bz = 0;
    }
    apply_member<MODE>(a, t, gi);
    gemm_tile<MODE>(a, blockIdx.x, by, bz);
}

// ---- the same contractions (MODE 0 / 1) on 32 x 32 tiles with the reduction index split over the workgroup's four waves.
// A 1,024-row layer of 512 / 256 / 128 / 64 units is 128 / 64 / 32 / 16 tiles of 64 x 64: half to a sixteenth of the 256
// CUs, each walking a serial chain of K / 2 `32x32x2` MFMAs per wave behind one staged 16-deep tile per round trip
// (12.6 us per launch on the Taobao-10 multi-task configs, profiles/r04g_*).  Here a workgroup owns a 32 x 32 tile
// (4 x the workgroups), stages T32_K = 128 reduction indices per round trip (4 + 4 float4 loads in flight per thread, the
// next stage requested before this one's MFMAs) and every wave contracts its own 32 of them into a full-tile accumulator:
// the MFMA chain per wave is K / 8 long.  The four partial tiles meet in LDS in wave order (fixed: bit-stable), and the
// epilogue runs on 4 neighbouring outputs per thread.  K needs no multiple of 128: the tail is staged as zeros.
constexpr int T32 = 32, T32_K = 128, T32_LD = 36;
template <int MODE>
__device__ __forceinline__ void gemm_tile32(const GemmArgs& a, const int bx, const int by) {
    __shared__ __attribute__((aligned(16))) float As[T32_K * T32_LD];
    __shared__ __attribute__((aligned(16))) float Bs[T32_K * T32_LD];
    static_assert(MODE == 0 || MODE == 1, "weight gradients keep the 64 x 64 tiles");
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = by * T32, n0 = bx * T32;
    constexpr bool B_KC = MODE == 1;
    const int r8 = tid >> 3, q8 = tid & 7;          // k-contiguous operand: tile row r8, float4s q8 + 8 j of its 128 k's
    f32x4 ra[4], rb[4];
    const float *A = a.A, *B = a.B;
    const int nkt = (a.K + T32_K - 1) / T32_K;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto gload = [&](int kt) {
        const int k0 = kt * T32_K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * (q8 + 8 * j);
            ra[j] = k < a.K ? *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + r8) * a.lda + k) : zero;
            if (B_KC) {
                rb[j] = k < a.K ? *reinterpret_cast<const f32x4*>(B + (size_t)(n0 + r8) * a.ldb + k) : zero;
            } else {            // B [K x N]: k row r8 + 32 j, float4 q8 of the tile's 32 columns
                const int kr = k0 + r8 + 32 * j;
                rb[j] = kr < a.K ? *reinterpret_cast<const f32x4*>(B + (size_t)kr * a.ldb + n0 + 4 * q8) : zero;
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * (q8 + 8 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) As[(k + i) * T32_LD + r8] = ra[j][i];
            if (B_KC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) Bs[(k + i) * T32_LD + r8] = rb[j][i];
            } else {
                *reinterpret_cast<f32x4*>(&Bs[(r8 + 32 * j) * T32_LD + 4 * q8]) = rb[j];
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int kk = lane >> 5, c = lane & 31;
    gload(0);
    for (int kt = 0; kt < nkt; ++kt) {
        lstore();
        __syncthreads();
        if (kt + 1 < nkt) gload(kt + 1);
        const float* ap = &As[(32 * w + kk) * T32_LD + c];
        const float* bp = &Bs[(32 * w + kk) * T32_LD + c];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = MAMDR_MFMA32(ap[2 * i * T32_LD], bp[2 * i * T32_LD], acc);
        __syncthreads();
    }
    // the waves' partial tiles -> LDS (D layout of 32x32x2: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    float* red = As;            // (the A stage is free after the loop's last barrier)
    static_assert(4 * 32 * 33 <= T32_K * T32_LD, "the partial tiles fit the A stage");
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(w * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk) * 33 + c] = acc[r];
    __syncthreads();
    const int row = m0 + r8, col = n0 + 4 * q8;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float t = red[(0 * 32 + r8) * 33 + 4 * q8 + j];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) t += red[(ww * 32 + r8) * 33 + 4 * q8 + j];
        v[j] = t;
    }
    float* cp = a.C + (size_t)row * a.ldc + col;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = v[j];
        if (MODE == 0) {
            for (int e = 0; e < a.n_xe; ++e) x = fmaf(a.xe[(size_t)row * a.xe_ld + e], a.we[(size_t)e * a.n_cols + col + j], x);
            if (a.bias) x += a.bias[col + j];
            if (a.relu) x = fmaxf(x, 0.f);
            if (a.use_dropout) {
                const uint32_t u = mamdr_dropout_u32(a.drop_key, (uint32_t)row * (uint32_t)a.n_cols + (uint32_t)(col + j));
                x = u >= a.drop_thresh ? x * a.keep_scale : 0.f;
            }
        } else {
            if (a.gate_y) x = a.gate_y[(size_t)row * a.gate_ld + col + j] > 0.f ? x * a.gate_scale : 0.f;
            if (a.accumulate) x += cp[j];
        }
        v[j] = x;
    }
    if ((reinterpret_cast<uintptr_t>(cp) & 15) == 0) {
        *reinterpret_cast<f32x4*>(cp) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) cp[j] = v[j];
    }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_graph_gemm32(const GemmArgs a) {
    gemm_tile32<MODE>(a, blockIdx.x, blockIdx.y);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_graph_gemm32_group(GemmArgs a, const GroupTab t) {
    const int gi = blockIdx.z;
    apply_member<MODE>(a, t, gi);
    gemm_tile32<MODE>(a, blockIdx.x, blockIdx.y);
}

}  // namespace
