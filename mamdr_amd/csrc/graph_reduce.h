// Generic-layer engine, device side 2 / 5: column sums, split sums, the weight-gradient queue and its ends, the gradient sink
// (store, or step the parameter on the spot), the narrow contractions.  After graph_gemm.h (GemmArgs, GroupTab, gemm_tile<2>).
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
#pragma once
#include "mamdr_kernels.h"

namespace {
using namespace mamdr;

// colsum_body: store(col, sum over the batch rows of dz[b][col]) for the 16 columns of block `blk` -- 16 row groups (8 loads
// in flight each) summed through LDS in a fixed order; the column's first row group hands the sum over
constexpr int CS_COLS = 16, CS_GROUPS = 16;
template <typename Store>
__device__ __forceinline__ void colsum_body(const float* dz, const int ld, const int rows, const int n_valid, const int blk,
                                            const Store store) {
    __shared__ float red[CS_GROUPS][CS_COLS + 1];
    const int c = threadIdx.x & (CS_COLS - 1), g = threadIdx.x / CS_COLS;
    const int col = blk * CS_COLS + c;
    float s = 0.f;
    if (col < n_valid) {
        const float* p = dz + col;
        int b = g;
        for (; b + 7 * CS_GROUPS < rows; b += 8 * CS_GROUPS) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(b + k * CS_GROUPS) * ld];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; b < rows; b += CS_GROUPS) s += p[(size_t)b * ld];
    }
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && col < n_valid) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < CS_GROUPS; ++k) t += red[k][c];
        store(col, t);
    }
}
// split_sum4: float4 i of part[0] + part[1] + .. + part[n - 1] (`stride` floats apart), added in that order
__device__ __forceinline__ f32x4 split_sum4(const float* part, const int n, const size_t stride, const int64_t i) {
    f32x4 t = reinterpret_cast<const f32x4*>(part)[i];
    for (int z = 1; z < n; ++z) {
        const f32x4 v = reinterpret_cast<const f32x4*>(part + z * stride)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += v[k];
    }
    return t;
}
// db[n] = sum over the batch rows of dz[b][n]
__global__ __launch_bounds__(256) void k_graph_colsum(const float* dz, int ld, int rows, float* out, int n_valid) {
    colsum_body(dz, ld, rows, n_valid, blockIdx.x, [&](int col, float t) { out[col] = t; });
}
// the end of a layer's weight gradient: workgroups [0, nb_red) add the split-K partial products of dW in a fixed order,
// the rest are the bias column sums above
__global__ __launch_bounds__(256) void k_graph_wfinish(const float* part, int n_split, size_t stride, int64_t n4, float* out,
                                                       int nb_red, const float* dz, int ld, int rows, float* db, int n_valid) {
    if ((int)blockIdx.x < nb_red) {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n4) reinterpret_cast<f32x4*>(out)[i] = split_sum4(part, n_split, stride, i);
        return;
    }
    colsum_body(dz, ld, rows, n_valid, (int)blockIdx.x - nb_red, [&](int col, float t) { db[col] = t; });
}
// the same for a group of weight gradients (blockIdx.y = the problem): partial products at part + (y n_split + z) stride,
// outputs at out + c_off[y], bias column sums of dz + a_off[y] into db + bias_off[y]
__global__ __launch_bounds__(256) void k_graph_wfinish_group(const float* part, int n_split, size_t stride, int64_t n4, float* out,
                                                             int nb_red, const float* dz, int ld, int rows, float* db, int n_valid,
                                                             const GroupTab t) {
    const int gi = blockIdx.y;
    if ((int)blockIdx.x < nb_red) {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i < n4) reinterpret_cast<f32x4*>(out + t.c_off[gi])[i] = split_sum4(part + (size_t)gi * n_split * stride, n_split, stride, i);
        return;
    }
    colsum_body(dz + t.a_off[gi], ld, rows, n_valid, (int)blockIdx.x - nb_red, [&](int col, float v) { db[t.bias_off[gi] + col] = v; });
}
// ---- every weight gradient of a step in ONE launch.  dW_l = in_l^T dz_l needs nothing but the activations and the d z's,
// which stay in the workspaces until the step ends: the backward pass runs its chain of d-input contractions first and
// queues the weight gradients (host: queue_wgrad / flush_wgrads); here a flat grid walks the queue -- workgroup ->
// (problem, tile, split of the batch rows) through the prefix table -- so that 90 tiles of four layers (shared_bottom) or of
// an expert group + gate + tower share the 256 CUs instead of following one another in 2 launches per layer.
constexpr int MAX_WQ = 40;
struct WMulti {
    int n;
    int first[MAX_WQ + 1];          // first workgroup of problem p
    const float* A[MAX_WQ]; const float* B[MAX_WQ]; float* C[MAX_WQ];       // C: the partial products' base, or dW itself (split 1)
    int lda[MAX_WQ], ldb[MAX_WQ], N[MAX_WQ], tx[MAX_WQ], ty[MAX_WQ], K[MAX_WQ];     // K = batch rows per split
    int mn[MAX_WQ];                 // M x N (stride between the splits' partial products)
    int M[MAX_WQ];                  // rows of dW (ty = the tiles that cover them, the last one possibly in part)
};
__global__ __launch_bounds__(256) void k_graph_wgrad_multi(const WMulti t) {
    int p = 0;
    while (p + 1 < t.n && (int)blockIdx.x >= t.first[p + 1]) ++p;
    int b = (int)blockIdx.x - t.first[p];
    const int tiles = t.tx[p] * t.ty[p];
    const int bz = b / tiles;
    b -= bz * tiles;
    const int by = b / t.tx[p], bx = b - by * t.tx[p];
    GemmArgs a;
    a.A = t.A[p];
    a.lda = t.lda[p];
    a.B = t.B[p];
    a.ldb = t.ldb[p];
    a.C = t.C[p];
    a.ldc = t.N[p];
    a.K = t.K[p];
    a.zstride = (size_t)t.mn[p];
    a.m_rows = t.M[p];
    gemm_tile<2>(a, bx, by, bz);
}
// ... and their ends: per problem, the workgroups that add the splits' partial products in a fixed order, then the ones
// that sum the columns of d z into the bias gradient (k_graph_wfinish's two halves, the queue's problems side by side)
// where a finished gradient element goes: into the gradient vector (p null), or straight through the optimiser -- the
// step's k_graph_adam launch folded into the launch that finishes the gradients (the same arithmetic per element: opt_elem)
struct GradSink {
    const float* g_base;        // base of the gradient vector (element 0 = flat-vector element `table_floats`)
    float *p, *m, *v;           // parameters / slots addressed like g_base (m: the accumulator for MAMDR_OPT_ACCUMULATE)
    int optimizer;
    float alpha, omb1, omb2, eps;
};
// (opt_step's arithmetic, mamdr_device.h, with the SGD test first.  It stays a copy: with opt_step's order of the tests
// k_graph_tail, k_graph_adam and k_graph_fm_bwd<256> compile to different code -- profiles/step_kernels_refactor.txt)
__device__ __forceinline__ void opt_elem(const int optimizer, const float g, float& p, float& m, float& v, const float alpha,
                                         const float omb1, const float omb2, const float eps) {
    if (optimizer == MAMDR_OPT_SGD) {
        p = p - g * alpha;
    } else if (optimizer == MAMDR_OPT_ACCUMULATE) {
        m = m + g;
    } else {        // TF1 ApplyAdam: m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); p -= m alpha / (sqrt(v) + eps)
        m = m + (g - m) * omb1;
        v = v + (g * g - v) * omb2;
        p = p - (m * alpha) / (sqrtf(v) + eps);
    }
}
// four neighbouring elements through the optimiser: p / m / v loaded as far as it reads them, opt_elem per lane, stored as far
// as it writes them (sink4 and k_graph_adam).  mp / vp are only formed, never read or written, where the optimiser has no
// such slot: they need not be valid then
__device__ __forceinline__ void opt_step4(const int optimizer, const f32x4 g, float* pp, float* mp, float* vp, const float alpha,
                                          const float omb1, const float omb2, const float eps) {
    f32x4 p = *reinterpret_cast<const f32x4*>(pp);
    f32x4 m = optimizer != MAMDR_OPT_SGD ? *reinterpret_cast<const f32x4*>(mp) : (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 v = optimizer == MAMDR_OPT_ADAM ? *reinterpret_cast<const f32x4*>(vp) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        opt_elem(optimizer, g[k], pk, mk, vk, alpha, omb1, omb2, eps);
        p[k] = pk; m[k] = mk; v[k] = vk;
    }
    if (optimizer != MAMDR_OPT_ACCUMULATE) *reinterpret_cast<f32x4*>(pp) = p;
    if (optimizer != MAMDR_OPT_SGD) *reinterpret_cast<f32x4*>(mp) = m;
    if (optimizer == MAMDR_OPT_ADAM) *reinterpret_cast<f32x4*>(vp) = v;
}
// no sink: the gradient is stored (the kernels of the per-layer plan)
__device__ __forceinline__ GradSink no_sink() {
    GradSink none;
    none.p = nullptr;
    return none;
}
__device__ __forceinline__ void sink1(const GradSink& s, float* gptr, const float g) {
    if (!s.p) {
        *gptr = g;
        return;
    }
    const size_t i = (size_t)(gptr - s.g_base);
    float p = s.p[i], m = s.m[i], v = s.optimizer == MAMDR_OPT_ADAM ? s.v[i] : 0.f;
    opt_elem(s.optimizer, g, p, m, v, s.alpha, s.omb1, s.omb2, s.eps);
    if (s.optimizer != MAMDR_OPT_ACCUMULATE) s.p[i] = p;
    if (s.optimizer != MAMDR_OPT_SGD) s.m[i] = m;
    if (s.optimizer == MAMDR_OPT_ADAM) s.v[i] = v;
}
__device__ __forceinline__ void sink4(const GradSink& s, float* gptr, const f32x4 g) {
    if (!s.p) {
        *reinterpret_cast<f32x4*>(gptr) = g;
        return;
    }
    const size_t i = (size_t)(gptr - s.g_base);
    opt_step4(s.optimizer, g, s.p + i, s.m + i, s.v + i, s.alpha, s.omb1, s.omb2, s.eps);
}
struct WFinish {
    int n;
    int first[MAX_WQ + 1];
    const float* part[MAX_WQ]; float* out[MAX_WQ]; const float* dz[MAX_WQ]; float* db[MAX_WQ];
    int split[MAX_WQ], nb_red[MAX_WQ], N[MAX_WQ], rows[MAX_WQ], ld[MAX_WQ], mn[MAX_WQ];
};
__device__ __forceinline__ void wfinish_multi_body(const WFinish& t, const int bid, const GradSink& sk) {
    int p = 0;
    while (p + 1 < t.n && bid >= t.first[p + 1]) ++p;
    const int bi = bid - t.first[p];
    if (bi < t.nb_red[p]) {
        const int64_t i = (int64_t)bi * 256 + threadIdx.x;
        if (i < t.mn[p] / 4) sink4(sk, t.out[p] + 4 * i, split_sum4(t.part[p], t.split[p], (size_t)t.mn[p], i));
        return;
    }
    float* db = t.db[p];
    colsum_body(t.dz[p], t.ld[p], t.rows[p], t.N[p], bi - t.nb_red[p], [&](int col, float v) { sink1(sk, db + col, v); });
}
// d x of a group's first layers: out[b][c] (+)= sum over the members of part[e][b][c], in member order
__global__ __launch_bounds__(256) void k_graph_dx_reduce(const float* part, int n_part, size_t stride, int rows, int n4_row,
                                                         float* out, int ld, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * n4_row) return;
    const int b = (int)(i / n4_row), c4 = (int)(i - (int64_t)b * n4_row);
    f32x4 v = split_sum4(part, n_part, stride, i);
    float* o = out + (size_t)b * ld + 4 * c4;
    if (accumulate) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = w[k] + v[k];
    }
    *reinterpret_cast<f32x4*>(o) = v;
}

// out[j][e] = sum_b in[b][j] * d[b][e]  for narrow right-hand sides (gate kernel Wg: e < n_e <= 32; head: n_e = 1; the
// attention projections: n_e = 128): 16 outputs per workgroup, the rows split over 16 groups summed through LDS in order
__device__ __forceinline__ void small_tn_body(const float* in, int in_ld, const float* d, int d_ld, int rows, int n_j, int n_e,
                                              float* out, float* sum_out, const int bid, const int nblk, const GradSink& sk) {
    __shared__ float red[CS_GROUPS][CS_COLS + 1];
    if (sum_out && bid == nblk - 1) {       // one more workgroup: sum_out[0] = sum over the rows of d[b][0], fixed order
        float* r1 = &red[0][0];                         // (the head's d global bias beside its d kernel: one launch less)
        float s1 = 0.f;
        for (int b = threadIdx.x; b < rows; b += 256) s1 += d[(size_t)b * d_ld];
        r1[threadIdx.x] = s1;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) r1[threadIdx.x] += r1[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) sink1(sk, sum_out, r1[0]);
        return;
    }
    const int c = threadIdx.x & (CS_COLS - 1), g = threadIdx.x / CS_COLS;
    const int idx = bid * CS_COLS + c;
    float s = 0.f;
    if (idx < n_j * n_e) {
        const int j = idx / n_e, e = idx - j * n_e;
        const float *pi = in + j, *pd = d + e;
        int b = g;
        for (; b + 3 * CS_GROUPS < rows; b += 4 * CS_GROUPS) {
            float x[4], y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k] = pi[(size_t)(b + k * CS_GROUPS) * in_ld];
                y[k] = pd[(size_t)(b + k * CS_GROUPS) * d_ld];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s = fmaf(x[k], y[k], s);
        }
        for (; b < rows; b += CS_GROUPS) s = fmaf(pi[(size_t)b * in_ld], pd[(size_t)b * d_ld], s);
    }
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && idx < n_j * n_e) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < CS_GROUPS; ++k) t += red[k][c];
        sink1(sk, out + idx, t);
    }
}
__global__ __launch_bounds__(256) void k_graph_small_tn(const float* in, int in_ld, const float* d, int d_ld, int rows,
                                                        int n_j, int n_e, float* out, float* sum_out) {
    small_tn_body(in, in_ld, d, d_ld, rows, n_j, n_e, out, sum_out, blockIdx.x, gridDim.x, no_sink());
}

}  // namespace
