// Generic-layer engine, device side 5 / 5: the Star forms' own kernels.  Needs nothing of the four headers before it; it stands last
// because its kernels always stood last in the code object.
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
#pragma once
#include "mamdr_kernels.h"

namespace {
using namespace mamdr;

// ------------------------------------------------------------------ Star forms (MAMDR_GRAPH_STAR)
// model_zoo/Star/star.py:70-96 as a family: norm none / PartitionedNorm / BatchNormalization, Dense / StarFCN hidden layers,
// the auxiliary network.  Everything per-domain is selected by d = the domain id of the batch's FIRST row, read on the
// device (partitioned_norm.py:136, star_fcn.py:112, auxiliary_net.py:100).  The contractions are the engine's own; here:
//   k_star_colstats<false>  per-chunk sum x / sum x^2 of the 384 input columns, double partials          (forward)
//   k_star_norm_fwd         the partials summed in chunk order, batch moments, x -> xn, the moving statistics' update of the
//                           right flavour (PN: domain d's pair, zero-debiased; BN: one pair, plain); evaluation: moving statistics
//   k_star_colstats<true>   per-chunk sum dxn / sum dxn x^                                                 (backward)
//   k_star_norm_bwd         s1, s2 finished in chunk order, dx, the norm's parameter gradients (zeros for the other domains)
//   k_star_eff              the step's effective tensors into scratch: Ws (.) Wd[d], bs + bd[d], aux_W[d], aux_b[d]
//   k_star_chain            scratch gradients dK / db -> g(Ws), g(Wd[d]), g(bs), g(bd[d]), g(aux_W[d]), g(aux_b[d]), zeros elsewhere
//   k_star_join_fwd / bwd   top = h_n + a; d top through both relu gates
// BatchNormalization's moving-average rule is restated from Keras' `_assign_moving_average` of TF 1.12 (no zero-debias) and,
// like every inner-step statement of this project, is PARITY UNPINNED against TF itself.
constexpr int SN_ROWS = 128;            // batch rows per chunk of a column reduction
constexpr int SN_VEC = XDIM / 4;        // float4 columns of a row (96); a block = 96 x 4 row lanes
constexpr float BN_DECAY = 0.01f;       // float32(1.0 - 0.99): Keras hands `1.0 - momentum` over as a Python float
struct StarNormArgs {
    const float* x; float* xn; int ld;          // raw input columns / normalised columns of the activation workspace
    const float* dxn; float* dx;                // their gradients
    int rows, rows_pad, n_chunks, n_domain;
    int norm, train;                            // 1 pn, 2 bn
    const int32_t* domrow;
    double* part;                               // [n_chunks][2][384]
    float* pnv;                                 // this step's [mean | inv | gamma inv], 3 x 384
    const float *gs, *bs, *gd, *bd;             // pn: shared / specific; bn: gs = gamma, bs = beta
    float *g_gs, *g_bs, *g_gd, *g_bd;
    float* aux;                                 // pn: [mov_mean | mov_var | biased_mean | biased_var] [D][384] each, steps [D]; bn: [mov_mean | mov_var] [384]
};
template <bool BWD>
__global__ __launch_bounds__(XDIM) void k_star_colstats(const StarNormArgs a) {
    __shared__ double sh[4][2][XDIM];
    const int tid = threadIdx.x, v = tid % SN_VEC, rl = tid / SN_VEC;
    const int r0 = blockIdx.x * SN_ROWS, r1 = min(r0 + SN_ROWS, a.rows);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, inv = mean;
    if (BWD) {
        mean = *reinterpret_cast<const f32x4*>(a.pnv + 4 * v);
        inv = *reinterpret_cast<const f32x4*>(a.pnv + XDIM + 4 * v);
    }
    for (int r = r0 + rl; r < r1; r += 4) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + (size_t)r * a.ld + 4 * v);
        if (BWD) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(a.dxn + (size_t)r * a.ld + 4 * v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = __fmul_rn(__fsub_rn(xv[k], mean[k]), inv[k]);
                s1[k] += (double)gv[k];
                s2[k] += (double)__fmul_rn(gv[k], xh);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double xd = (double)xv[k];
                s1[k] += xd;
                s2[k] += xd * xd;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sh[rl][0][4 * v + k] = s1[k];
        sh[rl][1][4 * v + k] = s2[k];
    }
    __syncthreads();
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {       // row lanes in lane order: fixed
        t1 += sh[q][0][tid];
        t2 += sh[q][1][tid];
    }
    a.part[(size_t)blockIdx.x * 2 * XDIM + tid] = t1;
    a.part[(size_t)blockIdx.x * 2 * XDIM + XDIM + tid] = t2;
}
// every block sums the chunks' partials itself (chunk order: the same bits in every block), block 0 keeps the results
__global__ __launch_bounds__(XDIM) void k_star_norm_fwd(const StarNormArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_scale[XDIM], sh_shift[XDIM];
    const int c = threadIdx.x, d = a.domrow[0];
    const bool pn = a.norm == 1, keep = blockIdx.x == 0;
    const size_t o = pn ? (size_t)d * XDIM + c : (size_t)c;
    const size_t dx = pn ? (size_t)a.n_domain * XDIM : (size_t)XDIM;       // floats per statistic
    float mean, var;
    if (a.train) {
        double S1 = 0.0, S2 = 0.0;
        for (int ch = 0; ch < a.n_chunks; ++ch) {
            S1 += a.part[(size_t)ch * 2 * XDIM + c];
            S2 += a.part[(size_t)ch * 2 * XDIM + XDIM + c];
        }
        // nn.moments: mean, then the population variance about that fp32 mean -- E[x^2] - 2 mean E[x] + mean^2 in double
        const double B = (double)a.rows, mu = S1 / B;
        mean = (float)mu;
        const double mf = (double)mean, vd = S2 / B - 2.0 * mf * mu + mf * mf;
        var = (float)(vd > 0.0 ? vd : 0.0);
        if (keep && pn) {
            // assign_moving_average(zero_debias=True): biased += (value - biased)(1 - momentum); moving = biased / (1 - momentum^step)
            const float t_step = a.aux[4 * dx + d] + 1.0f;
            const float factor = 1.0f - powf(PN_MOMENTUM, t_step), omm = 1.0f - PN_MOMENTUM;
            float bm = a.aux[2 * dx + o], bv = a.aux[3 * dx + o];
            bm += (mean - bm) * omm;
            bv += (var - bv) * omm;
            a.aux[2 * dx + o] = bm;
            a.aux[3 * dx + o] = bv;
            a.aux[o] = bm / factor;
            a.aux[dx + o] = bv / factor;
            __syncthreads();            // (every thread of the block has read the old step)
            if (c == 0) a.aux[4 * dx + d] = t_step;
        } else if (keep) {
            // Keras BatchNormalization._assign_moving_average (TF 1.12): moving -= (moving - value)(1 - momentum)
            const float mm = a.aux[o], mv = a.aux[dx + o];
            a.aux[o] = __fsub_rn(mm, __fmul_rn(__fsub_rn(mm, mean), BN_DECAY));
            a.aux[dx + o] = __fsub_rn(mv, __fmul_rn(__fsub_rn(mv, var), BN_DECAY));
        }
    } else {
        mean = a.aux[o];
        var = a.aux[dx + o];
    }
    const float inv = 1.0f / sqrtf(var + PN_EPS);
    const float gamma = pn ? a.gs[c] * a.gd[(size_t)d * XDIM + c] : a.gs[c];
    const float beta = pn ? a.bs[c] + a.bd[(size_t)d * XDIM + c] : a.bs[c];
    const float scale = __fmul_rn(inv, gamma);
    sh_scale[c] = scale;
    sh_shift[c] = __fsub_rn(beta, __fmul_rn(mean, scale));
    if (keep && a.train) {
        a.pnv[c] = mean;
        a.pnv[XDIM + c] = inv;
        a.pnv[2 * XDIM + c] = __fmul_rn(gamma, inv);
    }
    __syncthreads();
    const int v = c % SN_VEC, rl = c / SN_VEC;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(sh_scale + 4 * v), sf = *reinterpret_cast<const f32x4*>(sh_shift + 4 * v);
    const int r0 = blockIdx.x * SN_ROWS, r1 = min(r0 + SN_ROWS, a.rows_pad);
    for (int r = r0 + rl; r < r1; r += 4) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + (size_t)r * a.ld + 4 * v);
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = __fadd_rn(__fmul_rn(xv[k], sc[k]), sf[k]);
        *reinterpret_cast<f32x4*>(a.xn + (size_t)r * a.ld + 4 * v) = y;
    }
}
// s1 = sum dxn, s2 = sum dxn x^ (chunk order); dx = gamma inv (dxn - s1 / B - x^ s2 / B); block 0: the parameter gradients
__global__ __launch_bounds__(XDIM) void k_star_norm_bwd(const StarNormArgs a) {
    __shared__ __attribute__((aligned(16))) float sh_t1[XDIM], sh_t2[XDIM];
    const int c = threadIdx.x, d = a.domrow[0];
    double S1 = 0.0, S2 = 0.0;
    for (int ch = 0; ch < a.n_chunks; ++ch) {
        S1 += a.part[(size_t)ch * 2 * XDIM + c];
        S2 += a.part[(size_t)ch * 2 * XDIM + XDIM + c];
    }
    const float s1 = (float)S1, s2 = (float)S2, B = (float)a.rows;
    sh_t1[c] = __fdiv_rn(s1, B);
    sh_t2[c] = __fdiv_rn(s2, B);
    if (blockIdx.x == 0) {
        if (a.norm == 1) {
            a.g_bs[c] = s1;
            a.g_gs[c] = __fmul_rn(s2, a.gd[(size_t)d * XDIM + c]);
            const float gg = __fmul_rn(s2, a.gs[c]);
            for (int j = 0; j < a.n_domain; ++j) {
                a.g_gd[(size_t)j * XDIM + c] = j == d ? gg : 0.f;
                a.g_bd[(size_t)j * XDIM + c] = j == d ? s1 : 0.f;
            }
        } else {
            a.g_bs[c] = s1;
            a.g_gs[c] = s2;
        }
    }
    __syncthreads();
    const int v = c % SN_VEC, rl = c / SN_VEC;
    const f32x4 t1 = *reinterpret_cast<const f32x4*>(sh_t1 + 4 * v), t2 = *reinterpret_cast<const f32x4*>(sh_t2 + 4 * v);
    const f32x4 mean = *reinterpret_cast<const f32x4*>(a.pnv + 4 * v), inv = *reinterpret_cast<const f32x4*>(a.pnv + XDIM + 4 * v);
    const f32x4 coef = *reinterpret_cast<const f32x4*>(a.pnv + 2 * XDIM + 4 * v);
    const int r0 = blockIdx.x * SN_ROWS, r1 = min(r0 + SN_ROWS, a.rows_pad);
    for (int r = r0 + rl; r < r1; r += 4) {
        f32x4 y = {0.f, 0.f, 0.f, 0.f};
        if (r < a.rows) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + (size_t)r * a.ld + 4 * v);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(a.dxn + (size_t)r * a.ld + 4 * v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xh = __fmul_rn(__fsub_rn(xv[k], mean[k]), inv[k]);
                y[k] = __fmul_rn(coef[k], __fsub_rn(__fsub_rn(gv[k], t1[k]), __fmul_rn(xh, t2[k])));
            }
        }
        *reinterpret_cast<f32x4*>(a.dx + (size_t)r * a.ld + 4 * v) = y;
    }
}
// the per-domain tensors of a step: segment s of the scratch block = op(shared tensor, slice d of the specific tensor)
constexpr int MAX_SSEG = 10;            // 4 layers x (kernel, bias) + the auxiliary network's pair
enum { SSEG_MUL = 0, SSEG_ADD = 1, SSEG_COPY = 2 };
struct StarTab {
    int n;
    int first4[MAX_SSEG + 1];           // first float4 of segment s in the scratch block
    int64_t shared[MAX_SSEG], spec[MAX_SSEG];       // flat-vector offsets (shared unused for SSEG_COPY)
    int cnt[MAX_SSEG], op[MAX_SSEG];    // floats per slice
};
__global__ __launch_bounds__(256) void k_star_eff(const StarTab t, const float* params, const int32_t* domrow, float* eff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.first4[t.n]) return;
    int s = 0;
    while (s + 1 < t.n && i >= t.first4[s + 1]) ++s;
    const int e = 4 * (i - t.first4[s]), d = domrow[0];
    const f32x4 sp = *reinterpret_cast<const f32x4*>(params + t.spec[s] + (size_t)d * t.cnt[s] + e);
    f32x4 out = sp;
    if (t.op[s] != SSEG_COPY) {
        const f32x4 sh = *reinterpret_cast<const f32x4*>(params + t.shared[s] + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = t.op[s] == SSEG_MUL ? __fmul_rn(sh[k], sp[k]) : __fadd_rn(sh[k], sp[k]);
    }
    *reinterpret_cast<f32x4*>(eff + 4 * (size_t)i) = out;
}
// gbase is addressed like the flat vector (gradient of element `off` at gbase + off)
__global__ __launch_bounds__(256) void k_star_chain(const StarTab t, const float* params, const int32_t* domrow, const float* deff,
                                                    float* gbase, int n_domain) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.first4[t.n]) return;
    int s = 0;
    while (s + 1 < t.n && i >= t.first4[s + 1]) ++s;
    const int e = 4 * (i - t.first4[s]), d = domrow[0];
    const f32x4 dk = *reinterpret_cast<const f32x4*>(deff + 4 * (size_t)i);
    f32x4 gd = dk;
    if (t.op[s] == SSEG_MUL) {
        const f32x4 ws = *reinterpret_cast<const f32x4*>(params + t.shared[s] + e);
        const f32x4 wd = *reinterpret_cast<const f32x4*>(params + t.spec[s] + (size_t)d * t.cnt[s] + e);
        f32x4 gs;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gs[k] = __fmul_rn(dk[k], wd[k]);
            gd[k] = __fmul_rn(dk[k], ws[k]);
        }
        *reinterpret_cast<f32x4*>(gbase + t.shared[s] + e) = gs;
    } else if (t.op[s] == SSEG_ADD) {
        *reinterpret_cast<f32x4*>(gbase + t.shared[s] + e) = dk;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < n_domain; ++j)
        *reinterpret_cast<f32x4*>(gbase + t.spec[s] + (size_t)j * t.cnt[s] + e) = j == d ? gd : zero;
}
// the auxiliary branch's join (star.py:92-93): top = h_n + a; backward: d top through the relu of each summand
__global__ __launch_bounds__(256) void k_star_join_fwd(float* act, int ld, int h_col, int a_col, int top_col, int n, int rows_pad) {
    const int i = blockIdx.x * 256 + threadIdx.x, n4 = n / 4;
    if (i >= rows_pad * n4) return;
    float* row = act + (size_t)(i / n4) * ld;
    const int c = 4 * (i % n4);
    const f32x4 h = *reinterpret_cast<const f32x4*>(row + h_col + c), av = *reinterpret_cast<const f32x4*>(row + a_col + c);
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = __fadd_rn(h[k], av[k]);
    *reinterpret_cast<f32x4*>(row + top_col + c) = y;
}
__global__ __launch_bounds__(256) void k_star_join_bwd(const float* act, float* dact, int ld, int h_col, int a_col, int top_col, int n,
                                                       int rows_pad) {
    const int i = blockIdx.x * 256 + threadIdx.x, n4 = n / 4;
    if (i >= rows_pad * n4) return;
    const size_t ro = (size_t)(i / n4) * ld;
    const int c = 4 * (i % n4);
    const f32x4 h = *reinterpret_cast<const f32x4*>(act + ro + h_col + c), av = *reinterpret_cast<const f32x4*>(act + ro + a_col + c);
    const f32x4 dt = *reinterpret_cast<const f32x4*>(dact + ro + top_col + c);
    f32x4 dh, da;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        dh[k] = h[k] > 0.f ? dt[k] : 0.f;
        da[k] = av[k] > 0.f ? dt[k] : 0.f;
    }
    *reinterpret_cast<f32x4*>(dact + ro + h_col + c) = dh;
    *reinterpret_cast<f32x4*>(dact + ro + a_col + c) = da;
}

}  // namespace
