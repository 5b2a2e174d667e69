// Generic-layer engine, device side 3 / 5: what the towers add around the contractions -- gather, field interactions, CCPM,
// attention, gate, head, loss.  After graph_reduce.h (GradSink, sink1, no_sink; MAX_MIX is here).
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
#pragma once
#include "mamdr_kernels.h"

namespace {
using namespace mamdr;

constexpr int MAX_MIX = 32; // experts one task mixes (PLE: specific + shared)

// ------------------------------------------------------------------ gather
struct GatherArgs {
    const float *user_tab, *item_tab, *dm;
    const int32_t *uid, *pid, *dom, *perm;
    const float* label;
    int64_t row_base, n_rows_split;
    int rows, rows_pad, n_user, n_item, n_domain;
    float* x;
    int ld;
    int32_t* domrow;
    float* y;
    int32_t *urow, *irow, *map_u, *map_i;      // trainable tables: row of each position, first position of each row
    const float *lin_u, *lin_i, *lin_d;         // NFM: 1-d linear tables (lin_u / lin_i null while frozen at their zero init)
    float* extra;                               // NFM: sum of the linear terms per position
    float* xt;                                  // AutoInt: compact [rows_pad][384] copy of x (token-major: row 3 b + t)
};
// E = 128: one wave per batch position -- lanes 0..31 copy the user row, 32..63 the item row, then lanes 0..31 the domain row.
// Any accepted width E (32 / 64 / 128 / 256): a row's [user | item] pair is 2 E floats = E / 2 lanes of 16 bytes, so a wave
// serves 128 / E rows (4 at E = 32, where a table row is exactly one 128-byte line and 8 neighbouring lanes read it whole;
// 2 at E = 64) and at E = 256 every lane takes two vectors per field.  The first E / 4 lanes of a row's group then copy
// the domain row.  `sub` = the lane's float4 within the 2 E floats of [user | item].
template <int E>
__global__ __launch_bounds__(256) void k_graph_gather(const GatherArgs a) {
    constexpr int LPF = E / 4;                              // lanes (float4s) per field
    constexpr int GROUP = 2 * LPF < 64 ? 2 * LPF : 64;      // lanes that share a row
    constexpr int RPW = 64 / GROUP;                         // rows per wave
    constexpr int NJ = 2 * LPF / GROUP;                     // vectors per lane and pass
    const int lane = threadIdx.x & 63;
    const int r = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / GROUP, sub0 = lane % GROUP;
    if (r >= a.rows_pad) return;
    float* xr = a.x + (size_t)r * a.ld;
    if (r >= a.rows) {          // padding rows: zeros in, nothing out (their d loss / d logit is zero)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int sub = sub0 + 64 * j;
            *reinterpret_cast<f32x4*>(xr + 4 * sub) = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (sub < LPF) *reinterpret_cast<f32x4*>(xr + 2 * E + 4 * sub) = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (E == EMB && a.xt) {
                *reinterpret_cast<f32x4*>(a.xt + (size_t)r * XDIM + 4 * sub) = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (sub < LPF) *reinterpret_cast<f32x4*>(a.xt + (size_t)r * XDIM + 2 * EMB + 4 * sub) = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        if (sub0 == 0) {
            a.domrow[r] = -1;
            a.y[r] = 0.f;
            if (a.urow) { a.urow[r] = -1; a.irow[r] = -1; }
            if (a.extra) a.extra[r] = 0.f;
        }
        return;
    }
    int64_t src = a.perm ? (int64_t)a.perm[a.row_base + r] : a.row_base + r;
    src = src < 0 ? 0 : (src >= a.n_rows_split ? a.n_rows_split - 1 : src);
    int u = a.uid[src], it = a.pid[src], d = a.dom[src];
    u = u < 0 ? 0 : (u >= a.n_user ? a.n_user - 1 : u);
    it = it < 0 ? 0 : (it >= a.n_item ? a.n_item - 1 : it);
    d = d < 0 ? 0 : (d >= a.n_domain ? a.n_domain - 1 : d);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int sub = sub0 + 64 * j;
        const float* row = sub < LPF ? a.user_tab + (size_t)u * E + 4 * sub : a.item_tab + (size_t)it * E + 4 * (sub - LPF);
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(row);
        *reinterpret_cast<f32x4*>(xr + 4 * sub) = v0;
        if (E == EMB && a.xt) *reinterpret_cast<f32x4*>(a.xt + (size_t)r * XDIM + 4 * sub) = v0;
        if (sub < LPF) {
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.dm + (size_t)d * E + 4 * sub);
            *reinterpret_cast<f32x4*>(xr + 2 * E + 4 * sub) = v1;
            if (E == EMB && a.xt) *reinterpret_cast<f32x4*>(a.xt + (size_t)r * XDIM + 2 * EMB + 4 * sub) = v1;
        }
    }
    if (sub0 == 0) {
        a.domrow[r] = d;
        a.y[r] = a.label[src];
        if (a.extra) a.extra[r] = ((a.lin_u ? a.lin_u[u] : 0.f) + (a.lin_i ? a.lin_i[it] : 0.f)) + a.lin_d[d];
        if (a.urow) {       // representative of a table row = its smallest batch position (integer atomicMin: exact)
            a.urow[r] = u;
            a.irow[r] = it;
            atomicMin(a.map_u + u, r);
            atomicMin(a.map_i + it, r);
        }
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// ------------------------------------------------------------------ NFM / PNN: interactions of the three fields, one wave per row
// kind 0 (NFM): f[c] = u i + u d + i d (= 1/2 ((u+i+d)^2 - u^2 - i^2 - d^2), BiInteractionPooling), 128 columns
// kind 1 (PNN): f[0..2] = <u,i>, <u,d>, <i,d> (InnerProductLayer over the pairs (0,1), (0,2), (1,2))
// kind 2 (DeepFM): the FM second-order term  sum_k (u i + u d + i d)_k  joins the linear logit of the row (`extra`); no columns
struct FeatArgs {
    float* act; float* dact; int ld; int f_col; int rows_pad; int kind; int dx_all;
    const float* w_ip;      // PNN: rows 384..386 of the first kernel [3][n_out]
    int z_col, n_out;       // PNN: d z of the first layer
    float* extra;           // DeepFM: the per-row logit terms outside the DNN (linear part; the FM term is added here)
    const float* dlogit;    // DeepFM: d loss / d logit of the row
};
__global__ __launch_bounds__(256) void k_graph_feat_fwd(const FeatArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows_pad) return;
    float* row = a.act + (size_t)r * a.ld;
    const f32x2 u = *reinterpret_cast<const f32x2*>(row + 2 * lane), it = *reinterpret_cast<const f32x2*>(row + EMB + 2 * lane),
                d = *reinterpret_cast<const f32x2*>(row + 2 * EMB + 2 * lane);
    if (a.kind == 0) {
        f32x2 f;
#pragma unroll
        for (int k = 0; k < 2; ++k) f[k] = fmaf(it[k], d[k], fmaf(u[k], d[k], u[k] * it[k]));
        *reinterpret_cast<f32x2*>(row + a.f_col + 2 * lane) = f;
    } else if (a.kind == 2) {
        float f = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) f += fmaf(it[k], d[k], fmaf(u[k], d[k], u[k] * it[k]));
        f = wave_sum(f);
        if (lane == 0) a.extra[r] += f;
    } else {
        const float ui = wave_sum(fmaf(u[1], it[1], u[0] * it[0])), ud = wave_sum(fmaf(u[1], d[1], u[0] * d[0])),
                    id = wave_sum(fmaf(it[1], d[1], it[0] * d[0]));
        if (lane == 0) {
            row[a.f_col + 0] = ui;
            row[a.f_col + 1] = ud;
            row[a.f_col + 2] = id;
            row[a.f_col + 3] = 0.f;
        }
    }
}
// d f -> d x.  NFM: d u = df (i + d), d i = df (u + d), d d = df (u + i), WRITTEN (nothing else feeds d x).
// PNN: dip_j = sum_c dz[c] W0[384 + j][c]; d u += dip0 i + dip1 d, d i += dip0 u + dip2 d, d d += dip1 u + dip2 i, ADDED
// to what the first layer's d x = dz W0[0:384]^T left there.  User / item columns only when the tables train.
__global__ __launch_bounds__(256) void k_graph_feat_bwd(const FeatArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows_pad) return;
    const float* row = a.act + (size_t)r * a.ld;
    float* drow = a.dact + (size_t)r * a.ld;
    const f32x2 u = *reinterpret_cast<const f32x2*>(row + 2 * lane), it = *reinterpret_cast<const f32x2*>(row + EMB + 2 * lane),
                d = *reinterpret_cast<const f32x2*>(row + 2 * EMB + 2 * lane);
    f32x2 du, di, dd;
    if (a.kind == 0) {
        const f32x2 df = *reinterpret_cast<const f32x2*>(drow + a.f_col + 2 * lane);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            du[k] = df[k] * (it[k] + d[k]);
            di[k] = df[k] * (u[k] + d[k]);
            dd[k] = df[k] * (u[k] + it[k]);
        }
    } else if (a.kind == 2) {
        // DeepFM: d fm / d e_f = the sum of the other two fields' rows, ADDED to what the DNN's first layer left in d x
        const float dl = a.dlogit[r];
        const f32x2 du0 = *reinterpret_cast<const f32x2*>(drow + 2 * lane), di0 = *reinterpret_cast<const f32x2*>(drow + EMB + 2 * lane),
                    dd0 = *reinterpret_cast<const f32x2*>(drow + 2 * EMB + 2 * lane);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            du[k] = du0[k] + dl * (it[k] + d[k]);
            di[k] = di0[k] + dl * (u[k] + d[k]);
            dd[k] = dd0[k] + dl * (u[k] + it[k]);
        }
    } else {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        for (int c = lane; c < a.n_out; c += 64) {
            const float z = drow[a.z_col + c];
            p0 = fmaf(z, a.w_ip[c], p0);
            p1 = fmaf(z, a.w_ip[a.n_out + c], p1);
            p2 = fmaf(z, a.w_ip[2 * a.n_out + c], p2);
        }
        p0 = wave_sum(p0);
        p1 = wave_sum(p1);
        p2 = wave_sum(p2);
        const f32x2 du0 = *reinterpret_cast<const f32x2*>(drow + 2 * lane), di0 = *reinterpret_cast<const f32x2*>(drow + EMB + 2 * lane),
                    dd0 = *reinterpret_cast<const f32x2*>(drow + 2 * EMB + 2 * lane);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            du[k] = du0[k] + (p0 * it[k] + p1 * d[k]);
            di[k] = di0[k] + (p0 * u[k] + p2 * d[k]);
            dd[k] = dd0[k] + (p1 * u[k] + p2 * it[k]);
        }
    }
    if (a.dx_all) {
        *reinterpret_cast<f32x2*>(drow + 2 * lane) = du;
        *reinterpret_cast<f32x2*>(drow + EMB + 2 * lane) = di;
    }
    *reinterpret_cast<f32x2*>(drow + 2 * EMB + 2 * lane) = dd;
}
// DeepFM at a field width E other than 128 (32 / 64 / 256; the 128-wide tower stays on kind 2 above, whose summation order
// its recorded results are held to).  A row's field is E / 4 lanes of 16 bytes, so a wave serves 256 / E rows (8 at E = 32,
// 4 at E = 64, 1 at E = 256) and the FM term  sum_k (u i + u d + i d)_k  is a butterfly over the row's lanes alone.
template <int E>
__global__ __launch_bounds__(256) void k_graph_fm_fwd(const FeatArgs a) {
    constexpr int LPR = E / 4, RPW = 64 / LPR;              // lanes per row, rows per wave
    const int lane = threadIdx.x & 63, c4 = lane % LPR;
    const int r = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    if (r >= a.rows_pad) return;        // (rows_pad is a multiple of 64: the row's lanes leave together)
    const float* row = a.act + (size_t)r * a.ld + 4 * c4;
    const f32x4 u = *reinterpret_cast<const f32x4*>(row), it = *reinterpret_cast<const f32x4*>(row + E),
                d = *reinterpret_cast<const f32x4*>(row + 2 * E);
    float f = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) f += fmaf(it[k], d[k], fmaf(u[k], d[k], u[k] * it[k]));
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) f += __shfl_xor(f, o);
    if (c4 == 0) a.extra[r] += f;
}
// d fm / d e_f = d logit x the sum of the other two fields' rows, ADDED to what the DNN's first layer left in d x
// (user / item columns only when the tables train)
template <int E>
__global__ __launch_bounds__(256) void k_graph_fm_bwd(const FeatArgs a) {
    constexpr int LPR = E / 4, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, c4 = lane % LPR;
    const int r = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
    if (r >= a.rows_pad) return;
    const float* row = a.act + (size_t)r * a.ld + 4 * c4;
    float* drow = a.dact + (size_t)r * a.ld + 4 * c4;
    const f32x4 u = *reinterpret_cast<const f32x4*>(row), it = *reinterpret_cast<const f32x4*>(row + E),
                d = *reinterpret_cast<const f32x4*>(row + 2 * E);
    const float dl = a.dlogit[r];
    f32x4 dd = *reinterpret_cast<const f32x4*>(drow + 2 * E);
#pragma unroll
    for (int k = 0; k < 4; ++k) dd[k] = dd[k] + dl * (u[k] + it[k]);
    *reinterpret_cast<f32x4*>(drow + 2 * E) = dd;
    if (a.dx_all) {
        f32x4 du = *reinterpret_cast<const f32x4*>(drow), di = *reinterpret_cast<const f32x4*>(drow + E);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            du[k] = du[k] + dl * (it[k] + d[k]);
            di[k] = di[k] + dl * (u[k] + d[k]);
        }
        *reinterpret_cast<f32x4*>(drow) = du;
        *reinterpret_cast<f32x4*>(drow + E) = di;
    }
}
// NFM's linear domain table: g[d] = sum over the batch rows of domain d of d loss / d logit  +  2 l2_lin w[d]
// one workgroup per domain: rows strided over the 256 threads, LDS tree in a fixed order
__device__ __forceinline__ void lin_domain_grad_body(const float* dlogit, const int32_t* domrow, int rows, const float* w, float two_l2,
                                                     float* g, const int d, const GradSink& sk) {
    __shared__ float red[256];
    float s = 0.f;
    for (int b = threadIdx.x; b < rows; b += 256) s += domrow[b] == d ? dlogit[b] : 0.f;
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sink1(sk, g + d, red[0] + two_l2 * w[d]);
}
__global__ __launch_bounds__(256) void k_graph_lin_domain_grad(const float* dlogit, const int32_t* domrow, int rows, const float* w,
                                                               float two_l2, int n_domain, float* g) {
    lin_domain_grad_body(dlogit, domrow, rows, w, two_l2, g, blockIdx.x, no_sink());
}

// ------------------------------------------------------------------ CCPM: convolutions over the FIELD axis, one wave per row
// (deepctr CCPM with the three fields of this model, conv_kernel_width (6, 5), conv_filters (4, 4) -- oracle/fmnets.py:
// Conv2D((6, 1), 'same', tanh) over [3 fields x 128], maximum over the fields (KMaxPooling, k = 1), Conv2D((5, 1)) on the
// one row left = its centre tap, tanh; features [128 x 4]).  conv = [w1 6x4 | b1 4 | w2 4x4 (in, out) | b2 4] = 48 floats.
struct CcpmArgs {
    float* act; float* dact; int ld; int f_col, cg_col; int rows_pad; int dx_all;
    const float* conv;
};
// a1 of (position, filter) for the three raw values of one embedding column, its maximum and where it sits
__device__ __forceinline__ void ccpm_unit(const float* __restrict__ cv, const float (&x)[3], float (&m1)[4], int (&arg)[4],
                                          float (&a2)[4]) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        float best = -3.0e38f;
        int at = 0;
#pragma unroll
        for (int pos = 0; pos < 3; ++pos) {
            float pre = 0.f;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int src = pos + t - 2;        // TF 'same' for an even kernel: 2 taps before, 3 after
                if (src >= 0 && src < 3) pre += x[src] * cv[t * 4 + f];
            }
            const float a = tanhf(pre + cv[24 + f]);
            if (a > best) { best = a; at = pos; }  // (the first maximum wins a tie, as numpy's argmax)
        }
        m1[f] = best;
        arg[f] = at;
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float pre = 0.f;
#pragma unroll
        for (int f = 0; f < 4; ++f) pre += m1[f] * cv[28 + f * 4 + o];
        a2[o] = tanhf(pre + cv[44 + o]);
    }
}
__global__ __launch_bounds__(256) void k_graph_ccpm_fwd(const CcpmArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows_pad) return;
    float* row = a.act + (size_t)r * a.ld;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = 2 * lane + q;
        const float x[3] = {row[e], row[EMB + e], row[2 * EMB + e]};
        float m1[4], a2[4];
        int arg[4];
        ccpm_unit(a.conv, x, m1, arg, a2);
        *reinterpret_cast<f32x4*>(row + a.f_col + 4 * e) = (f32x4){a2[0], a2[1], a2[2], a2[3]};
    }
}
// d features -> d x and the row's share of the 48 convolution gradients (summed over the batch by k_graph_colsum)
__global__ __launch_bounds__(256) void k_graph_ccpm_bwd(const CcpmArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows_pad) return;
    const float* row = a.act + (size_t)r * a.ld;
    float* drow = a.dact + (size_t)r * a.ld;
    const float* cv = a.conv;
    float gc[48];
#pragma unroll
    for (int k = 0; k < 48; ++k) gc[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = 2 * lane + q;
        const float x[3] = {row[e], row[EMB + e], row[2 * EMB + e]};
        float m1[4], a2[4], dx[3] = {0.f, 0.f, 0.f};
        int arg[4];
        ccpm_unit(cv, x, m1, arg, a2);
        const f32x4 df = *reinterpret_cast<const f32x4*>(drow + a.f_col + 4 * e);
        float dm1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float dp2 = df[o] * (1.0f - a2[o] * a2[o]);
            gc[44 + o] += dp2;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                gc[28 + f * 4 + o] += m1[f] * dp2;
                dm1[f] += dp2 * cv[28 + f * 4 + o];
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const float dp1 = dm1[f] * (1.0f - m1[f] * m1[f]);      // m1 = a1 at its maximum
            gc[24 + f] += dp1;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
#pragma unroll
                for (int pos = 0; pos < 3; ++pos) {
                    const int src = pos + t - 2;
                    if (src >= 0 && src < 3 && pos == arg[f]) {
                        gc[t * 4 + f] += x[src] * dp1;
                        dx[src] += dp1 * cv[t * 4 + f];
                    }
                }
            }
        }
        if (a.dx_all) {
            drow[e] = dx[0];
            drow[EMB + e] = dx[1];
        }
        drow[2 * EMB + e] = dx[2];
    }
#pragma unroll
    for (int k = 0; k < 48; ++k) {
        const float v = wave_sum(gc[k]);
        if (lane == 0) drow[a.cg_col + k] = v;
    }
}

// ------------------------------------------------------------------ AutoInt: multi-head self-attention over the three fields
// (deepctr InteractingLayer, att_embedding_size 8, 4 heads, residual, no scaling -- oracle/fmnets.py).  Token-major compact
// buffers: row 3 b + t = field t of batch row b.  Per layer: P = X W (k_graph_gemm, W = [W_query | W_key | W_value | W_res],
// [d][128]) -> per batch row (one wave): scores Q_h K_h^T [3 x 3] per head, softmax over the fields, A V, + R, relu.
constexpr int ATT_OUT = 32, ATT_DIM = 8, ATT_P = 4 * ATT_OUT;      // 4 heads x 8; 128 projection columns per token
struct AttArgs {
    const float* P;      // [3 rows_pad][128]
    float* A;            // [rows_pad][36]: probabilities [head][field][field]
    float* Y;            // [3 rows_pad][32]
    const float* dY;     // [3 rows_pad][32] (backward)
    float* dP;           // [3 rows_pad][128] (backward)
    float* top; int top_ld;      // forward, last layer: also [rows_pad][96] inside the activation workspace (for the head)
    const float* dtop; int dtop_ld;   // backward, last layer: d Y comes from the gradient workspace
    int rows_pad;
};
__global__ __launch_bounds__(256) void k_graph_att_fwd(const AttArgs a) {
    __shared__ float lds[4][3 * ATT_P + 48];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + w;
    if (r >= a.rows_pad) return;
    float* p = lds[w];
    float* sc = p + 3 * ATT_P;
    for (int i = lane; i < 3 * ATT_P; i += 64) p[i] = a.P[(size_t)r * 3 * ATT_P + i];
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) {
        const int h = lane / 9, t = (lane % 9) / 3, s_ = lane % 3;
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < ATT_DIM; ++j) v = fmaf(p[t * ATT_P + h * ATT_DIM + j], p[s_ * ATT_P + ATT_OUT + h * ATT_DIM + j], v);
        sc[lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) {
        const int base = lane - lane % 3;
        const float m = fmaxf(fmaxf(sc[base], sc[base + 1]), sc[base + 2]);
        const float e0 = __expf(sc[base] - m), e1 = __expf(sc[base + 1] - m), e2 = __expf(sc[base + 2] - m);
        const float mine = __expf(sc[lane] - m) / ((e0 + e1) + e2);
        a.A[(size_t)r * 36 + lane] = mine;
        __builtin_amdgcn_wave_barrier();
        sc[lane] = mine;
    } else {
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < 3 * ATT_OUT; i += 64) {
        const int t = i / ATT_OUT, c = i % ATT_OUT, h = c / ATT_DIM;
        float o = 0.f;
#pragma unroll
        for (int s_ = 0; s_ < 3; ++s_) o = fmaf(sc[h * 9 + t * 3 + s_], p[s_ * ATT_P + 2 * ATT_OUT + c], o);
        const float y = fmaxf(o + p[t * ATT_P + 3 * ATT_OUT + c], 0.f);
        a.Y[(size_t)r * 3 * ATT_OUT + i] = y;
        if (a.top) a.top[(size_t)r * a.top_ld + i] = y;
    }
}
__global__ __launch_bounds__(256) void k_graph_att_bwd(const AttArgs a) {
    __shared__ float lds[4][3 * ATT_P + 48 + 48 + 96];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + w;
    if (r >= a.rows_pad) return;
    float* p = lds[w];
    float* pa = p + 3 * ATT_P;       // probabilities
    float* ds = pa + 48;             // d scores
    float* dz = ds + 48;             // d (O + R) = d Y through the relu
    for (int i = lane; i < 3 * ATT_P; i += 64) p[i] = a.P[(size_t)r * 3 * ATT_P + i];
    if (lane < 36) pa[lane] = a.A[(size_t)r * 36 + lane];
    for (int i = lane; i < 3 * ATT_OUT; i += 64) {
        const float dy = a.dtop ? a.dtop[(size_t)r * a.dtop_ld + i] : a.dY[(size_t)r * 3 * ATT_OUT + i];
        dz[i] = a.Y[(size_t)r * 3 * ATT_OUT + i] > 0.f ? dy : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    float da = 0.f;
    if (lane < 36) {
        const int h = lane / 9, t = (lane % 9) / 3, s_ = lane % 3;
#pragma unroll
        for (int j = 0; j < ATT_DIM; ++j) da = fmaf(dz[t * ATT_OUT + h * ATT_DIM + j], p[s_ * ATT_P + 2 * ATT_OUT + h * ATT_DIM + j], da);
        ds[lane] = da * pa[lane];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 36) {
        const int base = lane - lane % 3;
        const float dot = (ds[base] + ds[base + 1]) + ds[base + 2];
        const float v = pa[lane] * (da - dot);
        __builtin_amdgcn_wave_barrier();
        ds[lane] = v;
    } else {
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    float* dp = a.dP + (size_t)r * 3 * ATT_P;
    for (int i = lane; i < 3 * ATT_OUT; i += 64) {
        const int t = i / ATT_OUT, c = i % ATT_OUT, h = c / ATT_DIM;
        float dq = 0.f, dk = 0.f, dv = 0.f;
#pragma unroll
        for (int s_ = 0; s_ < 3; ++s_) {
            dq = fmaf(ds[h * 9 + t * 3 + s_], p[s_ * ATT_P + ATT_OUT + c], dq);           // d Q[t] = sum_s dS[t][s] K[s]
            dk = fmaf(ds[h * 9 + s_ * 3 + t], p[s_ * ATT_P + c], dk);                      // d K[t] = sum_s dS[s][t] Q[s]
            dv = fmaf(pa[h * 9 + s_ * 3 + t], dz[s_ * ATT_OUT + c], dv);                   // d V[t] = sum_s A[s][t] dZ[s]
        }
        dp[t * ATT_P + c] = dq;
        dp[t * ATT_P + ATT_OUT + c] = dk;
        dp[t * ATT_P + 2 * ATT_OUT + c] = dv;
        dp[t * ATT_P + 3 * ATT_OUT + c] = dz[i];
    }
}
// out[r][k] = sum_c d[r][c] W[k][c] for a NARROW result (k < n_k <= 32; c < n_c): d X of the 32-wide attention layers
__global__ __launch_bounds__(256) void k_graph_small_nt(const float* d, int n_c, const float* W, int n_k, int rows, float* out) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * n_k) return;
    const int r = idx / n_k, k = idx - r * n_k;
    const f32x4* dr = reinterpret_cast<const f32x4*>(d + (size_t)r * n_c);       // n_c is a multiple of 4 (128)
    const f32x4* wr = reinterpret_cast<const f32x4*>(W + (size_t)k * n_c);
    float s = 0.f;
    for (int c4 = 0; c4 < n_c / 4; c4 += 4) {           // 16-B loads, eight in flight; the chain keeps its order
        f32x4 x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = dr[c4 + u];
            y[u] = wr[c4 + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) s = fmaf(x[u][q], y[u][q], s);
    }
    out[idx] = s;
}
// d x[:, first .. first + n) (+)= compact [rows][384] columns first .. first + n
__global__ __launch_bounds__(256) void k_graph_add_x(float* dact, int ld, const float* src, int rows, int first, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * n) return;
    const int r = idx / n, c = first + (idx - r * n);
    dact[(size_t)r * ld + c] += src[(size_t)r * XDIM + c];
}

// ------------------------------------------------------------------ gate: softmax(q Wg) and the mixture, one wave per row
struct GateArgs {
    float* act; float* dact; int ld;
    int q_col, n_q;             // gate DNN output
    const float* wg; int n_e;   // [n_q][n_e]
    int e_col[MAX_MIX];         // last-layer output of each mixed expert
    int n_h;                    // expert width
    int g_col, m_col;           // gate probabilities (n_e columns), mixture (n_h columns)
    int rows_pad;
    float gate_scale;           // 1 / keep of the dropout behind every DNN layer (1 in inference)
};
// One workgroup per batch row (4 waves: the gate logits / the d gate sums are dealt over the waves, the expert width over all
// 256 lanes) -- with one wave per row the 1,024 rows of a batch were 1,024 waves on 1,024 SIMDs, each walking its experts'
// reductions one after the other (23 us for 12 experts).  Same summation orders as that form: bit-identical results.
__global__ __launch_bounds__(256) void k_graph_gate_fwd(const GateArgs a) {
    __shared__ float sl[MAX_MIX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float* row = a.act + (size_t)r * a.ld;
    for (int e = w; e < a.n_e; e += 4) {
        float s = 0.f;
        for (int j = lane; j < a.n_q; j += 64) s = fmaf(row[a.q_col + j], a.wg[j * a.n_e + e], s);
        s = wave_sum(s);
        if (lane == 0) sl[e] = s;
    }
    __syncthreads();
    float mx = -3.0e38f;
    for (int e = 0; e < a.n_e; ++e) mx = fmaxf(mx, sl[e]);
    float den = 0.f;
    for (int e = 0; e < a.n_e; ++e) den += __expf(sl[e] - mx);
    if (tid < a.n_e) row[a.g_col + tid] = __expf(sl[tid] - mx) / den;
    for (int cidx = tid; cidx < a.n_h; cidx += 256) {
        float m = 0.f;
        for (int e = 0; e < a.n_e; ++e) m += (__expf(sl[e] - mx) / den) * row[a.e_col[e] + cidx];
        row[a.m_col + cidx] = m;
    }
}
// d mixture -> d expert outputs (times their relu / dropout gate = d z of the experts' last layers), d gate logits
// (kept: dWg = q^T dgl) and d q (times q's gate = d z of the gate DNN's last layer)
__global__ __launch_bounds__(256) void k_graph_gate_bwd(const GateArgs a) {
    __shared__ float sdg[MAX_MIX], sgp[MAX_MIX];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = a.act + (size_t)r * a.ld;
    float* drow = a.dact + (size_t)r * a.ld;
    for (int e = w; e < a.n_e; e += 4) {
        float t = 0.f;
        for (int cidx = lane; cidx < a.n_h; cidx += 64) t = fmaf(drow[a.m_col + cidx], row[a.e_col[e] + cidx], t);
        t = wave_sum(t);
        if (lane == 0) {
            sdg[e] = t;
            sgp[e] = row[a.g_col + e];
        }
    }
    __syncthreads();
    float s = 0.f;
    for (int e = 0; e < a.n_e; ++e) s = fmaf(sgp[e], sdg[e], s);
    for (int cidx = tid; cidx < a.n_h; cidx += 256) {
        const float dm = drow[a.m_col + cidx];
        for (int e = 0; e < a.n_e; ++e) {
            const float h = row[a.e_col[e] + cidx];
            drow[a.e_col[e] + cidx] = h > 0.f ? (sgp[e] * dm) * a.gate_scale : 0.f;
        }
    }
    __syncthreads();        // (every read of d mixture is done before g_col / q_col, which may neighbour it, are written)
    if (tid < a.n_e) drow[a.g_col + tid] = sgp[tid] * (sdg[tid] - s);        // d gate logit
    for (int j = tid; j < a.n_q; j += 256) {
        float v = 0.f;
        for (int e = 0; e < a.n_e; ++e) v = fmaf(sgp[e] * (sdg[e] - s), a.wg[j * a.n_e + e], v);
        drow[a.q_col + j] = row[a.q_col + j] > 0.f ? v * a.gate_scale : 0.f;
    }
}

// ------------------------------------------------------------------ head: Dense(1, no bias) + global bias, sigmoid, Keras BCE
struct HeadArgs {
    const float* act; float* dact; int ld;
    int t_col, n_t;
    int n_plain;                // leading columns that no dropout follows (AutoInt: the attention output): gate only
    const float* w; const float* gb;
    const float* y; int rows, rows_pad;
    const float* extra;         // NFM: the linear logit of every position (null otherwise)
    float* dlogit; float* rowloss;
    int train; float gate_scale;
    const float* thresholds; uint32_t* hist; float* pred_out;       // inference
    const float* log_var; const int32_t* domrow;    // weighted loss (training only): d logit scaled by 1 / var^2, var =
                                                    // log_var[domain of the batch's FIRST row] (weighted_loss.py:38-41)
};
// the logit of row r, in every lane of its wave: the head's one reduction order (k_graph_head and the retrieval head of
// graph_retrieval.h form it here, so a retrieval score is the evaluation's score)
__device__ __forceinline__ float head_logit(const HeadArgs& a, int r, int lane) {
    const float* row = a.act + (size_t)r * a.ld;
    float s = 0.f;
    for (int cidx = lane; cidx < a.n_t; cidx += 64) s = fmaf(row[a.t_col + cidx], a.w[cidx], s);
    return wave_sum(s) + a.gb[0] + (a.extra ? a.extra[r] : 0.f);
}
__global__ __launch_bounds__(256) void k_graph_head(const HeadArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows_pad) return;
    const float* row = a.act + (size_t)r * a.ld;
    const float logit = head_logit(a, r, lane);
    float p;
    if (logit >= 0.f) {
        p = 1.0f / (1.0f + __expf(-logit));
    } else {
        const float ez = __expf(logit);
        p = ez / (1.0f + ez);
    }
    const bool valid = r < a.rows;
    const float y = a.y[r];
    const float lo = 1e-7f, hi = 1.0f - 1e-7f;
    const float pc = fminf(fmaxf(p, lo), hi);
    const float zc = __logf(pc / (1.0f - pc));
    const float loss = fmaxf(zc, 0.f) - zc * y + __logf(1.0f + __expf(-fabsf(zc)));
    if (lane == 0) a.rowloss[r] = valid ? loss : 0.f;
    if (a.train) {
        const float inside = (p >= lo && p <= hi) ? 1.0f : 0.0f;
        float dl = valid ? ((p - y) * inside) / (float)a.rows : 0.f;
        if (a.log_var) {
            const float var = a.log_var[a.domrow[0]];
            dl *= 1.0f / (var * var);
        }
        if (lane == 0) a.dlogit[r] = dl;
        float* drow = a.dact + (size_t)r * a.ld;
        for (int cidx = lane; cidx < a.n_t; cidx += 64)
            drow[a.t_col + cidx] = row[a.t_col + cidx] > 0.f ? (dl * a.w[cidx]) * (cidx < a.n_plain ? 1.0f : a.gate_scale) : 0.f;
    } else if (lane == 0 && valid) {
        int blo = 0, bhi = 500;          // AUC bin = number of thresholds strictly below p (utils/metrics_utils.py:309)
        while (blo < bhi) {
            const int mid = (blo + bhi) >> 1;
            if (a.thresholds[mid] < p) blo = mid + 1; else bhi = mid;
        }
        atomicAdd(a.hist + (y != 0.f ? 501 : 0) + blo, 1u);
        if (a.pred_out) a.pred_out[r] = p;
    }
}

// batch loss = mean of the rows' BCE + l2 (sum of squares of the three tables); one workgroup, fixed order.
// mode 0: out[0] = loss;  mode 1 (evaluation): out[0] += loss
__global__ __launch_bounds__(256) void k_graph_loss(const float* rowloss, int rows, const float* dm, int dm_count, float l2,
                                                    const float* frozen_sumsq, float* out, int mode, const float* lin_d,
                                                    int n_lin_d, float l2_lin, const float* log_var = nullptr,
                                                    const int32_t* domrow = nullptr, float* g_log_var = nullptr,
                                                    int n_domain = 0) {
    __shared__ float red[256];
    float s = 0.f, q = 0.f;
    for (int b = threadIdx.x; b < rows; b += 256) s += rowloss[b];
    for (int e = threadIdx.x; e < dm_count; e += 256) q = fmaf(dm[e], dm[e], q);
    float ql = 0.f;         // NFM: l2_lin * (sum of squares of the three 1-d linear tables)
    if (threadIdx.x == 0 && lin_d) {
        for (int e = 0; e < n_lin_d; ++e) ql = fmaf(lin_d[e], lin_d[e], ql);
        ql = l2_lin * ((frozen_sumsq[2] + frozen_sumsq[3]) + ql);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float tot = red[0];
    __syncthreads();
    red[threadIdx.x] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float data = tot / (float)rows;
        if (log_var) {      // weighted_loss.py:30-35: mean(BCE / var^2 + log var); d / d var = -2 mean(BCE) / var^3 + 1 / var
            const int d0 = domrow[0];
            const float var = log_var[d0];
            for (int d = 0; d < n_domain; ++d) g_log_var[d] = d == d0 ? -2.0f * data / (var * var * var) + 1.0f / var : 0.f;
            data = (1.0f / (var * var)) * data + logf(var);
        }
        const float loss = data + l2 * ((frozen_sumsq[0] + frozen_sumsq[1]) + red[0]) + ql;
        out[0] = mode ? out[0] + loss : loss;
    }
}
__global__ void k_graph_scale(float* x, float s) { x[0] *= s; }

}  // namespace
