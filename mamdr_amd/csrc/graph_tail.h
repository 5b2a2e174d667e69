// Generic-layer engine, device side 4 / 5: the end of a step -- the domain table's gradient, the tail launch that finishes every
// queued gradient, the optimiser launch.  After graph_reduce.h (GradSink, sink1, no_sink, CS_*, opt_step4,
// wfinish_multi_body, small_tn_body) and graph_towers.h (lin_domain_grad_body).
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
#pragma once
#include "mamdr_kernels.h"

namespace {
using namespace mamdr;

// ------------------------------------------------------------------ domain table gradient
// g[d][c] = sum over the batch rows of domain d of d x[b][256 + c]  +  2 l2 Dm[d][c]   (rows in batch order)
// grid (8 column blocks, domains): 16 columns x 16 row groups per workgroup, 8 loads in flight, summed through LDS in a
// fixed order; a domain with no row in the batch (all but one of them in a domain step) leaves after one look at the ids.
// (emb = the table's width: emb / 16 column blocks, first column x_col = 2 emb of d x)
__device__ __forceinline__ void domain_grad_body(const float* dx, int ld, int x_col, const int32_t* domrow, int rows,
                                                 const float* dm, float two_l2, float* g, const int bx, const int by,
                                                 const int emb, const GradSink& sk) {
    __shared__ float red[CS_GROUPS][CS_COLS + 1];
    const int d = by, c = threadIdx.x & (CS_COLS - 1), rg = threadIdx.x / CS_COLS;
    const int col = bx * CS_COLS + c;
    int mine = 0;
    for (int b = threadIdx.x; b < rows; b += 256) mine |= domrow[b] == d;
    if (!__syncthreads_or(mine)) {
        if (rg == 0) sink1(sk, g + d * emb + col, two_l2 * dm[d * emb + col]);
        return;
    }
    const float* p = dx + x_col + col;
    float s = 0.f;
    int b = rg;
    for (; b + 7 * CS_GROUPS < rows; b += 8 * CS_GROUPS) {
        float v[8];
        int id[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            id[k] = domrow[b + k * CS_GROUPS];
            v[k] = p[(size_t)(b + k * CS_GROUPS) * ld];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s += id[k] == d ? v[k] : 0.f;
    }
    for (; b < rows; b += CS_GROUPS) s += domrow[b] == d ? p[(size_t)b * ld] : 0.f;
    red[rg][c] = s;
    __syncthreads();
    if (rg == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < CS_GROUPS; ++k) t += red[k][c];
        sink1(sk, g + d * emb + col, t + two_l2 * dm[d * emb + col]);
    }
}
__global__ __launch_bounds__(256) void k_graph_domain_grad(const float* dx, int ld, int x_col, const int32_t* domrow, int rows,
                                                           const float* dm, float two_l2, float* g, int emb) {
    domain_grad_body(dx, ld, x_col, domrow, rows, dm, two_l2, g, blockIdx.x, blockIdx.y, emb, no_sink());
}
// ---- the tail of a step's backward pass in ONE launch: the ends of the queued weight gradients (wfinish_multi_body's
// workgroups), the narrow contractions that were queued with them (head / gate kernels, PNN's inner-product rows, the
// attention projections: k_graph_small_tn's workgroups) and the domain table's gradient (k_graph_domain_grad's) -- all of
// them read what the backward pass left in the workspaces and write gradients nothing but the optimiser reads.
constexpr int MAX_TQ = 6;
struct TailJobs {
    int n_tn;
    int tn_first[MAX_TQ + 1];       // first workgroup (behind the weight gradients' ends) of narrow contraction q
    const float* in[MAX_TQ]; const float* d[MAX_TQ]; float* out[MAX_TQ]; float* sum_out[MAX_TQ];
    int in_ld[MAX_TQ], d_ld[MAX_TQ], rows[MAX_TQ], n_j[MAX_TQ], n_e[MAX_TQ];
    int dg_first, dg_blocks;        // the domain table's gradient: dg_emb / 16 column blocks x n_domain (0 blocks: not in this launch)
    int dg_emb;                     // ... its width
    const float* dx; int ld, x_col; const int32_t* domrow; int dg_rows; const float* dm; float two_l2; float* g_dm;
    int lin_blocks;                 // the 1-d linear domain table's gradient (k_graph_lin_domain_grad's workgroups: one per domain)
    const float* lin_dlogit; const float* lin_w; float lin_two_l2; float* lin_g;
    GradSink sink;                  // p non-null: every finished gradient element steps its parameter right here
};
__global__ __launch_bounds__(256) void k_graph_tail(const WFinish f, const TailJobs j) {
    const int nf = f.n ? f.first[f.n] : 0;
    int bid = blockIdx.x;
    if (bid < nf) {
        wfinish_multi_body(f, bid, j.sink);
        return;
    }
    bid -= nf;
    if (bid < j.dg_first) {
        int q = 0;
        while (q + 1 < j.n_tn && bid >= j.tn_first[q + 1]) ++q;
        small_tn_body(j.in[q], j.in_ld[q], j.d[q], j.d_ld[q], j.rows[q], j.n_j[q], j.n_e[q], j.out[q], j.sum_out[q],
                      bid - j.tn_first[q], j.tn_first[q + 1] - j.tn_first[q], j.sink);
        return;
    }
    bid -= j.dg_first;
    if (bid < j.dg_blocks) {
        const int cb = j.dg_emb / CS_COLS;
        domain_grad_body(j.dx, j.ld, j.x_col, j.domrow, j.dg_rows, j.dm, j.two_l2, j.g_dm, bid % cb, bid / cb, j.dg_emb, j.sink);
        return;
    }
    bid -= j.dg_blocks;
    if (bid < j.lin_blocks) lin_domain_grad_body(j.lin_dlogit, j.domrow, j.dg_rows, j.lin_w, j.lin_two_l2, j.lin_g, bid, j.sink);
}

// ------------------------------------------------------------------ optimiser on a range of the flat vector
struct AdamArgs {           // up to two ranges of the flat vector in one launch (the shared block and the task's block)
    float *p, *m, *v;       // bases of the flat vector / its slots (m: the accumulator for MAMDR_OPT_ACCUMULATE)
    const float* g;         // gradient base, addressed like p
    int64_t off4[2], n4[2]; // float4 offsets / counts of the ranges
    int optimizer;          // MAMDR_OPT_ADAM / MAMDR_OPT_SGD / MAMDR_OPT_ACCUMULATE (m += g, nothing else)
    float alpha, omb1, omb2, eps;
};
__global__ __launch_bounds__(256) void k_graph_adam(const AdamArgs a) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n4[0]) i += a.off4[0];
    else if (i - a.n4[0] < a.n4[1]) i = i - a.n4[0] + a.off4[1];
    else return;
    opt_step4(a.optimizer, reinterpret_cast<const f32x4*>(a.g)[i], a.p + 4 * i, a.m + 4 * i, a.v + 4 * i, a.alpha, a.omb1, a.omb2, a.eps);
}

}  // namespace
