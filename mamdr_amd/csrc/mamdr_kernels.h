// Internal launch interface between the C ABI (mamdr_api.hip, step_*.hip) and the kernel
// translation units.  Not part of the public boundary (include/mamdr_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "mamdr_device.h"
#include "wave_exchange.h"
#include "pregather_plan.h"
#include "host_base.h"

namespace mamdr {

// optimiser hyper-parameters of one step (shared by the dense and the table paths)
struct OptArgsLite {
    int optimizer;             // 0 adam, 1 sgd
    float alpha;               // adam: lr*sqrt(1-b2^t)/(1-b1^t); sgd: lr
    float omb1, omb2, eps;
    float two_l2;
};
constexpr int32_t EMB_UNTOUCHED = 0x7fffffff;

// Profiling (step_ctx.h: Prof): while a timed launch is being issued, g_prof_stop is the event the launch
// carries as its OWN stop event (hipExtLaunchKernelGGL: recorded by the kernel's completion, no marker packet
// between the kernels).  A kernel's time is then its stop event minus the stop event of the kernel before it.
extern thread_local hipEvent_t g_prof_stop;
int env_warn_unknown();          // step_context.hip: MAMDR_* names of the environment missing from env_registry.h, reported once
#define MAMDR_LAUNCH(kernel, grid, block, lds, stream, ...)                                               \
    do {                                                                                                  \
        if (::mamdr::g_prof_stop) {                                                                       \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, nullptr, ::mamdr::g_prof_stop, 0, __VA_ARGS__); \
            ::mamdr::g_prof_stop = nullptr;                                                               \
        } else {                                                                                          \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                            \
        }                                                                                                 \
    } while (0)

// ---- domain table under k_wgrad_adam.  Its gradient is a sum over the S workgroups' partials, i.e. a device-wide
// dependency inside the step.  Instead of a kernel of its own per step (4 us of launch + drain for 1,280 elements)
// the step stays PENDING: the next step's tower kernel applies it on the fly -- every workgroup recomputes the
// row(s) its samples use from (p, m, v before the step, the partials), workgroup d < n_domain also writes row d
// back -- and k_dm_finish materialises the last step of a mamdr_train_steps call.  All three sites run dm_step4:
// explicit roundings, the same bits wherever it is instantiated.
constexpr int DM_PARTS = 32;       // partial gradients per step = S workgroups of k_wgrad_adam
constexpr int DM_PAIRS = DM_PARTS / 2;
struct DmStep {
    const float* snap;         // [3][n_domain][EMB]: p, m, v of the domain table BEFORE the pending step; null = none pending
    const float* pdm;          // [n_part][n_domain][EMB] partial gradients of the pending step
    int n_part, n_domain;
    int optimizer;             // of the pending step: 0 adam, 1 sgd, 2 accumulate
    float alpha, omb1, omb2, eps, two_l2;
};
// Canonical arithmetic (every site, bit for bit): pair sums s_j = pdm[2 j] + pdm[2 j + 1] (j < 16), group sums
// G_q = ((s_4q + s_4q+1) + s_4q+2) + s_4q+3 (q < 4), g = ((G_0 + G_1) + G_2) + G_3, g += 2 l2 p, optimiser step with
// separately rounded operations.  (A tree, so that four lanes can each sum a quarter of the partials.)
__device__ __forceinline__ f32x4 dm_pair(const DmStep& q, int d, int c4, int j) {
#pragma clang fp contract(off)
    const size_t row = (size_t)d * EMB + 4 * c4, plane = (size_t)q.n_domain * EMB;
    const f32x4 a = *reinterpret_cast<const f32x4*>(q.pdm + (size_t)(2 * j) * plane + row);
    const f32x4 b = *reinterpret_cast<const f32x4*>(q.pdm + (size_t)(2 * j + 1) * plane + row);
    return a + b;
}
// (p, m, v of the row BEFORE the step: separate, so that a caller can request them ahead of a barrier)
__device__ __forceinline__ void dm_load4(const DmStep& q, int d, int c4, f32x4& p, f32x4& m, f32x4& v) {
    const size_t row = (size_t)d * EMB + 4 * c4, plane = (size_t)q.n_domain * EMB;
    p = *reinterpret_cast<const f32x4*>(q.snap + row);
    m = *reinterpret_cast<const f32x4*>(q.snap + plane + row);
    v = *reinterpret_cast<const f32x4*>(q.snap + 2 * plane + row);
}
__device__ __forceinline__ void dm_apply4(const DmStep& q, f32x4 g, f32x4& p, f32x4& m, f32x4& v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gk = g[k] + q.two_l2 * p[k];
        if (q.optimizer == 0) {
            m[k] = m[k] + (gk - m[k]) * q.omb1;
            v[k] = v[k] + (gk * gk - v[k]) * q.omb2;
            p[k] = p[k] - (m[k] * q.alpha) / (sqrtf(v[k]) + q.eps);
        } else if (q.optimizer == 1) {
            p[k] = p[k] - gk * q.alpha;
        } else {
            m[k] = m[k] + gk;
        }
    }
}
// one lane does it all (the writer workgroups and k_dm_finish: off the critical path): four batches of loads
__device__ __forceinline__ void dm_step4(const DmStep& q, int d, int c4, f32x4& p, f32x4& m, f32x4& v) {
#pragma clang fp contract(off)
    static_assert(DM_PAIRS == 16, "four groups of four pair sums");
    dm_load4(q, d, c4, p, m, v);
    f32x4 G[4];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        f32x4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = dm_pair(q, d, c4, 4 * gq + k);
        G[gq] = ((t[0] + t[1]) + t[2]) + t[3];
    }
    const f32x4 g = ((G[0] + G[1]) + G[2]) + G[3];
    dm_apply4(q, g, p, m, v);
}

// One launch of the fused tower kernel: gather -> MLP forward -> BCE -> (train:
// backward activation chain) over a contiguous range of positions of one split.
struct TowerArgs {
    // tables and dense parameters
    const float* user_tab;
    const float* item_tab;
    const float* dense;        // dense block base (domain table first)
    DenseLayout L;
    int n_user, n_item, n_domain;
    // bound split columns
    const int32_t* uid;
    const int32_t* pid;
    const int32_t* dom;
    const float* label;
    const int32_t* perm;       // nullable
    int64_t row_base;          // position (in perm order) of row 0 of this launch
    int64_t n_rows_split;      // rows in the bound split (for clamping)
    int rows;                  // rows covered by this launch (train: rows of the batch)
    int batch;                 // eval: batch size (loss is averaged per batch); train: == rows
    // dropout stream
    uint32_t seed, step, drop_thresh;
    float keep_scale;
    int use_dropout;
    // train outputs (workspace)
    float* acts;               // [rows_pad][ACT_LD]
    float* dz;                 // [rows_pad][DZ_LD]
    float* dlogit;             // [rows_pad]
    int32_t* domrow;           // [rows_pad]
    // trainable user / item tables only (null otherwise)
    float* dxe;                // [rows_pad][dx_ld]  d loss / d [user | item (| domain)] embedding row
    int dx_ld;                 // 256, or 384 for the Star tower
    const float* pn_aff;       // Star: [scale 384 | shift 384 | mean 384 | inv 384 | ...] of PartitionedNorm, null otherwise
    float* pn_part;            // Star training: [tiles][2][384] per-tile sums of PartitionedNorm's backward (s1 = sum dxn,
                               // s2 = sum dxn * xhat), written by the tower's tail and summed by k_star_pnb_final
    int32_t* urow;             // [rows_pad] user row of each batch position (-1 = padding)
    int32_t* irow;             // [rows_pad]
    int32_t* map_u;            // [n_user] / [n_item]: atomicMin of the batch position touching the row (null: frozen tables)
    int32_t* map_i;
    float* loss_part;          // [tiles] sum of per-row BCE of the tile
    // DeepFM: logit += FM second-order term + linear tables
    int deepfm;                // FM instances: 1 DeepFM, 2 WDL (linear tables only), 3 PNN (inner products of the field pairs)
    float* ipbuf;              // PNN: [rows_pad][4] inner products <u,i> <u,d> <i,d> of the batch's rows (train)
    const float* lin_user;     // [n_user] / [n_item] 1-d tables; null = frozen at their zero initialisation
    const float* lin_item;
    float* fmq;                // train: [rows_pad][EMB] dlogit * (user + item embedding), for the domain-table gradient
    // uncertainty weighting (model_zoo/uncertainty_weight/weighted_loss.py:30-43): the BCE term of the loss is
    // divided by var^2, var = dense[uw_off] (the batch's domain); -1 = off
    int uw_off;
    const float* wT;           // k_tower4 only: transposed W1 / W2 copies
    // k_wgrad_adam path, domain table (see DmStep): the pending step to apply on the fly, the live rows workgroup
    // d < n_domain writes back, and the snapshot [3][n_domain][EMB] of (p, m, v) as this step's forward pass saw them
    // pre-gathered pass (k_pass_prep; frozen tables on the k_wgrad_adam path): row i of this launch reads its
    // [user | item] embedding rows, domain and label at xpre[i], pdom[i], plabel[i] -- no chain of dependent loads
    const float* xpre;         // [rows][2 EMB], null = gather through perm / uid / pid
    const int32_t* pdom;
    const float* plabel;
    int no_w1l;                // k_tower4: keep streaming W1 / W1^T (MAMDR_T4_NO_W1L=1, diagnostic)
    int w2_direct;             // k_tower4<.., W1L, PRE>: the backward pass reads W2 itself instead of the copy W2T (every
                               // tower of a call where all of them can -- CallPlan::w2_all -- otherwise the first
                               // step of a call whose copies are stale)
    DmStep dms;
    int dm_hint;               // the domain the caller expects every row of the batch to carry (the pass's domain)
    float* dm_live_p;
    float* dm_live_m;
    float* dm_live_v;
    float* dm_snap_out;
    // eval outputs
    const float* thresholds;   // 500 fp32 AUC thresholds
    uint32_t* hist;            // [2][501]
    float* pred_out;           // nullable, [n_rows] in position order
#ifdef MAMDR_STAMPS
    unsigned long long* stamps; // diagnostic build only: [tiles][16] s_memtime stamps
#endif
};

// weight-gradient GEMMs (K = batch rows) + bias / output-layer / domain-table sums
struct TileDesc {
    int a_kind, a_off;         // 0: acts column block, 1: ones (row 0), 2: one-hot(domain) rows a_off.., 3: ipbuf columns (PNN)
    int b_kind, b_off;         // 0: dz column block, 1: dlogit (col 0), 2: fmq column block
    int dst_off, dst_ld;       // destination in the dense-block gradient slab
    int m_valid, n_valid;      // valid rows / cols of the 32x32 tile
    int big;                   // 1: full 64x64 tile of acts^T dz (LDS-staged path), 0: 32x32 tile with synthesised operands
};

struct WgradArgs {
    const float* acts;
    const float* dz;
    const float* dlogit;
    const int32_t* domrow;
    const float* fmq;          // DeepFM / PNN only
    const float* ipbuf;        // PNN only: [rows_pad][4]
    const TileDesc* tiles;
    int n_tiles;
    int rows_pad;              // batch rows rounded up to TILE_ROWS
    int n_groups;              // K-split groups (one gradient slab each)
    int rows_per_group;        // multiple of 8
    float* slabs;              // [n_groups][slab_ld]
    int slab_ld;
    // loss of the step (optional)
    const float* loss_part;
    int n_loss_tiles;
    int rows;                  // actual batch rows
    const float* dense;        // for the domain-table regulariser
    int dm_count;
    float l2_emb;
    const float* frozen_sumsq; // [4] sums of squares: user, item table; DeepFM linear user, item table
    int ld_off, ld_count;      // DeepFM: linear domain table inside the dense block (regulariser l2_lin)
    float l2_lin;
    int lv_off, lv_count, uw_d; // uncertainty weighting: per-domain scalars in the dense block, the batch's domain
    float* loss_out;           // nullable: 1 float
    const float* w0dom;        // W0[256:384, :] (live weights)
    float* w0dom_copy;         // its pre-update snapshot, read by k_update
    float* dm_copy;            // pre-update snapshot of the domain table (k_update: dW0[256:384] by linearity), nullable
#ifdef MAMDR_STAMPS
    unsigned long long* stamps; // diagnostic build only
#endif
};

struct UpdateArgs {
    float* p;                  // dense block of params
    float* m;
    float* v;
    const float* slabs;
    int n_groups;
    int slab_ld;
    int count4;                // float4 elements
    int dm_count;              // elements [0, dm_count): domain table, gradient = S . W0dom^T + 2*l2*p
    int s_off;                 // offset of S = onehot(domain)^T dz1 ([n_domain][256]) inside a slab
    const float* w0dom_copy;
    const float* dm_copy;      // not null: dW0[256:384, :] = Dm^T . S (the slabs carry no tiles for those rows)
    int n_domain;
    int s2_off;                // DeepFM: offset of S2 = onehot(domain)^T fmq ([n_domain][EMB]) inside a slab, 0 = none
    int ld_off, ld_count;      // DeepFM: linear domain table (gradient += 2 l2_lin p)
    float two_l2_lin;
    float two_l2;
    int optimizer;             // 0 adam, 1 sgd
    float alpha;               // adam: lr*sqrt(1-b2^t)/(1-b1^t); sgd: lr
    float omb1, omb2, eps;
    float* wT;                 // nullable: transposed W1 / W2 copies to keep current
    int w1_off, w2_off;        // offsets of W1 / W2 in the dense block
    int w0_off, w0t;           // W0 offset; w0t: also keep W0T (trainable tables)
    int no_sdm;                // NFM: rows 256..383 of W0 do not meet the domain row -- no S . W0dom^T term in the table's gradient
#ifdef MAMDR_STAMPS
    unsigned long long* stamps; // diagnostic build only: [workgroups][4] s_memtime stamps (entry, operands summed, exit)
#endif
};

// ---- the tile workgroups' domain-table duty (DmStep).  Everything is requested at kernel start, beside the weight
// prefetch, from the domain the caller expects (dm_hint: per-domain datasets carry one domain per batch), so the
// round trip to the partials hides behind the row bookkeeping's own dependent loads:
//   reader  all 512 lanes fetch one pair sum each of row dm_hint (16 pairs x 32 float4) -> LDS -> behind a barrier
//           32 lanes add them in order and step the row: the tile's x[256:384] (if the batch's rows do carry
//           dm_hint; otherwise every lane of a domain segment runs dm_step4 alone)
//   writer  workgroup d < n_domain does the same for row d with lanes 32..63 and writes it back: live p / m / v and
//           the snapshot [3][n_domain][EMB] this step's k_wgrad_adam and the next step's towers read
__device__ __forceinline__ void dm_apply1(const DmStep& q, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    const float gk = g + q.two_l2 * p;
    if (q.optimizer == 0) {
        m = m + (gk - m) * q.omb1;
        v = v + (gk * gk - v) * q.omb2;
        p = p - (m * q.alpha) / (sqrtf(v) + q.eps);
    } else if (q.optimizer == 1) {
        p = p - gk * q.alpha;
    } else {
        m = m + gk;
    }
}
// ---- the 4-row tower's form, without LDS and without a barrier: wave w owns the 16 domain columns its second
// layer-0 segment contracts; lane (l = lane & 15, q = lane >> 4) loads partials 8 q .. 8 q + 7 of column 16 w + l,
// sums its group G_q, and four cross-lane reads complete the tree.  Requested behind the row bookkeeping, consumed
// between layer 0's segments.
struct DmWave {
    float r[8], w[8];          // partials of the batch's domain row / of the row this workgroup writes back
    float rp, rm, rv, wp, wm, wv;
};
// addresses first (pure arithmetic, from the domain the caller expects: done while the row bookkeeping's loads are in
// flight), loads second (behind the bookkeeping barrier: a dozen instructions)
struct DmWaveAddr {
    const float* rb;           // partial 8 q of column c of row dm_hint; + k * plane for the others
    const float* wb;           // ... of row `tile`
    const float* rs;           // snapshot p of (dm_hint, c); + plane: m, + 2 plane: v
    const float* ws;           // snapshot (or live) p of (tile, c)
};
__device__ __forceinline__ void dm_wave_addr(const TowerArgs& a, int tile, DmWaveAddr& q) {
    const int lane = (int)threadIdx.x & 63, l = lane & 15, gq = lane >> 4, c = 16 * ((int)threadIdx.x >> 6) + l;
    const size_t plane = (size_t)a.n_domain * EMB;
    const size_t er = (size_t)a.dm_hint * EMB + c, ew = (size_t)min(tile, a.n_domain - 1) * EMB + c;
    q.rb = a.dms.pdm + (size_t)(8 * gq) * plane + er;
    q.wb = a.dms.pdm + (size_t)(8 * gq) * plane + ew;
    q.rs = a.dms.snap + er;
    q.ws = (a.dms.snap ? a.dms.snap : a.dm_live_p) + ew;
}
__device__ __forceinline__ void dm_wave_begin(const TowerArgs& a, int tile, bool do_read, const DmWaveAddr& q, DmWave& t) {
    const bool pend = a.dms.snap != nullptr, wr = tile < a.n_domain;      // uniform
    const size_t plane = (size_t)a.n_domain * EMB;
#pragma unroll
    for (int k = 0; k < 8; ++k) t.r[k] = t.w[k] = 0.f;
    t.rp = t.rm = t.rv = t.wp = t.wm = t.wv = 0.f;
    if (pend && do_read) {
#pragma unroll
        for (int k = 0; k < 8; ++k) t.r[k] = q.rb[(size_t)k * plane];
        t.rp = q.rs[0];
        t.rm = q.rs[plane];
        t.rv = q.rs[2 * plane];
    }
    if (wr) {
        if (pend) {
#pragma unroll
            for (int k = 0; k < 8; ++k) t.w[k] = q.wb[(size_t)k * plane];
            t.wp = q.ws[0];
            t.wm = q.ws[plane];
            t.wv = q.ws[2 * plane];
        } else {
            const size_t off = (size_t)(q.ws - a.dm_live_p);
            t.wp = q.ws[0];
            t.wm = a.dm_live_m[off];
            t.wv = a.dm_live_v[off];
        }
    }
}
__device__ __forceinline__ float dm_wave_sum(const float (&x)[8]) {
#pragma clang fp contract(off)
    const float G = (((x[0] + x[1]) + (x[2] + x[3])) + (x[4] + x[5])) + (x[6] + x[7]);
    float Gq[4];                   // G of lanes l, l + 16, l + 32, l + 48 (l = lane & 15), on the vector ALU: wave_exchange.h
    wave_gather_rows16(G, Gq);
    return ((Gq[0] + Gq[1]) + Gq[2]) + Gq[3];
}
// one element: the 16 staged pair sums of column c in order, then the step (the scalar form of dm_step4: same bits)
__device__ __forceinline__ void dm_elem_finish(const DmStep& q, int c, const float* parts, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    float t[DM_PAIRS];
#pragma unroll
    for (int j = 0; j < DM_PAIRS; ++j) t[j] = parts[j * EMB + c];
    float G[4];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) G[gq] = ((t[4 * gq] + t[4 * gq + 1]) + t[4 * gq + 2]) + t[4 * gq + 3];
    dm_apply1(q, ((G[0] + G[1]) + G[2]) + G[3], p, m, v);
}
// per-lane state of the tile workgroups' duty.  Only waves 4..7 take part: wave 0 runs the row bookkeeping's chain of
// dependent loads, and loads retire in order -- anything requested ahead of that chain is waited for with it.
//   waves 4..7 (256 lanes)  two pair sums each of the hinted row (and of the row to write back): lane L' = lane - 256
//                            owns float4 c4 = L' & 31 of pairs g and g + 8, g = L' >> 5
//   waves 4, 5 (reader)     lane L' < 128: (p, m, v) of column L' of the hinted row
//   waves 6, 7 (writer)     lane L' - 128: the same for the row this workgroup writes back
struct DmTile {
    f32x4 pr[2][2], pw[2][2];  // the two partials of each pair, as loaded: added only when staged (an add right behind
                               // the loads would make the wave wait out their round trip before its next barrier)
    float p, m, v;
};
__device__ __forceinline__ void dm_pair_load(const DmStep& q, int d, int c4, int j, f32x4 (&t)[2]) {
    const size_t row = (size_t)d * EMB + 4 * c4, plane = (size_t)q.n_domain * EMB;
    t[0] = *reinterpret_cast<const f32x4*>(q.pdm + (size_t)(2 * j) * plane + row);
    t[1] = *reinterpret_cast<const f32x4*>(q.pdm + (size_t)(2 * j + 1) * plane + row);
}
__device__ __forceinline__ f32x4 dm_pair_add(const f32x4 (&t)[2]) {
#pragma clang fp contract(off)
    return t[0] + t[1];
}
__device__ __forceinline__ void dm_tile_begin(const TowerArgs& a, int tile, int d_read, DmTile& t) {
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // scalar branches below: no divergence
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    t.pr[0][0] = t.pr[0][1] = t.pr[1][0] = t.pr[1][1] = zero;
    t.pw[0][0] = t.pw[0][1] = t.pw[1][0] = t.pw[1][1] = zero;
    t.p = t.m = t.v = 0.f;
    if (wv < 4) return;
    const bool pend = a.dms.snap != nullptr, wr = tile < a.n_domain;      // both uniform
    const int dw = min(tile, a.n_domain - 1);
    const int lp = (int)threadIdx.x - 256, grp = lp >> 5, c4 = lp & 31;
    if (pend) {
        dm_pair_load(a.dms, d_read, c4, grp, t.pr[0]);
        dm_pair_load(a.dms, d_read, c4, grp + 8, t.pr[1]);
        if (wr) {
            dm_pair_load(a.dms, dw, c4, grp, t.pw[0]);
            dm_pair_load(a.dms, dw, c4, grp + 8, t.pw[1]);
        }
    }
    const size_t plane = (size_t)a.n_domain * EMB;
    const int c = lp & (EMB - 1);
    if (wv < 6) {
        if (pend) {
            const size_t e = (size_t)d_read * EMB + c;
            t.p = a.dms.snap[e];
            t.m = a.dms.snap[plane + e];
            t.v = a.dms.snap[2 * plane + e];
        }
    } else if (wr) {
        const size_t e = (size_t)dw * EMB + c;
        if (pend) {
            t.p = a.dms.snap[e];
            t.m = a.dms.snap[plane + e];
            t.v = a.dms.snap[2 * plane + e];
        } else {
            t.p = a.dm_live_p[e];
            t.m = a.dm_live_m[e];
            t.v = a.dm_live_v[e];
        }
    }
}
// pair sums -> LDS parts[2][16][128] floats (16 KB)
__device__ __forceinline__ void dm_tile_stage(const TowerArgs& a, int tile, const DmTile& t, float* parts) {
    if (!a.dms.snap || threadIdx.x < 256) return;
    const int lp = (int)threadIdx.x - 256;
    *reinterpret_cast<f32x4*>(parts + lp * 4) = dm_pair_add(t.pr[0]);
    *reinterpret_cast<f32x4*>(parts + 1024 + lp * 4) = dm_pair_add(t.pr[1]);
    if (tile < a.n_domain) {
        *reinterpret_cast<f32x4*>(parts + 2048 + lp * 4) = dm_pair_add(t.pw[0]);
        *reinterpret_cast<f32x4*>(parts + 3072 + lp * 4) = dm_pair_add(t.pw[1]);
    }
}
// behind the barrier that follows dm_tile_stage: the hinted row's element c after the pending step
__device__ __forceinline__ float dm_tile_reader(const TowerArgs& a, int c, const float* parts, const DmTile& t) {
    float p = t.p, m = t.m, v = t.v;
    dm_elem_finish(a.dms, c, parts, p, m, v);
    return p;
}
__device__ __forceinline__ void dm_store_elem(const TowerArgs& a, size_t e, bool stepped, float p, float m, float v) {
    const size_t plane = (size_t)a.n_domain * EMB;
    if (stepped) {
        if (a.dms.optimizer != 2) a.dm_live_p[e] = p;
        if (a.dms.optimizer != 1) a.dm_live_m[e] = m;
        if (a.dms.optimizer == 0) a.dm_live_v[e] = v;
    }
    a.dm_snap_out[e] = p;
    a.dm_snap_out[plane + e] = m;
    a.dm_snap_out[2 * plane + e] = v;
}
// writer lanes (waves 6, 7: c = lane - 384), behind the same barrier
__device__ __forceinline__ void dm_tile_writer(const TowerArgs& a, int tile, int n_tiles, int c, const float* parts,
                                               const DmTile& t) {
    const bool pend = a.dms.snap != nullptr;
    if (tile < a.n_domain) {
        float p = t.p, m = t.m, v = t.v;
        if (pend) dm_elem_finish(a.dms, c, parts + 2048, p, m, v);
        dm_store_elem(a, (size_t)tile * EMB + c, pend, p, m, v);
    }
    // grids smaller than the domain count (tiny batches): the remaining rows, one lane chain per float4
    if (c < EMB / 4) {
        for (int d = tile + n_tiles; d < a.n_domain; d += n_tiles) {
            f32x4 p, m, v;
            const size_t row = (size_t)d * EMB + 4 * c, plane = (size_t)a.n_domain * EMB;
            if (pend) {
                dm_step4(a.dms, d, c, p, m, v);
                if (a.dms.optimizer != 2) *reinterpret_cast<f32x4*>(a.dm_live_p + row) = p;
                if (a.dms.optimizer != 1) *reinterpret_cast<f32x4*>(a.dm_live_m + row) = m;
                if (a.dms.optimizer == 0) *reinterpret_cast<f32x4*>(a.dm_live_v + row) = v;
            } else {
                p = *reinterpret_cast<const f32x4*>(a.dm_live_p + row);
                m = *reinterpret_cast<const f32x4*>(a.dm_live_m + row);
                v = *reinterpret_cast<const f32x4*>(a.dm_live_v + row);
            }
            *reinterpret_cast<f32x4*>(a.dm_snap_out + row) = p;
            *reinterpret_cast<f32x4*>(a.dm_snap_out + plane + row) = m;
            *reinterpret_cast<f32x4*>(a.dm_snap_out + 2 * plane + row) = v;
        }
    }
}

// Riders of k_wgrad_adam: the launch's own 242 / 243 workgroups leave CUs of a larger part idle for its whole span, and
// up to that many rider workgroups gather a slice of the NEXT pass window there (mamdr_pregather_ahead) -- what
// k_pass_prep_multi would write, bit for bit, into the pass-buffer set that window will adopt.  A rider owns FZ_RIDE_ROWS
// consecutive positions of the slice; the slice is at most two segments of one pass each (pregather_plan.h).
constexpr int FZ_RIDE_ROWS = 64;      // positions per rider and launch (8 rows per wave: 8 float4 loads in flight per lane)
constexpr int FZ_RIDE_CAP = 32;       // riders per launch, at most (and never more than the CUs the launch leaves idle)
struct RideArgs {
    const float* user_tab;
    const float* item_tab;
    float* xpre;               // the ahead set of the pass buffer
    int32_t* pdom;
    float* plabel;
    int n_user, n_item;
    int n_wg;                  // rider workgroups of this launch
    struct Seg {               // positions [first, first + count) of a pass of n rows (+ 16 padding rows) at row out_off
        const int32_t* uid;
        const int32_t* pid;
        const int32_t* dom;
        const float* label;
        const int32_t* perm;   // nullable
        int64_t out_off;
        int n, n_rows_split, first, count, pad_dom;
    } seg[2];
};
// k_wgrad_adam (fused_kernels.hip): weight gradients + optimiser step of the dense block in one launch
constexpr int FZ_F_W1T_UNREAD = 1;     // no tower launch of this context reads W1T (tower4_never_streams): W1T is left alone
constexpr int FZ_F_W2T_UNREAD = 2;     // every tower of this call reads W2 in place (k_tower4<.., W2D>): W2T is left alone too
constexpr int FZ_F_S_INORDER = 4;      // MAMDR_FZ_S_INORDER=1: S workgroup b takes column block b (A/B switch; same bits)
constexpr int FZ_F_DEAL_RESIDUE = 8;   // MAMDR_FZ_DEAL_RESIDUE=1 (or FZ_F_S_INORDER): the residue dealing of wgrad_adam_deal.h instead of
                                       // the dealing by matrix (A/B switch; same bits)
struct FusedArgs {
    const float* acts;         // [rows_pad][ACT_LD]
    const float* dz;           // [rows_pad][DZ_LD]
    const float* dlogit;       // [rows_pad]
    const int32_t* domrow;     // [rows_pad]
    const float* xa;           // A operand of dW0[0:256, :]: rows of [user | item] embeddings, leading dimension xa_ld
    int xa_ld;
    int rows_pad, rows;
    float* p;                  // dense block of params / slots (m = accumulator for optimizer 2)
    float* m;
    float* v;
    DenseLayout L;
    int n_domain;
    const float* dm_snap;      // pre-update domain table (the tower's dm_snap_out)
    float* pdm;                // [8][n_domain][EMB] partial domain-table gradients
    float* wT;                 // nullable: k_tower4's transposed W1 / W2 copies
    int flags;                 // FZ_F_* below (ONE word next to wT: the kernel fetches both with its first argument loads;
                               // as words of their own the compiler fetched them where they are used, behind the barrier)
    int optimizer;             // 0 adam, 1 sgd, 2 accumulate
    float alpha, omb1, omb2, eps, two_l2;
    const float* loss_part;    // loss of the step (optional)
    int n_loss_tiles;
    const float* frozen_sumsq;
    float l2_emb;
    float* loss_out;
    RideArgs ride;             // rider workgroups behind the launch's own (n_wg == 0: none)
#ifdef MAMDR_STAMPS
    unsigned long long* stamps; // diagnostic build only: [workgroups][8] s_memtime stamps of wave 0
#endif
};
void launch_wgrad_adam(const FusedArgs& a, hipStream_t s);
int wgrad_adam_own_wgs(bool with_loss);      // workgroups of a launch before its riders
// positions [pos0, pos0 + n) of a pass resolved once per mamdr_train_steps call: src = perm[pos] (or pos), clamped;
// xpre[i] = [user row | item row] of src, pdom[i] / plabel[i] its domain (clamped) and label
struct PassPrepArgs {
    const float* user_tab;
    const float* item_tab;
    const int32_t* uid;
    const int32_t* pid;
    const int32_t* dom;
    const float* label;
    const int32_t* perm;       // nullable
    int64_t pos0, n, n_rows_split;
    int n_user, n_item, n_domain;
    int pad_dom;               // domain written for the padding rows (the pass's domain)
    float* xpre;
    int32_t* pdom;
    float* plabel;
    // k_transpose_w's work riding in the same launch (both open a mamdr_train_steps call): workgroups
    // [n_prep_wgs, n_prep_wgs + TRANSPOSE_WGS) when tw_wT is set
    const float* tw_dense;
    DenseLayout tw_L;
    float* tw_wT;
    int n_prep_wgs;
};
// several passes in ONE launch (mamdr_pregather_passes): pass k owns workgroups [wg_end[k - 1], wg_end[k]) and the
// rows [out_off, out_off + n + 16) of the pass buffer
constexpr int PREP_MAX_PASSES = 16;
struct PassPrepMultiArgs {
    const float* user_tab;
    const float* item_tab;
    int n_user, n_item, n_domain, n_pass;
    float* xpre;
    int32_t* pdom;
    float* plabel;
    int wg_end[PREP_MAX_PASSES];
    struct Pass {
        const int32_t* uid;
        const int32_t* pid;
        const int32_t* dom;
        const float* label;
        const int32_t* perm;   // nullable
        int64_t n, n_rows_split, out_off;
        int64_t i0;            // first position of the launch in this pass (what riders gathered before it is skipped)
        int pad_dom;
    } p[PREP_MAX_PASSES];
};
void launch_pass_prep_multi(const PassPrepMultiArgs& a, hipStream_t s);
// ---- W1 [256][128] as an LDS image (both towers, when a workgroup has its CU to itself).  LDS-DMA
// (global_load_lds_dwordx4: 16 B per lane, two rows per wave instruction, no registers) writes a lane-linear image, so
// the swizzle sits on the SOURCE address: the 16-B chunk q of row r lives at chunk position q ^ (r & 31) -- row reads
// (layer 1's B operand) and column-chunk reads (its backward contraction) are both bank-conflict free.
// The requests are inline asm, i.e. NOT in the compiler's vmcnt bookkeeping: a counted LDS-DMA makes hipcc wait
// vmcnt(0) at the next use of any load.  Uncounted, they only make the counted waits behind them conservative (vmcnt
// retires in order); w1_image_landed() is the wait, a workgroup barrier must follow before another wave reads.
template <int ROWS>
__device__ __forceinline__ void w1_image_request(const float* __restrict__ W1, float* w1s, const int row0) {
    const int lane = threadIdx.x & 63;
    const uint32_t base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(w1s + row0 * H2));
#pragma unroll
    for (int kk = 0; kk < ROWS; kk += 2) {
        const int k = row0 + kk + (lane >> 5);
        const float* src = W1 + k * H2 + 4 * ((lane & 31) ^ (k & 31));
        const uint32_t dst = base + kk * H2 * 4;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
}
__device__ __forceinline__ void w1_image_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// float offset of W1[row][4 chunk + c] in the image
__device__ __forceinline__ int w1_image_at(int row, int chunk) { return row * H2 + 4 * (chunk ^ (row & 31)); }

constexpr int TRANSPOSE_WGS = (WT_FLOATS + 255) / 256;
// W1T / W2T / W0T element e from the live weights (see k_transpose_w)
__device__ __forceinline__ void transpose_w_elem(const float* dense, const DenseLayout& L, float* wT, int e) {
    if (e < H1 * H2) {
        const int r = e / H2, c = e - r * H2;               // W1[r][c], r < 256, c < 128
        wT[W1T_OFF + c * H1 + r] = dense[L.w1 + e];
    } else if (e < H1 * H2 + H2 * H3) {
        const int f = e - H1 * H2;
        const int r = f / H3, c = f - r * H3;               // W2[r][c], r < 128, c < 64
        wT[W2T_OFF + c * H2 + r] = dense[L.w2 + f];
    } else if (e < WT_FLOATS) {
        const int f = e - (H1 * H2 + H2 * H3);
        const int r = f / H1, c = f - r * H1;               // W0[r][c], r < 256 (user | item rows), c < 256
        wT[W0T_OFF + c * (2 * EMB) + r] = dense[L.w0 + f];
    }
}
void launch_pass_prep(const PassPrepArgs& a, hipStream_t s);
// materialise a pending domain-table step (end of a mamdr_train_steps call): live p / m / v := dm_step4
void launch_dm_finish(const DmStep& q, float* live_p, float* live_m, float* live_v, hipStream_t s);

void launch_tower_train(const TowerArgs& a, hipStream_t s);
void launch_tower_eval(const TowerArgs& a, hipStream_t s);
// -> 0, or one of T4_E_* (a state the caller's own predicate should have excluded / a refused LDS limit): the C ABI reports
// them as MAMDR_ESTATE / MAMDR_EHIP through mamdr_last_error -- the library never aborts
constexpr int T4_E_W2D_LDS = 1;        // k_tower4<.., W2D> was refused its LDS limit
constexpr int T4_E_W2D_STATE = 2;      // w2_direct asked of a launch that does not take the W1-image instance
int launch_tower4_train(const TowerArgs& a, hipStream_t s);
// the W1-image instance of the pre-gathered tower can run (its LDS limit was granted): grids of up to one tile per CU
bool tower4_w1l_ready();
bool tower4_takes_w1l(int64_t rows, int no_w1l);      // launch_tower4_train's choice of the W1-image instance for a batch
// no launch of the frozen-table mlp k_tower4 of up to max_rows rows, pre-gathered or not, can be a streaming instance
// (the only reader of W1T): every such grid fits one round of workgroups and both W1-image instances have their LDS limit
bool tower4_never_streams(int64_t max_rows, int no_w1l);
void launch_transpose_w(const float* dense, const DenseLayout& L, float* wT, hipStream_t s);
struct EvalFinishArgs {
    const float* loss_part;
    int64_t n_rows;
    int batch;
    const float* dense;
    int dm_count;
    float l2_emb;
    const float* frozen_sumsq; // [4]
    int ld_off, ld_count;
    float l2_lin;
    float* loss_out;
};
void launch_eval_finish(const EvalFinishArgs& a, hipStream_t s);
struct GatherPf;
void launch_wgrad(const WgradArgs& a, hipStream_t s, const GatherPf* pf = nullptr);
// the NEXT step's gather, touched ahead of time by rider workgroups in k_wgrad's launch.  What one kernel leaves in an
// XCD's L2 survives the kernel boundary (tools/probes/l2_survive_probe.hip: 240 cycles for a line the same workgroup id
// touched in the kernel before, 1,400 cold, 600 when another XCD touched it), and workgroup b of any 1-d grid runs on XCD
// b mod 8: rider b' = tile (mod 8) walks tile's dependent chain perm -> uid / pid / domain / label -> table rows, so the
// tower's three dependent misses per step become three L2 hits.
struct GatherPf {
    const int32_t *perm, *uid, *pid, *dom;
    const float* label;
    const float *user_tab, *item_tab;
    int64_t row_base, n_rows_split;
    int rows, n_user, n_item, n_tiles;     // n_tiles = 0: no rider
    float* sink;
};
void launch_update(const UpdateArgs& a, hipStream_t s);
void launch_gather(const TowerArgs& a, float* out, hipStream_t s);
void launch_sumsq(const float* x, int64_t n, float* partials /*>=1024 floats*/, float* out, hipStream_t s);

size_t tower_lds_bytes();

// emb_kernels.hip: trainable embedding tables (TF1 dense Adam over every row)
struct EmbTable {
    int64_t n_rows;
    const int32_t* brow;       // [rows] table row of each batch position (-1 = padding)
    int32_t* map;              // [n_rows] first batch position touching the row, EMB_UNTOUCHED otherwise (set by k_tower)
    float* gbuf;               // [rows][EMB] summed row gradients, indexed by representative position
    int32_t* hasdup;           // [rows] 1 if the representative's row occurs again in the batch (self-resetting)
    int32_t* last;             // [n_rows] Adam step up to which the row's (p, m, v) are current (lazy mode), or null
    int dx_off;                // 0 = user slice of dxe, EMB = item slice
    // DeepFM 1-d linear table of the same feature (null otherwise): gradient = scatter-add of dlogit
    float* lin_p;
    float* lin_m;
    float* lin_v;
    float* glin;               // [rows] summed dlogit, indexed by representative position
};
struct EmbStepArgs {
    float* p;                  // [user table | item table], contiguous at the head of the flat vector
    float* m;
    float* v;
    EmbTable t[2];             // user, item
    const float* dxe;          // [rows][dx_ld]
    int dx_ld;                 // 256, or 384 for the Star tower
    const float* dlogit;       // [rows]
    int rows;                  // batch rows
    float two_l2_lin;
    OptArgsLite opt;
    // lazy dense-Adam bookkeeping (emb_kernels.hip): alpha of every Adam step in a ring, current step
    const float* alpha_log;
    int log_mask;
    int t_now;
    int flags_done;            // duplicate flags were set by k_emb_catchup (lazy mode): skip k_emb_flag
    int apply_now;             // lazy mode: k_emb_reduce applies Adam step t_now to the rows it reduces
    // Star tower: dxe holds d loss / d NORMALISED input; PartitionedNorm's backward through the batch statistics,
    // dx = coef (( dxn - s1 / B) - xhat s2 / B), xhat = (x - mean) inv, is applied to every gathered gradient row on the
    // fly (x = the table row itself) -- k_star_pnb_apply's arithmetic without its pass over the batch.  null = dxe is d x
    const float* pn_sums;      // [2][384] column sums s1, s2 over the batch (k_star_pnb_final); null: dxe is d x
    const float* pn_means;     // [2][384] s1 / B, s2 / B (k_star_pnb_final forms the quotients once: the same IEEE division
                               // every consumer did per element)
    const float* pn;           // PartitionedNorm workspace [scale | shift | mean | inv | coef | ...] x 384
};
struct EmbRowsArgs {           // k_emb_rows: row ids + representatives of the batch BEFORE the tower runs
    const int32_t* uid;
    const int32_t* pid;
    const int32_t* perm;
    int64_t row_base, n_rows_split;
    int rows, rows_pad, n_user, n_item;
    int32_t* urow;
    int32_t* irow;
    int32_t* map_u;
    int32_t* map_i;
    float* alpha_log;
    int log_idx;
    float alpha;
};
void launch_emb_rows(const EmbRowsArgs& a, hipStream_t s);
// k_wgrad + k_emb_reduce (+ the NEXT step's k_emb_rows, into the alternate row / map buffers) in one launch;
// k_update (+ DeepFM's k_lin_sweep) (+ the NEXT step's k_emb_catchup) in one launch
struct StarPnBwdArgs;
void launch_wgrad_reduce(const WgradArgs& a, const EmbStepArgs& e, const EmbRowsArgs* next_rows, const StarPnBwdArgs* star_dm,
                         hipStream_t s);     // star_dm: also the Star tower's domain-row column sums (k_star_dm_final)
void launch_update_lin(const UpdateArgs& a, const EmbStepArgs& e, bool lin, const EmbStepArgs* next_catchup, hipStream_t s);
void launch_emb_catchup(const EmbStepArgs& a, hipStream_t s);     // rows of the batch -> current at t_now - 1
void launch_emb_flush(const EmbStepArgs& a, hipStream_t s);       // every row -> current at t_now
void launch_emb_reduce(const EmbStepArgs& a, hipStream_t s, int emb = EMB);     // emb: row width (generic-layer engine: 32 / 64 / 128 / 256)
void launch_emb_sweep(const EmbStepArgs& a, hipStream_t s, int emb = EMB);
void launch_lin_sweep(const EmbStepArgs& a, hipStream_t s);
void launch_emb_map_init(int32_t* map, int64_t n, hipStream_t s);

// star_kernels.hip: Star tower = PartitionedNorm + StarFCN (model_zoo/Star).  The step reuses
// k_tower / k_wgrad on an "effective" dense block (kernel_shared * kernel_specific[d], ...) built per step.
struct StarPrepArgs {
    const float* blk;          // Star block of the live weights
    StarLayout SL;
    DenseLayout L;             // layout of the effective block
    int n_domain, d;
    float* eff;                // effective dense block [L.alloc]
    float* pn;                 // [PN_WS_FLOATS]
    const float* part;         // training: [chunks][2][384] DOUBLES: sum x / sum x^2 of the raw input columns per chunk
    int n_chunks, rows;
    float* aux;                // moving statistics (read at eval, updated in training)
    StarAuxLayout AL;
    int train;
    int skip_eff;              // the effective block is current already (written by the previous step's k_star_update)
};
struct StarPnBwdArgs {
    const float* user_tab;
    const float* item_tab;
    const float* dm_row;       // domain table row d
    const int32_t* urow;       // [rows] (-1 = padding)
    const int32_t* irow;
    int rows, n_chunks;
    float* dxe;                // in: d loss / d normalised input [rows][384]; out: d loss / d raw input
    const float* pn;
    float* part;               // [chunks][2][384]
    float* sums;               // [2][384] s1 = sum dxn, s2 = sum dxn * xhat
    float* means;              // [2][384] s1 / B, s2 / B
    float* dmpart;             // [chunks][EMB] column sums of dx[:, 256:384]
    float* dmsum;              // [EMB] their total
    int fused;                 // 0: k_star_pnb_apply rewrites dxe, k_star_dm_final sums dmpart;
                               // 2 (the default inside a call, round 6): k_star_pnb_final is the only launch, the table
                               // rows get their d x inside k_emb_reduce, the domain columns' partials are formed by
                               // star_pnb_dom_body in k_wgrad_reduce and summed + stepped by star_dm_step_body in
                               // k_star_update_catchup -- k_star_pnb_apply's arithmetic and order, without its launch
};
struct StarUpdateArgs {
    float* p;                  // Star block of weights / Adam m / Adam v (or accumulator)
    float* m;
    float* v;
    StarLayout SL;
    DenseLayout L;
    int n_domain, d;
    const float* slabs;        // k_wgrad output on the effective layout
    int n_groups, slab_ld;
    const float* sums;         // PartitionedNorm [2][384]
    const float* dmsum;        // [EMB] gradient of the domain-table row d
    const float* xdom;         // [EMB] the batch's normalised domain row (k_star_prep)
    OptArgsLite opt;
    // lazy replay of the other domains' slices (Adam only): the launch covers slice d alone and logs the step's alpha
    int only_live;
    float* alpha_log;          // [log_mask + 1] alphas of this call's steps, slot = step index inside the call
    int log_idx;
    int dm_elsewhere;          // 1: the live domain row is stepped by star_dm_step_body in the same launch
    float* eff_out;            // nullable: the NEXT step's effective dense block (same domain) -- K_l = Ws_l * Wd_l[d],
                               // b_l = bs_l + bd_l[d], the output unit, row d of the domain table -- from the values
                               // just stepped (k_star_prep then skips that part)
};
// k_star_catchup: every slice but d_live takes the n_steps zero-gradient Adam steps it skipped (same arithmetic, same
// order: bit-identical to the per-step sweep)
struct StarCatchArgs {
    float* p;
    float* m;
    float* v;
    StarLayout SL;
    int n_domain, d_live;
    const float* alpha_log;
    int first_idx, n_steps, log_mask;
    float omb1, omb2, eps;
};
void launch_star_catchup(const StarCatchArgs& a, hipStream_t s);
void launch_star_stats(const TowerArgs& a, float* part, float* step_counter, hipStream_t s);
void launch_star_prep(const StarPrepArgs& a, hipStream_t s);
void launch_star_pn_bwd(const StarPnBwdArgs& a, bool dm_final, hipStream_t s);
void launch_star_update(const StarUpdateArgs& a, hipStream_t s);
// k_star_update + the NEXT step's k_emb_catchup in one launch (lazy table Adam)
void launch_star_update_catchup(const StarUpdateArgs& a, const EmbStepArgs& next_catchup, const StarPnBwdArgs* dm, hipStream_t s);

// outer_kernels.hip (compiled with -ffp-contract=off)
void launch_interp(float* dst, const float* a, const float* b, float scale, int64_t n, hipStream_t s);
void launch_moving_average(float* unbiased, float* biased, const float* value, float decay, float denom, int64_t n,
                           hipStream_t s);
void launch_merge(float* dst, const float* t, const float* p, int mode, int64_t n, hipStream_t s);
void launch_dr_advance(float* phi, float* w, float* merged, const float* theta, float gamma, int mode, int assign, int64_t n,
                       hipStream_t s);
void launch_dr_advance_dm(float* phi, float* w, float* merged, const float* theta, float gamma, int mode, int assign, int64_t n,
                          const DmStep& q, float* live_m, float* live_v, int64_t dm_off4, int dm_n4, hipStream_t s);
void launch_sub(float* dst, const float* a, const float* b, int64_t n, hipStream_t s);
void launch_accumulate(float* acc, const float* a, const float* b, const float* shared, float divisor, int64_t n,
                       hipStream_t s);
void launch_apply_accumulated(float* dst, float* acc, float divisor, float scale, int64_t n, hipStream_t s);
void launch_adam_apply(float* p, float* m, float* v, const float* g, float gscale, float alpha, float omb1, float omb2,
                       float eps, int64_t n, hipStream_t s);
// PCGrad projection (model_zoo/pcgrad.py:152-160) over tensors described as (offset, rows, cols) slices
constexpr int PCG_MAX_SEG = 24;
struct PcgArgs {
    float* fin;                // running gradient (= current gradient), updated in place
    float* aux;                // auxiliary gradient, projected in place
    int n_seg;
    int64_t off[PCG_MAX_SEG];
    int64_t row_start[PCG_MAX_SEG + 1];   // prefix sums of the row counts
    int cols[PCG_MAX_SEG];
};
void launch_pcgrad(const PcgArgs& a, hipStream_t s);

// recommend_kernels.hip: top-K retrieval (mamdr_recommend, mamdr_recommend_domain), exact ranks (mamdr_rank_domain) and per-query slates (mamdr_rank_slates).  One RecArgs describes a block of queries x a chunk of
// candidates; the query-side pointers (uid, dom, excl_off, the outputs) are already offset to the block's first query.
// (REC_TILE, REC_KMAX, REC_QBLOCK and SLATE_WAVE: host_base.h)
struct RecArgs {
    const float* user_tab;
    const float* item_tab;
    const float* dense;
    DenseLayout L;
    int n_user, n_item, n_domain;
    int mode;                  // 0 mlp, 1 deepfm (linear tables + FM term), 2 wdl (linear tables)
    const float* lin_user;     // null = frozen at their zero initialisation
    const float* lin_item;
    const int32_t* uid;        // [n_query]
    const int32_t* dom;
    int dom_all;               // -1: query q is in domain dom[q]; otherwise every query is in this domain and dom may be null
    const float* pn;           // Star: PartitionedNorm's workspace of domain dom_all (scale | shift | ... | xdom, k_star_prep
                               // with train = 0) and `dense` the effective block of that domain; null otherwise
    int n_query;
    const int32_t* cand;       // [n_cand], null: candidate at position p is item p
    int64_t n_cand, c_base;    // the chunk covers positions [c_base, c_base + n_chunk)
    int n_chunk;
    const int64_t* excl_off;   // nullable CSR: the ids excluded for query q are excl_ids[excl_off[q] .. excl_off[q + 1]), ascending
    const int32_t* excl_ids;
    int k, kt;                 // K; entries kept per tile = min(K, REC_TILE)
    int tiles, tiles_cap;      // tiles of this chunk / stride of `part` per query
    int first_chunk, last_chunk;
    // workspace (owned by the context)
    float* P;                  // [chunk][H1] item term of layer 0
    float* lin_i;              // [chunk] lin_item[cand] (wdl / deepfm)
    float* q0;                 // [REC_QBLOCK][H1] query term of layer 0 (+ b0)
    float* qud;                // [REC_QBLOCK][EMB] deepfm: u + d
    float* qs;                 // [REC_QBLOCK][2] u . d (deepfm) | lin_user + lin_domain
    unsigned long long* part;  // [REC_QBLOCK][tiles_cap][kt] per-tile lists, descending
    unsigned long long* best;  // [REC_QBLOCK][REC_KMAX] running best of the call
    // outputs
    int32_t* ids_out;          // [n_query][k]
    float* scores_out;
    float* scores_all;         // nullable [n_query][n_cand]
    // mamdr_rank_domain and mamdr_rank_slates (null / unused on the top-K path): positions j into the call's flat target list
    // (mamdr_rank_slates: the slates' entries are the targets; rank_out and live_out stay unused)
    const int64_t* tgt_off;    // [n_query + 1] CSR of the block's queries: query q owns targets [tgt_off[q], tgt_off[q + 1])
    unsigned long long* tkey;  // [n targets of the call] workspace: key(q, t), written by k_rec_pair, read by the counting tiles
    float* tscore_out;         // nullable [n targets]: sigmoid(logit(q, t))
    int32_t* rank_out;         // [n targets], zeroed by the call
    int32_t* live_out;         // [n_query] of the block, zeroed by the call
};
void launch_rec_item_proj(const RecArgs& a, hipStream_t s);
void launch_rec_query_proj(const RecArgs& a, hipStream_t s);
bool launch_rec_score(const RecArgs& a, hipStream_t s);        // false: its LDS limit was refused, nothing launched
void launch_rec_merge(const RecArgs& a, hipStream_t s);
// mamdr_rank_domain: the pair tiles over targets [c_base, c_base + n_chunk) (cand = the target ids, P / lin_i their item
// terms) and the counting ending of k_rec_score; false as launch_rec_score
bool launch_rec_pair(const RecArgs& a, hipStream_t s);
bool launch_rec_count(const RecArgs& a, hipStream_t s);
// mamdr_rank_slates: the order inside each slate of a block of queries, from the keys k_rec_pair left in `tkey`.  Offsets
// and positions j are the call's (absolute); `off` is already offset to the block's first query
constexpr int SLATE_TILE = 256;       // longer slates: entries per workgroup
constexpr int SLATE_STAGE = 1024;     // ... keys of the slate staged in LDS per round
struct SlateArgs {
    const int64_t* off;                 // [n_query + 1] slate q owns entries [off[q], off[q + 1])
    const unsigned long long* tkey;     // [entries of the call] key(q, x) of every entry
    int32_t* pos_out;                   // [entries of the call] keys of the same slate that are greater
    int32_t* order_out;                 // nullable [entries of the call], filled with -1 by the call: order[off[q] + pos[j]] = j - off[q]
    int n_query;
};
// max_len: the longest slate of the block; any_short: some slate has 1 .. SLATE_WAVE entries (both from the offsets the
// call read back): the launches a block does not need are left out.  The long form's grid is ceil(max_len / SLATE_TILE) x
// n_query: workgroups of shorter slates and behind a slate's end leave at once
void launch_slate_order(const SlateArgs& a, int64_t max_len, bool any_short, hipStream_t s);

// the order-preserving 32-bit key of a prediction, as mamdr_group_auc, mamdr_exact_metrics and mamdr_auc_bootstrap compare
// scores (gauc_kernels.hip, exact_kernels.hip): NaN -> 0, below everything and equal to NaN; -0 and +0 -> 0x80000000; every
// other value ordered as its float (-inf -> 0x007fffff, +inf -> 0xff800000)
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0u;
    if (s == 0.f) return 0x80000000u;
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// gauc_kernels.hip: per-user grouped AUC of one split's predictions (mamdr_group_auc)
constexpr int GAUC_SMALL = 64;        // groups of up to this many rows: one wave each (k_gauc_small)
constexpr int GAUC_TILE = 256;        // larger groups: positions per workgroup of k_gauc_tiles
struct GaucArgs {
    const float* pred;             // [n] in file order
    const float* label;            // [n]
    const int32_t* order;          // [n] row indices, grouped
    const int64_t* group_off;      // [n_groups + 1] into order
    const int32_t* tile_group;     // [n_tiles]
    const int64_t* tile_first;     // [n_tiles] first position (into order) of the tile
    int64_t n, n_groups, n_tiles;
    unsigned long long* T;         // [n_groups], zeroed by the call
    uint32_t* P;                   // [n_groups], zeroed by the call
    double* part_num;              // [n_parts] partial sums of k_gauc_terms' blocks
    unsigned long long* part_rows;
    unsigned long long* part_valid;
    int64_t n_parts;
    double* result;                // [4] num, rows_valid, n_valid, n_groups
};
int64_t gauc_parts(int64_t n_groups);
void launch_gauc(const GaucArgs& a, hipStream_t s);

// exact_kernels.hip: exact AUC, average precision and equal-mass calibration bins of one split (mamdr_exact_metrics).
// (mamdr_amd/exact.py carries the same four tile constants for the tests)
constexpr int EXACT_RADIX_BITS = 8;           // digit width of the sort: 5 passes over the 33-bit composites
constexpr int EXACT_SORT_TILE = 2048;         // composites per workgroup of k_exact_hist / k_exact_scatter
constexpr int EXACT_SCAN_TILE = 512;          // elements per workgroup of the device-wide scans
constexpr int EXACT_METRIC_TILE = 1024;       // sorted positions per workgroup of k_exact_runs / k_exact_metrics
constexpr int EXACT_MAX_BINS = 4096;          // (= MAMDR_EXACT_MAX_BINS)
struct ExactArgs {
    const float* pred;                 // [n] in file order
    const float* label;                // [n]
    int64_t n;
    int n_bins;
    unsigned long long* counts;        // [5] T, P, N, n_runs, n_nan; zeroed by the call
    double* ap;                        // [1]
    unsigned long long* bins;          // [3][n_bins] rows, positives, Q32 prediction sums; zeroed by the call
    unsigned long long* sorted_out;    // nullable [n]: the last pass scatters here
    char* ws;                          // exact_workspace_bytes(n) bytes, 16-byte aligned
};
size_t exact_workspace_bytes(int64_t n);
void launch_exact(const ExactArgs& a, hipStream_t s);      // n > 0
// the chain's radix sort on its own (launch_exact's first phase; bootstrap_kernels.hip sorts its wider word with it)
struct ExactSortArgs {
    const float* pred;                 // [n] in file order
    const float* label;                // [n]
    int64_t n;
    int rows;                          // 0: the composites key << 1 | positive, sorted on bits 0 .. 32;
                                       // 1: the words key << 32 | positive << 31 | row (n <= 2^31), sorted on bits 31 .. 63
    unsigned long long* sorted_out;    // nullable [n]: the last pass scatters here
    char* ws;                          // exact_sort_workspace_bytes(n) bytes, 16-byte aligned (the head of launch_exact's)
};
size_t exact_sort_workspace_bytes(int64_t n);
const unsigned long long* launch_exact_sort(const ExactSortArgs& a, hipStream_t s);      // n > 0 -> the sorted array

// bootstrap_kernels.hip: Poisson-bootstrap replicates of the exact AUC's integers (mamdr_auc_bootstrap).
// (mamdr_amd/bootstrap.py carries the same constants for the tests)
constexpr int BOOT_TILE = 1024;               // sorted positions per wave: 16 consecutive ones per lane, in registers
constexpr int BOOT_GROUP = 16;                // replicates per workgroup: 4 waves x 4 replicates in turn
constexpr int64_t BOOT_PART_WORDS = 1 << 24;  // 32-bit words of per-(tile, replicate) partials at a time (64 MiB): more
                                              // replicates than fit run in chunks
struct BootArgs {
    const float* pred;                 // [n] in file order
    const float* label;                // [n]
    const int32_t* unit;               // nullable [n]: the resampling unit of a row; null = the row itself
    int64_t n;
    int n_rep;
    uint64_t seed;
    unsigned long long* T;             // [n_rep + 1], zeroed by the call
    long long* P;                      // [n_rep + 1]
    long long* N;                      // [n_rep + 1]
    int64_t part_words;                // BOOT_PART_WORDS, or a test's smaller bound
    char* ws;                          // boot_workspace_bytes(n, n_rep, part_words) bytes, 16-byte aligned
};
int boot_chunk(int64_t n, int n_rep, int64_t part_words);       // replicate slots per chunk, a multiple of BOOT_GROUP
size_t boot_workspace_bytes(int64_t n, int n_rep, int64_t part_words);
void launch_boot(const BootArgs& a, hipStream_t s);        // n > 0

// isotonic_kernels.hip: the isotonic (PAV) fit of one split, its application and the Brier / log-loss sums
// (mamdr_isotonic_fit(_bounded), mamdr_isotonic_apply, mamdr_score_sums).
// (mamdr_amd/isotonic.py carries the same constants for the tests)
constexpr int ISO_POINT_TILE = 1024;          // sorted positions per workgroup of k_iso_run_sums / k_iso_points
constexpr int ISO_SCAN_TILE = 1024;           // 64-bit words per workgroup of the device-wide scans
constexpr int ISO_HULL_TILE = 64;             // points per tile of the hull's levels (one thread each): mamdr_isotonic_fit's
constexpr int ISO_MIN_TILE = 4;               // smallest tile_points of mamdr_isotonic_fit_bounded (= MAMDR_ISOTONIC_MIN_TILE)
constexpr int ISO_MAX_LEVELS = 32;            // levels of the hull at most (a tile of 4 halves 2^31 points 30 times)
constexpr int ISO_APPLY_TILE = 2048;          // rows per workgroup of k_iso_apply
constexpr int ISO_APPLY_LDS = 4096;           // blocks up to which k_iso_apply searches first_key in LDS
constexpr int ISO_SCORE_TILE = 1024;          // rows per workgroup of k_score_parts
struct IsoFitArgs {
    const float* pred;                 // [n] in file order
    const float* label;                // [n]
    int64_t n;
    int tile;                          // points per tile of the hull's levels, >= ISO_MIN_TILE
    long long* counts;                 // [4] n_blocks, n_runs, n_nan, P; zeroed by the call
    uint32_t* first_key;               // [n] capacity; n_blocks entries are written
    long long* rows;
    long long* positives;
    char* ws;                          // iso_fit_workspace_bytes(n, tile) bytes, 16-byte aligned
};
int iso_levels(int64_t n, int tile);                       // levels of tiles before the final chain
size_t iso_fit_workspace_bytes(int64_t n, int tile);
void launch_iso_fit(const IsoFitArgs& a, hipStream_t s);   // n > 0
struct IsoApplyArgs {
    const uint32_t* first_key;         // [n_blocks] ascending
    const long long* rows;
    const long long* positives;
    int64_t n_blocks;                  // > 0
    const float* pred;                 // [n]
    int64_t n;
    float* out;                        // [n]
};
void launch_iso_apply(const IsoApplyArgs& a, hipStream_t s);        // n > 0
struct ScoreArgs {
    const float* pred;                 // [n]
    const float* label;                // [n]
    int64_t n;
    double* part;                      // score_workspace_bytes(n): [tiles][2]
    double* out;                       // [2] Brier sum, log-loss sum
};
size_t score_workspace_bytes(int64_t n);
void launch_score_sums(const ScoreArgs& a, hipStream_t s);          // n > 0

// gram_kernels.hip: fp64 Gram matrices of up to GRAM_MAX_VEC flat vectors over column ranges (mamdr_gram).  One GramArgs
// describes a batch of up to GRAM_MAX_RANGES ranges: two launches
constexpr int GRAM_SLAB = 16384;      // columns per workgroup of k_gram_slab (= MAMDR_GRAM_SLAB)
constexpr int GRAM_MAX_VEC = 32;
constexpr int GRAM_MAX_RANGES = 64;
struct GramArgs {
    const float* vecs;             // vector i = vecs + i * stride
    int64_t stride;
    int n_vec, n_range;            // ranges of this batch
    int64_t off[GRAM_MAX_RANGES], count[GRAM_MAX_RANGES];
    int64_t first[GRAM_MAX_RANGES + 1];    // slabs of the batch before range r; first[n_range] = all of them
    double* work;                  // [slabs of the call][n_vec][n_vec]
    int64_t work_first;            // slabs of the call before this batch
    double* out;                   // [ranges of the call][n_vec][n_vec]
    int64_t out_first;             // ranges of the call before this batch
};
void launch_gram(const GramArgs& a, hipStream_t s);

// list_kernels.hip: what top-K lists are made of (mamdr_id_counts, mamdr_list_similarity)
constexpr int LIST_SIM_MAX_K = 128;   // = MAMDR_LIST_MAX_K
struct IdCountArgs {
    const int32_t* ids;            // [n]
    const float* label;            // [n] or null: every position counts
    int64_t n, n_bins;
    uint32_t* counts;              // [n_bins], zeroed on the stream before the launch
};
void launch_id_counts(const IdCountArgs& a, hipStream_t s);         // n > 0
struct ListSimArgs {
    const int32_t* ids;            // [n_list][k]
    int n_list, k;
    const float* rows;             // [n_rows][emb_dim], 16-byte aligned
    int64_t n_rows;
    int emb_dim;                   // 32, 64, 128 or 256
    double* sim_sum;               // [n_list]
    int32_t* pairs;                // [n_list]
};
void launch_list_sim(const ListSimArgs& a, hipStream_t s);          // n_list > 0

// diversify_kernels.hip: greedy MMR re-ranking of candidate lists (mamdr_list_diversify)
struct ListDivArgs {
    const int32_t* ids;            // [n_list][n]
    const float* rel;              // [n_list][n]
    int n_list, n, k;              // 1 <= k <= n <= LIST_SIM_MAX_K
    float lambda;                  // in [0, 1]
    const float* rows;             // [n_rows][emb_dim], 16-byte aligned
    int64_t n_rows;
    int emb_dim;                   // 32, 64, 128 or 256
    int32_t* pos_out;              // [n_list][k]
    float* value_out;              // [n_list][k] or null
};
void launch_list_div(const ListDivArgs& a, hipStream_t s);          // n_list > 0

// knn_kernels.hip: exact cosine nearest neighbours of table rows (mamdr_row_neighbours)
constexpr int KNN_MAX_K = 128;        // = MAMDR_KNN_MAX_K: entries of a running list
constexpr int KNN_QBLOCK = 64;        // queries of a workgroup
constexpr int KNN_TILE = 64;          // candidates of a tile
struct KnnArgs {
    const float* rows;             // [n_rows][emb_dim], 16-byte aligned
    int64_t n_rows;
    int emb_dim;                   // 32, 64, 128 or 256
    const int32_t* query;          // [n_query]
    int n_query;
    const int32_t* cand;           // [n_cand] or null: candidate p is row p
    int64_t c_base;                // candidates of the call before this pass
    int n_chunk;                   // candidates of this pass
    int exclude_self, k;
    float* qn2;                    // [n_query] squared norms of the query rows (0 for an id out of range)
    float* cn2;                    // [n_chunk] squared norms of the pass's candidate rows
    unsigned long long* best;      // [n_query rounded up to KNN_QBLOCK][splits][KNN_MAX_K] running lists, sorted descending
    int splits;                    // gridDim.y of the tile kernel: the same in every pass of a call
    int first_chunk;               // the running lists start empty
    int32_t* ids_out;              // [n_query][k]
    float* sim_out;                // [n_query][k]
};
void launch_knn_query_norms(const KnnArgs& a, hipStream_t s);       // qn2 of all queries
void launch_knn_cand_norms(const KnnArgs& a, hipStream_t s);        // cn2 of the pass
bool launch_knn_tile(const KnnArgs& a, hipStream_t s);              // -> false: the LDS was refused, nothing was launched
void launch_knn_merge(const KnnArgs& a, hipStream_t s);             // the splits' lists -> the outputs

// baseline_kernels.hip: item co-occurrence, ItemKNN scores of user histories, ranks and top-K lists from a caller's score
// matrix (mamdr_item_cooc, mamdr_history_scores, mamdr_rank_scores, mamdr_topk_scores)
constexpr int BASE_MAX_ITEMS = 65535;   // m of the co-occurrence matrix: m * m * 4 bytes stays below 2^34
constexpr int BASE_MAX_K = 128;         // = MAMDR_SCORES_MAX_K
struct HistArgs {
    const int64_t* hist_off;       // [n_user + 1], clamped into [0, nnz] by every reader
    const int32_t* hist_pos;       // [nnz] catalogue positions; one outside [0, m) is skipped
    int64_t nnz;
    int n_user, m;
    uint32_t* cooc;                // [m][m]; k_item_cooc adds into it (zeroed on the stream before), k_hist_scores reads it
    const int32_t* query;          // [n_query] user indices, one outside [0, n_user) scores all +0.0f
    int n_query;
    float shrink;
    float* root;                   // [m] sqrtf(float(cooc[a][a])): the call's own scratch
    float* scores;                 // [n_query][m]
    int vec4;                      // rows of cooc / scores are 16-byte aligned: four columns per lane
};
void launch_item_cooc(const HistArgs& a, hipStream_t s);            // n_user > 0
void launch_hist_scores(const HistArgs& a, hipStream_t s);          // the roots, then the scores; n_query > 0
struct ScoreRankArgs {
    const float* scores;           // candidate position p of query q: scores[q * row_stride + p]
    int64_t row_stride;            // 0: one row serves every query
    int n_query;
    const int32_t* cand;           // [n_cand] ascending distinct ids, or null: the id of position p is p
    int n_cand;
    const int64_t* excl_off;       // [n_query + 1] or null
    const int32_t* excl_ids;
    const int64_t* tgt_off;        // [n_query + 1], clamped into [0, n_tgt]
    const int32_t* tgt_ids;
    int64_t n_tgt;
    int32_t* rank_out;             // [n_tgt], zeroed on the stream before the launch
    float* score_out;              // [n_tgt] or null
    int32_t* live_out;             // [n_query], zeroed on the stream before the launch
    int k;                         // top-K only
    int32_t* ids_out;              // [n_query][k]
    float* topk_out;               // [n_query][k]
};
void launch_rank_scores(const ScoreRankArgs& a, hipStream_t s);     // n_query > 0, n_cand > 0
void launch_topk_scores(const ScoreRankArgs& a, hipStream_t s);     // n_query > 0, n_cand > 0, 1 <= k <= BASE_MAX_K

}  // namespace mamdr
