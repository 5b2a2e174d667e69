// Top-K item retrieval from a trained mlp / wdl / deepfm tower (mamdr_recommend) and, one domain per call, from those and
// the Star tower (mamdr_recommend_domain; include/mamdr_hip.h).  No reference counterpart: the reference's pipeline ends at
// per-domain loss and AUC.
//
// The tower's first layer separates by field,
//     z0 = (u . W0[0:128] + d . W0[256:384] + b0) + i . W0[128:256],
// so the query term is formed once per query (k_rec_query_proj), the item term once per candidate and call
// (k_rec_item_proj, shared by every query), and only layers 1 and 2 (256 -> 128 -> 64) and the head remain per
// (query, candidate) pair (k_rec_score): 2 (256 x 128 + 128 x 64 + 64) = 82,048 flop per pair instead of the full tower's
// 360,576, and no [u | i | d] row is ever materialised.  One launch per phase: the kernel boundary is the hand-off.
//
// Star (RecArgs::pn set, one domain d per call): in inference PartitionedNorm is the per-column affine
// xn = x * scale_d + shift_d and layer 0 a plain matmul with K0_d = Ws0 * Wd0[d], b0_d = bs0 + bd0[d], so the same split
// holds on the normalised rows with the effective dense block k_star_prep (train = 0) wrote: the affine is applied where
// a row is staged, with the tower gather's separately rounded multiply and add, and everything behind is unchanged.
//
// Determinism: every contraction has ONE reduction order per output element -- k ascending inside the MFMA chains, fixed
// shuffle trees elsewhere -- and no operand depends on where a pair sits in the grid: a pair's logit is the same bits in a
// full tile and in the remainder tile, under any chunking, beside any other query.
//
// Ranking: one 64-bit key per pair, (order-preserving bits of the logit << 32) | ~id: descending key order = descending
// logit, equal logits by ascending item id, a NaN logit behind every number; key 0 = no entry (excluded pair, padding).
// Keys of distinct ids are distinct, so the top K of a query is one well-defined list whatever the tiles and chunks.
//
// Exact ranks (mamdr_rank_domain): the same phases with a counting ending.  The targets' keys first -- their item term
// (k_rec_item_proj over the flat target list), then k_rec_pair, 64 (query, target) pairs per workgroup through the layers
// and the head of the scoring tile, so a target's key is the bits the grid computes for the same pair --, then
// k_rec_score<REC_EPI_COUNT>: a tile counts its keys above each target key of its query by ballot + popcount and adds the
// count with one integer atomic.  No sort, no merge; integers only, so the sums do not depend on the tiles' order.
#include "mamdr_kernels.h"
#include "rec_device.h"

namespace mamdr {
namespace {

constexpr int REC_THREADS = 256;
constexpr int IP_ROWS = 32;                   // candidates per workgroup of k_rec_item_proj
constexpr int XS_LD = EMB + 4;                // LDS row strides: 4 floats of padding keep the 16-B operand reads of 16
constexpr int H0_LD = H1 + 4;                 // consecutive rows on disjoint banks
constexpr int H1_LD = H2 + 4;
constexpr int H2_LD = H3 + 4;
// k_rec_score's LDS (floats): h0 [64][260]; behind the barrier that ends layer 1, h1 [64][132] and h2 [64][68] reuse it
constexpr int SC_H1_OFF = 0;
constexpr int SC_H2_OFF = REC_TILE * H1_LD;                   // 8,448
constexpr int SC_KEY_OFF = SC_H2_OFF + REC_TILE * H2_LD;      // 12,800: 64 keys (8-byte aligned)
constexpr int SC_UD_OFF = REC_TILE * H0_LD;                   // 16,640: deepfm's u + d of the query
constexpr int SC_FLOATS = SC_UD_OFF + EMB;
static_assert(SC_KEY_OFF + 2 * REC_TILE <= SC_UD_OFF && (SC_KEY_OFF % 2) == 0, "keys inside the h0 region");

__device__ __forceinline__ int rec_cand_id(const RecArgs& a, int pos) {      // pos < n_chunk
    const int id = a.cand ? a.cand[a.c_base + pos] : (int)(a.c_base + pos);
    return clampi(id, 0, a.n_item - 1);
}

// ---- P[c, 0:256] = I[cand[c]] . W0[128:256, :] for the chunk's candidates: 32 gathered rows per workgroup in LDS, wave w
// owns columns [64 w, 64 w + 64) as two 32 x 32 x 2 fp32 MFMA chains over k = 0 .. 127
__global__ __launch_bounds__(REC_THREADS) void k_rec_item_proj(const RecArgs a) {
    __shared__ float xs[IP_ROWS * XS_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * IP_ROWS;
    // Star: the item columns' affine of PartitionedNorm; a thread stages one column quad (tid & 31) of every row it touches
    f32x4 sc = (f32x4){1.f, 1.f, 1.f, 1.f}, sh = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.pn) {
        sc = *reinterpret_cast<const f32x4*>(a.pn + EMB + 4 * (tid & 31));
        sh = *reinterpret_cast<const f32x4*>(a.pn + XDIM + EMB + 4 * (tid & 31));
    }
#pragma unroll
    for (int t = 0; t < IP_ROWS * (EMB / 4) / REC_THREADS; ++t) {
        const int e = tid + REC_THREADS * t, r = e >> 5, c4 = e & 31, pos = r0 + r;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (pos < a.n_chunk) {
            v = *reinterpret_cast<const f32x4*>(a.item_tab + (size_t)rec_cand_id(a, pos) * EMB + 4 * c4);
            if (a.pn) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = __fadd_rn(__fmul_rn(v[k], sc[k]), sh[k]);
            }
        }
        *reinterpret_cast<f32x4*>(xs + r * XS_LD + 4 * c4) = v;
    }
    if (a.mode != 0 && tid < IP_ROWS && r0 + tid < a.n_chunk)
        a.lin_i[r0 + tid] = a.lin_item ? a.lin_item[rec_cand_id(a, r0 + tid)] : 0.f;
    __syncthreads();
    const float* __restrict__ W = a.dense + a.L.w0 + EMB * H1;
    const int c = lane & 31, h = lane >> 5;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    // the MFMA's two k slots carry k = 8 g + j and 8 g + 4 + j (j = 0 .. 3): one 16-B LDS read feeds four MFMAs
#pragma unroll 4
    for (int g = 0; g < EMB / 8; ++g) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(xs + c * XS_LD + 8 * g + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* wr = W + (size_t)(8 * g + 4 * h + j) * H1 + 64 * w + c;
            acc0 = MAMDR_MFMA32(av[j], wr[0], acc0);
            acc1 = MAMDR_MFMA32(av[j], wr[32], acc1);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int pos = r0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (pos < a.n_chunk) {
            a.P[(size_t)pos * H1 + 64 * w + c] = acc0[r];
            a.P[(size_t)pos * H1 + 64 * w + 32 + c] = acc1[r];
        }
    }
}

// ---- q0[q, 0:256] = U[uid] . W0[0:128] + Dm[dom] . W0[256:384] + b0, one workgroup per query, thread n owns column n (one
// fma chain, k ascending); deepfm: u + d and u . d; wdl / deepfm: lin_user[uid] + lin_domain[dom].  Star: the user row takes
// PartitionedNorm's affine of columns [0, 128) and the domain part is the normalised domain row k_star_prep left behind
__global__ __launch_bounds__(REC_THREADS) void k_rec_query_proj(const RecArgs a) {
    __shared__ float us[EMB], ds[EMB], red[2];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int uid = clampi(a.uid[q], 0, a.n_user - 1), dom = clampi(a.dom_all >= 0 ? a.dom_all : a.dom[q], 0, a.n_domain - 1);
    if (tid < EMB) {
        float x = a.user_tab[(size_t)uid * EMB + tid];
        if (a.pn) x = __fadd_rn(__fmul_rn(x, a.pn[tid]), a.pn[XDIM + tid]);
        us[tid] = x;
    } else {
        ds[tid - EMB] = a.pn ? a.pn[PN_XDOM_OFF + tid - EMB] : a.dense[a.L.dm + dom * EMB + tid - EMB];
    }
    __syncthreads();
    const float* __restrict__ W0 = a.dense + a.L.w0;
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < EMB; ++k) acc = fmaf(us[k], W0[(size_t)k * H1 + tid], acc);
#pragma unroll 8
    for (int k = 0; k < EMB; ++k) acc = fmaf(ds[k], W0[(size_t)(2 * EMB + k) * H1 + tid], acc);
    a.q0[(size_t)q * H1 + tid] = acc + a.dense[a.L.b0 + tid];
    if (a.mode == 1) {
        float p = 0.f;
        if (tid < EMB) {
            a.qud[(size_t)q * EMB + tid] = us[tid] + ds[tid];
            p = us[tid] * ds[tid];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) p += __shfl_xor(p, m);
        if (tid < EMB && (tid & 63) == 0) red[tid >> 6] = p;
        __syncthreads();
    }
    if (tid == 0) {
        a.qs[2 * q] = a.mode == 1 ? red[0] + red[1] : 0.f;
        a.qs[2 * q + 1] = a.mode != 0 ? (a.lin_user ? a.lin_user[uid] : 0.f) + a.dense[a.L.ld + dom] : 0.f;
    }
}

// ---- layers 1 and 2 of a 64-row tile whose h0 [64][260] the caller has staged in LDS (entered before the barrier that
// publishes h0, left behind the barrier that publishes h2 [64][68]): fp32 MFMA with bias + relu between them.  Layer 1:
// wave w owns columns [32 w, 32 w + 32) of both 32-row halves (each weight element fetched once per tile); layer 2: wave w
// owns the 32 x 32 quadrant (w >> 1, w & 1).  Rows never meet: a row's h2 depends on its own h0 and the weights only, so
// the grid tile (k_rec_score) and the pair tile (k_rec_pair) give one pair the same bits.
__device__ __forceinline__ void rec_layers12(const RecArgs& a, float* smem, int tid) {
    const float* __restrict__ dense = a.dense;
    const int lane = tid & 63, w = tid >> 6;
    __syncthreads();
    const int c = lane & 31, h = lane >> 5;
    {
        const float* __restrict__ W1 = dense + a.L.w1;
        f32x16 acc0, acc1;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
#pragma unroll 4
        for (int g = 0; g < H1 / 8; ++g) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(smem + c * H0_LD + 8 * g + 4 * h);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(smem + (32 + c) * H0_LD + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = W1[(size_t)(8 * g + 4 * h + j) * H2 + 32 * w + c];
                acc0 = MAMDR_MFMA32(a0[j], b, acc0);
                acc1 = MAMDR_MFMA32(a1[j], b, acc1);
            }
        }
        const float bias = dense[a.L.b1 + 32 * w + c];
        __syncthreads();                          // every wave is done with h0: h1 takes its place
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            smem[SC_H1_OFF + row * H1_LD + 32 * w + c] = fmaxf(acc0[r] + bias, 0.f);
            smem[SC_H1_OFF + (32 + row) * H1_LD + 32 * w + c] = fmaxf(acc1[r] + bias, 0.f);
        }
    }
    __syncthreads();
    {
        const float* __restrict__ W2 = dense + a.L.w2;
        const int rb = w >> 1, cb = w & 1;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 4
        for (int g = 0; g < H2 / 8; ++g) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(smem + SC_H1_OFF + (32 * rb + c) * H1_LD + 8 * g + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = MAMDR_MFMA32(av[j], W2[(size_t)(8 * g + 4 * h + j) * H3 + 32 * cb + c], acc);
        }
        const float bias = dense[a.L.b2 + 32 * cb + c];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * h;
            smem[SC_H2_OFF + row * H2_LD + 32 * cb + c] = fmaxf(acc[r] + bias, 0.f);
        }
    }
    __syncthreads();
}

// ---- the head of one pair (tile row `row`, item `id`, position `pos` of the chunk when `in`) of query q: four lanes per
// pair (part = 0 .. 3), 16 hidden units (and 32 elements of deepfm's i . (u + d)) each, a two-step xor tree; then wo, gb
// and the wdl / deepfm extras.  `ud` is the query's u + d -- the tile's LDS copy or a.qud's row: the same values, the same
// fma order.  Every lane of the four returns the logit
__device__ __forceinline__ float rec_head(const RecArgs& a, const float* smem, int row, int part, bool in, int id, int pos,
                                          int q, const float* ud) {
    const float* __restrict__ dense = a.dense;
    const float* wo = dense + a.L.wo + 16 * part;
    const float* hr = smem + SC_H2_OFF + row * H2_LD + 16 * part;
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < 16; ++n) s = fmaf(hr[n], wo[n], s);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    float logit = s + dense[a.L.gb];
    if (a.mode != 0) {
        float fm = 0.f;
        if (a.mode == 1) {
            const float* ir = a.item_tab + (size_t)id * EMB + 32 * part;
            ud += 32 * part;
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const f32x4 iv = *reinterpret_cast<const f32x4*>(ir + 4 * k4);
#pragma unroll
                for (int e = 0; e < 4; ++e) fm = fmaf(iv[e], ud[4 * k4 + e], fm);
            }
            fm += __shfl_xor(fm, 1);
            fm += __shfl_xor(fm, 2);
            fm += a.qs[2 * q];
        }
        const float lin = a.qs[2 * q + 1] + (in ? a.lin_i[pos] : 0.f);
        logit += fm + lin;
    }
    logit += 0.f;                                 // -0 -> +0: equal logits are equal keys
    return logit;
}

// ---- one (query, 64 candidates) tile: h0 = relu(q0[q] + P[c]) staged in LDS, layers 1 and 2 (rec_layers12), the head
// (rec_head), the optional dense score matrix, the tile's 64 keys in LDS (0 = excluded pair or padding) and one of two
// endings.  REC_EPI_TOPK: the tile's partial top-K (mamdr_recommend, mamdr_recommend_domain).  REC_EPI_COUNT
// (mamdr_rank_domain): lane l of every wave holds key l; wave w takes the query's targets tgt_off[q] + w, + 4, ... and adds
// popcount(ballot(key_l > tkey[j])) to rank_out[j]; wave 0 adds the tile's live candidates to live_out[q].  Integer atomics
// only: the sums are the same whatever the order the tiles arrive in.
enum { REC_EPI_TOPK = 0, REC_EPI_COUNT = 1 };
template <int EPI>
__global__ __launch_bounds__(REC_THREADS) void k_rec_score(const RecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tile = blockIdx.x, q = blockIdx.y;
    const int p0 = tile * REC_TILE;
    {
        const int c4 = tid & 63;
        const f32x4 qv = *reinterpret_cast<const f32x4*>(a.q0 + (size_t)q * H1 + 4 * c4);
#pragma unroll 4
        for (int t = 0; t < REC_TILE * (H1 / 4) / REC_THREADS; ++t) {
            const int r = (tid >> 6) + 4 * t, pos = p0 + r;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (pos < a.n_chunk) {
                const f32x4 pv = *reinterpret_cast<const f32x4*>(a.P + (size_t)pos * H1 + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(qv[e] + pv[e], 0.f);
            }
            *reinterpret_cast<f32x4*>(smem + r * H0_LD + 4 * c4) = v;
        }
        if (a.mode == 1 && tid < EMB) smem[SC_UD_OFF + tid] = a.qud[(size_t)q * EMB + tid];
    }
    rec_layers12(a, smem, tid);
    u64* keys = reinterpret_cast<u64*>(smem + SC_KEY_OFF);
    {
        const int row = tid >> 2, part = tid & 3, pos = p0 + row;
        const bool in = pos < a.n_chunk;
        const int id = in ? rec_cand_id(a, pos) : 0;
        const float logit = rec_head(a, smem, row, part, in, id, pos, q, smem + SC_UD_OFF);
        if (part == 0) {
            bool valid = in;
            if (valid && a.excl_off) {            // the query's excluded ids, ascending
                int64_t lo = a.excl_off[q], hi = a.excl_off[q + 1];
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (a.excl_ids[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < a.excl_off[q + 1] && a.excl_ids[lo] == id) valid = false;
            }
            if (in && a.scores_all) a.scores_all[(size_t)q * a.n_cand + a.c_base + pos] = valid ? rec_sigmoid(logit) : 0.f;
            keys[row] = valid ? rec_key(logit, id) : 0ull;
        }
    }
    __syncthreads();
    if (EPI == REC_EPI_TOPK) {
        if (w == 0) {
            const u64 key = rec_wave_sort(keys[lane], lane);
            if (lane < a.kt) a.part[((size_t)q * a.tiles_cap + tile) * a.kt + lane] = key;
        }
    } else {
        const u64 key = keys[lane];
        if (w == 0) {
            const int live = __popcll(__ballot(key != 0ull));
            if (lane == 0 && live) atomicAdd(a.live_out + q, live);
        }
        const int64_t t1 = a.tgt_off[q + 1];
        for (int64_t j = a.tgt_off[q] + w; j < t1; j += REC_THREADS / 64) {
            const int cnt = __popcll(__ballot(key > a.tkey[j]));      // (a key of 0 is above no target: tkey >= 1 << 32)
            if (lane == 0 && cnt) atomicAdd(a.rank_out + j, cnt);
        }
    }
}

// ---- the pair form of the scoring tile (mamdr_rank_domain's target pre-pass): 64 consecutive positions of the flat target
// list per workgroup, row r = target j = c_base + p0 + r of the query that a binary search of j in tgt_off finds (queries
// without targets are stepped over).  h0 = relu(q0[q_r] + P[r]) with P the targets' item term (k_rec_item_proj over
// cand = tgt_ids), then rec_layers12 and rec_head as the grid tile runs them: tkey[j] is the key the grid computes for the
// pair (q_r, tgt_ids[j]), whether or not the item is a candidate or excluded; score_out[j] = sigmoid of the same logit.
__global__ __launch_bounds__(REC_THREADS) void k_rec_pair(const RecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* rowq = reinterpret_cast<int*>(smem + SC_UD_OFF);          // [64] the rows' queries (the u + d slot is free here)
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * REC_TILE;
    if (tid < REC_TILE) {
        int lo = 0;
        if (p0 + tid < a.n_chunk) {
            const int64_t j = a.c_base + p0 + tid;
            int hi = a.n_query - 1;                                // first q with tgt_off[q + 1] > j
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a.tgt_off[mid + 1] <= j) lo = mid + 1; else hi = mid;
            }
        }
        rowq[tid] = lo;
    }
    __syncthreads();
    {
        const int c4 = tid & 63;
#pragma unroll 4
        for (int t = 0; t < REC_TILE * (H1 / 4) / REC_THREADS; ++t) {
            const int r = (tid >> 6) + 4 * t, pos = p0 + r;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (pos < a.n_chunk) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(a.q0 + (size_t)rowq[r] * H1 + 4 * c4);
                const f32x4 pv = *reinterpret_cast<const f32x4*>(a.P + (size_t)pos * H1 + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(qv[e] + pv[e], 0.f);
            }
            *reinterpret_cast<f32x4*>(smem + r * H0_LD + 4 * c4) = v;
        }
    }
    const int row = tid >> 2, part = tid & 3, pos = p0 + row;
    const int q = rowq[row];                                       // (read before layer 1's barriers; nothing overwrites it)
    rec_layers12(a, smem, tid);
    const bool in = pos < a.n_chunk;
    const int id = in ? rec_cand_id(a, pos) : 0;
    const float logit = rec_head(a, smem, row, part, in, id, pos, q, a.qud + (size_t)q * EMB);
    if (part == 0 && in) {
        a.tkey[a.c_base + pos] = rec_key(logit, id);
        if (a.tscore_out) a.tscore_out[a.c_base + pos] = rec_sigmoid(logit);
    }
}

// ---- one workgroup per query: the chunk's per-tile lists merged into the query's running best 128 (kept across the
// chunks of a call), 128 keys per round through a 256-key bitonic sort in LDS; a round none of whose keys beats the
// current K-th is skipped.  The last chunk writes the call's outputs.
__global__ __launch_bounds__(REC_THREADS) void k_rec_merge(const RecArgs a) {
    __shared__ u64 buf[2 * REC_KMAX];
    const int t = threadIdx.x, q = blockIdx.x;
    u64* best = a.best + (size_t)q * REC_KMAX;
    buf[t] = (t < REC_KMAX && !a.first_chunk) ? best[t] : 0ull;
    __syncthreads();
    const u64* list = a.part + (size_t)q * a.tiles_cap * a.kt;
    const int n = a.tiles * a.kt;
    for (int base = 0; base < n; base += REC_KMAX) {
        const u64 key = (t < REC_KMAX && base + t < n) ? list[base + t] : 0ull;
        const u64 kth = buf[a.k - 1];
        if (!__syncthreads_or(key > kth)) continue;
        if (t < REC_KMAX) buf[REC_KMAX + t] = key;
        __syncthreads();
        for (int k = 2; k <= 2 * REC_KMAX; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int o = t ^ j;
                if (o > t) {
                    const u64 x = buf[t], y = buf[o];
                    if (((t & k) == 0) ? x < y : x > y) {
                        buf[t] = y;
                        buf[o] = x;
                    }
                }
                __syncthreads();
            }
        }
    }
    if (t < REC_KMAX) best[t] = buf[t];
    if (a.last_chunk && t < a.k) {
        const u64 key = buf[t];
        a.ids_out[(size_t)q * a.k + t] = key ? (int32_t)~(uint32_t)key : -1;
        a.scores_out[(size_t)q * a.k + t] = key ? rec_sigmoid(rec_key_logit(key)) : 0.f;
    }
}

// ---- the order inside each slate (mamdr_rank_slates): pos[j] = the keys of j's slate that are greater than key j, and,
// when asked for, the inverse permutation.  O(L^2) compares per slate, on purpose: slates are short, and ordering a whole
// catalogue is mamdr_rank_domain's job.  Integers only, no atomics: every output word has one writer (slates of distinct
// ids have distinct keys, so their positions are a permutation and no two entries claim one slot of `order`).
//   LONG = false: slates of 1 .. SLATE_WAVE entries, one wave per query of the block (wave w of workgroup b: query 4 b + w;
//     other lengths are stepped over).  Lane l holds key l, 0 behind the slate's end -- below every key, keys being at
//     least 1 << 32 --, and key i reaches every lane as two lane reads with a wave-uniform index.
//   LONG = true: longer slates, one workgroup per (SLATE_TILE entries, query) (workgroups of other slates and behind a
//     slate's end leave at once).  The slate's keys pass through LDS SLATE_STAGE at a time; every thread compares its own
//     key with each staged key: all lanes read one address, a broadcast without bank conflicts.
template <bool LONG>
__global__ __launch_bounds__(REC_THREADS) void k_slate_order(const SlateArgs a) {
    const int tid = threadIdx.x;
    if (!LONG) {
        const int lane = tid & 63;
        const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * (REC_THREADS / 64) + (tid >> 6));
        if (q >= a.n_query) return;
        const int64_t o0 = a.off[q];
        const int64_t len = a.off[q + 1] - o0;
        if (len < 1 || len > SLATE_WAVE) return;
        const int L = __builtin_amdgcn_readfirstlane((int)len);
        const u64 key = lane < L ? a.tkey[o0 + lane] : 0ull;
        const int klo = (int)(uint32_t)key, khi = (int)(uint32_t)(key >> 32);
        int cnt = 0;
        for (int i = 0; i < L; ++i) {
            const u64 other = ((u64)(uint32_t)__builtin_amdgcn_readlane(khi, i) << 32) |
                              (u64)(uint32_t)__builtin_amdgcn_readlane(klo, i);
            cnt += other > key ? 1 : 0;
        }
        if (lane < L) {
            a.pos_out[o0 + lane] = cnt;
            if (a.order_out) a.order_out[o0 + cnt] = lane;
        }
    } else {
        __shared__ u64 sk[SLATE_STAGE];
        const int q = blockIdx.y;
        const int64_t o0 = a.off[q];
        const int64_t len = a.off[q + 1] - o0;
        const int64_t e0 = (int64_t)blockIdx.x * SLATE_TILE;
        if (len <= SLATE_WAVE || e0 >= len) return;              // (uniform over the workgroup: before any barrier)
        const int64_t e = e0 + tid;
        const bool in = e < len;
        const u64 key = in ? a.tkey[o0 + e] : ~0ull;
        int cnt = 0;
        for (int64_t s0 = 0; s0 < len; s0 += SLATE_STAGE) {
            const int n = (int)(len - s0 < SLATE_STAGE ? len - s0 : SLATE_STAGE);
            if (s0) __syncthreads();                             // every thread is done with the stage before
#pragma unroll
            for (int t = 0; t < SLATE_STAGE / REC_THREADS; ++t) {
                const int i = tid + REC_THREADS * t;
                if (i < n) sk[i] = a.tkey[o0 + s0 + i];
            }
            __syncthreads();
#pragma unroll 8
            for (int i = 0; i < n; ++i) cnt += sk[i] > key ? 1 : 0;
        }
        if (in) {
            a.pos_out[o0 + e] = cnt;
            if (a.order_out) a.order_out[o0 + cnt] = (int32_t)e;
        }
    }
}

}  // namespace

void launch_slate_order(const SlateArgs& a, int64_t max_len, bool any_short, hipStream_t s) {
    // (the block's LAST launch carries a profiling scope's stop event: the slot times both)
    const bool any_long = max_len > SLATE_WAVE;
    if (any_short) {
        const dim3 grid((a.n_query + REC_THREADS / 64 - 1) / (REC_THREADS / 64));
        if (any_long) hipLaunchKernelGGL(k_slate_order<false>, grid, dim3(REC_THREADS), 0, s, a);
        else MAMDR_LAUNCH(k_slate_order<false>, grid, dim3(REC_THREADS), 0, s, a);
    }
    if (any_long)
        MAMDR_LAUNCH(k_slate_order<true>, dim3((unsigned)((max_len + SLATE_TILE - 1) / SLATE_TILE), a.n_query), dim3(REC_THREADS),
                     0, s, a);
}

void launch_rec_item_proj(const RecArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_rec_item_proj, dim3((a.n_chunk + IP_ROWS - 1) / IP_ROWS), dim3(REC_THREADS), 0, s, a);
}
void launch_rec_query_proj(const RecArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_rec_query_proj, dim3(a.n_query), dim3(REC_THREADS), 0, s, a);
}
// -> false: the 66 KB of LDS were refused (hipFuncSetAttribute), nothing was launched
template <typename K>
static bool raise_lds(K kernel) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(SC_FLOATS * sizeof(float))) == hipSuccess;
}
bool launch_rec_score(const RecArgs& a, hipStream_t s) {
    static const bool raised = raise_lds(k_rec_score<REC_EPI_TOPK>);
    if (!raised) return false;
    MAMDR_LAUNCH(k_rec_score<REC_EPI_TOPK>, dim3(a.tiles, a.n_query), dim3(REC_THREADS), SC_FLOATS * sizeof(float), s, a);
    return true;
}
bool launch_rec_count(const RecArgs& a, hipStream_t s) {
    static const bool raised = raise_lds(k_rec_score<REC_EPI_COUNT>);
    if (!raised) return false;
    MAMDR_LAUNCH(k_rec_score<REC_EPI_COUNT>, dim3(a.tiles, a.n_query), dim3(REC_THREADS), SC_FLOATS * sizeof(float), s, a);
    return true;
}
bool launch_rec_pair(const RecArgs& a, hipStream_t s) {
    static const bool raised = raise_lds(k_rec_pair);
    if (!raised) return false;
    MAMDR_LAUNCH(k_rec_pair, dim3((a.n_chunk + REC_TILE - 1) / REC_TILE), dim3(REC_THREADS), SC_FLOATS * sizeof(float), s, a);
    return true;
}
void launch_rec_merge(const RecArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_rec_merge, dim3(a.n_query), dim3(REC_THREADS), 0, s, a);
}

}  // namespace mamdr
