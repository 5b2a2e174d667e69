// Per-user grouped AUC (GAUC) of one split's predictions (mamdr_group_auc, include/mamdr_hip.h).  No reference
// counterpart: the reference's pipeline ends at one 500-threshold AUC per domain.
//
// Definition.  For one split of one domain, group the rows by uid.  For a group u with r_u rows, P_u of them positive
// (label != 0, as the eval histogram classifies) and N_u negative:
//   T_u = 2 * #{(p, n): s_p > s_n} + #{(p, n): s_p == s_n} over positive rows p and negative rows n of the group.  It is
//   an integer.  AUC_u = T_u / (2 * P_u * N_u), the Mann-Whitney statistic with ties counted half.
//   Predictions compare as IEEE floats, with three rules.  -0 equals +0.  A NaN is below every number, -inf included.
//   Two NaNs are equal.
//   A group is valid when P_u > 0 and N_u > 0.
//   GAUC = sum_valid r_u * AUC_u / sum_valid r_u.
//   Reported beside it: n_groups, n_valid and rows_valid = sum_valid r_u.
//   When no group is valid, GAUC is reported as 0.0 with n_valid = 0 (the convention of recommend.ranking_metrics).
//
// Phases, one launch each, the kernel boundary is the hand-off:
//   k_gauc_small    groups of up to 64 rows: one wave per group, one row per lane; every negative row's key is broadcast
//                   by a wave shuffle and two ballots count the positive lanes above / not below it.  Counters are
//                   wave-uniform integers; no LDS, no atomics.  Stores T_u and P_u.
//   k_gauc_tiles    groups of more than 64 rows: one workgroup per tile of up to 256 consecutive positions of one group;
//                   thread t owns position tile_first + t.  The WHOLE group streams through LDS 256 positions at a time
//                   as (order-preserving 32-bit key, negative flag); a positive owner counts the negatives it is above /
//                   not below.  Wave shuffle tree, the four waves through LDS, then ONE 64-bit integer atomicAdd per tile
//                   into T_u (and one 32-bit one into P_u): r^2 / 256 comparisons per tile, any group size.
//   k_gauc_terms    per block of 2,048 groups: the fp64 terms (double) r_u * ((double) T_u / (double)(2 P_u N_u)) of the
//                   valid groups and the integer sums rows_valid, n_valid, added up by a fixed tree.
//   k_gauc_finish   one workgroup adds the blocks' partials by the same tree and writes the four results.
//
// Determinism: T_u and P_u are integers (integer atomics commute); the fp64 sum has ONE order per G -- thread t of block
// b adds groups 2048 b + t + 256 i for i = 0 .. 7 in turn, then block_sum's tree (eval_device.h); thread t of the finish
// adds blocks t + 256 i in turn and the same tree -- so the scalar is the same bits from run to run, and, since T_u, P_u
// and r_u do not depend on where a group's rows sit in the file or in `order`, under any row permutation.  No
// floating-point atomics.  This unit is compiled with -ffp-contract=off: the term is one division, one multiplication and
// then additions, as the host definition (mamdr_amd/gauc.py) computes it.
#include "eval_device.h"

namespace mamdr {
namespace {

constexpr int GAUC_THREADS = THREADS;
constexpr int GAUC_WAVES = WAVES;
constexpr int TERMS_PER_THREAD = 8;
constexpr int TERMS_PER_BLOCK = GAUC_THREADS * TERMS_PER_THREAD;       // 2,048 groups per block of k_gauc_terms
static_assert(GAUC_TILE == GAUC_THREADS, "one thread per tile position");
static_assert(GAUC_SMALL == 64, "one lane per row of a small group");

// (key, is-positive) of the row at position `pos` of `order`, the key being score_key (mamdr_kernels.h): the definition's
// comparison; a row index outside the split is clamped into it
__device__ __forceinline__ uint32_t gauc_row(const GaucArgs& a, int64_t pos, bool& positive) {
    const int row = clampi(a.order[pos], 0, (int)(a.n - 1));
    positive = a.label[row] != 0.f;
    return score_key(a.pred[row]);
}

__global__ __launch_bounds__(GAUC_THREADS) void k_gauc_small(const GaucArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * GAUC_WAVES + (threadIdx.x >> 6);
    if (g >= a.n_groups) return;
    const int64_t lo = a.group_off[g], r = a.group_off[g + 1] - lo;
    if (r > GAUC_SMALL) return;                       // k_gauc_tiles' groups
    const bool in = lane < r && lo + lane < a.n;
    bool positive = false;
    uint32_t key = 0u;
    if (in) key = gauc_row(a, lo + lane, positive);
    const u64 pos_mask = __ballot(in && positive);
    u64 neg_mask = __ballot(in && !positive);
    uint32_t t = 0u;
    if (pos_mask != 0ull)
        while (neg_mask != 0ull) {                    // (wave-uniform: every lane walks the same negatives)
            const int j = __ffsll((long long)neg_mask) - 1;
            neg_mask &= neg_mask - 1ull;
            const uint32_t kj = (uint32_t)__shfl((int)key, j);
            t += (uint32_t)__popcll(__ballot(in && positive && key > kj)) + (uint32_t)__popcll(__ballot(in && positive && key >= kj));
        }
    if (lane == 0) {
        a.T[g] = t;
        a.P[g] = (uint32_t)__popcll(pos_mask);
    }
}

__global__ __launch_bounds__(GAUC_THREADS) void k_gauc_tiles(const GaucArgs a) {
    __shared__ uint32_t keys[GAUC_TILE];
    __shared__ uint32_t is_neg[GAUC_TILE];
    __shared__ u64 part_t[GAUC_WAVES];
    __shared__ uint32_t part_p[GAUC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t g = a.tile_group[blockIdx.x];
    if (g < 0 || g >= a.n_groups) return;             // (block-uniform)
    const int64_t lo = a.group_off[g];
    if (a.group_off[g + 1] - lo <= GAUC_SMALL) return;          // (k_gauc_small's group: a tile has no business here)
    const int64_t hi = a.group_off[g + 1] < a.n ? a.group_off[g + 1] : a.n;
    const int64_t mine = a.tile_first[blockIdx.x] + tid;
    bool positive = false;
    uint32_t key = 0u;
    if (mine >= lo && mine < hi) key = gauc_row(a, mine, positive);
    const bool counts = positive;                     // a positive row of this tile
    uint32_t above = 0u, not_below = 0u;              // each at most r < 2^31
    for (int64_t c0 = lo; c0 < hi; c0 += GAUC_TILE) {
        bool p = true;
        uint32_t k = 0u;
        if (c0 + tid < hi) k = gauc_row(a, c0 + tid, p);
        __syncthreads();                              // (the previous chunk has been read)
        keys[tid] = k;
        is_neg[tid] = p ? 0u : 1u;
        __syncthreads();
        if (counts) {
#pragma unroll 8
            for (int j = 0; j < GAUC_TILE; ++j) {
                const uint32_t kj = keys[j], nj = is_neg[j];      // (LDS broadcasts)
                above += (key > kj ? nj : 0u);
                not_below += (key >= kj ? nj : 0u);
            }
        }
    }
    // integers: any order gives the same sums.  Not block_sum: the positives of a wave are one popcount, and a (u64, uint32)
    // struct per wave would pad the LDS parts from 48 to 64 bytes
    const u64 t = wave_reduce<AddU64>(counts ? (u64)above + (u64)not_below : 0ull);
    const uint32_t pcount = (uint32_t)__popcll(__ballot(counts));
    if (lane == 0) {
        part_t[w] = t;
        part_p[w] = pcount;
    }
    __syncthreads();
    if (tid == 0) {
        u64 tt = 0ull;
        uint32_t pp = 0u;
#pragma unroll
        for (int i = 0; i < GAUC_WAVES; ++i) {
            tt += part_t[i];
            pp += part_p[i];
        }
        atomicAdd(a.T + g, tt);                       // integer atomics: the sums do not depend on the arrival order
        atomicAdd(a.P + g, pp);
    }
}

struct GaucSum {                 // (block_sum, eval_device.h)
    double num;
    u64 rows, valid;
    __device__ __forceinline__ void add(const GaucSum& o) {
        num += o.num;
        rows += o.rows;
        valid += o.valid;
    }
    __device__ __forceinline__ GaucSum down(int o) const { return GaucSum{__shfl_down(num, o), __shfl_down(rows, o), __shfl_down(valid, o)}; }
};

__global__ __launch_bounds__(GAUC_THREADS) void k_gauc_terms(const GaucArgs a) {
    __shared__ GaucSum lds[GAUC_WAVES];
    GaucSum v = {0.0, 0ull, 0ull};
#pragma unroll
    for (int i = 0; i < TERMS_PER_THREAD; ++i) {
        const int64_t g = (int64_t)blockIdx.x * TERMS_PER_BLOCK + i * GAUC_THREADS + threadIdx.x;
        if (g >= a.n_groups) continue;
        const u64 r = (u64)(a.group_off[g + 1] - a.group_off[g]);
        const u64 p = a.P[g];
        if (p == 0ull || p >= r) continue;            // all-negative / all-positive: not a valid group
        const u64 nn = r - p;
        v.num += (double)r * ((double)a.T[g] / (double)(2ull * p * nn));
        v.rows += r;
        v.valid += 1ull;
    }
    const GaucSum s = block_sum(v, lds);
    if (threadIdx.x == 0) {
        a.part_num[blockIdx.x] = s.num;
        a.part_rows[blockIdx.x] = s.rows;
        a.part_valid[blockIdx.x] = s.valid;
    }
}

__global__ __launch_bounds__(GAUC_THREADS) void k_gauc_finish(const GaucArgs a) {
    __shared__ GaucSum lds[GAUC_WAVES];
    GaucSum v = {0.0, 0ull, 0ull};
    for (int64_t b = threadIdx.x; b < a.n_parts; b += GAUC_THREADS) {
        v.num += a.part_num[b];
        v.rows += a.part_rows[b];
        v.valid += a.part_valid[b];
    }
    const GaucSum s = block_sum(v, lds);
    if (threadIdx.x == 0) {
        a.result[0] = s.num;
        a.result[1] = (double)s.rows;
        a.result[2] = (double)s.valid;
        a.result[3] = (double)a.n_groups;
    }
}

}  // namespace

int64_t gauc_parts(int64_t n_groups) { return (n_groups + TERMS_PER_BLOCK - 1) / TERMS_PER_BLOCK; }

void launch_gauc(const GaucArgs& a, hipStream_t s) {
    if (a.n_groups > 0) {
        MAMDR_LAUNCH(k_gauc_small, dim3((unsigned)((a.n_groups + GAUC_WAVES - 1) / GAUC_WAVES)), dim3(GAUC_THREADS), 0, s, a);
        if (a.n_tiles > 0) MAMDR_LAUNCH(k_gauc_tiles, dim3((unsigned)a.n_tiles), dim3(GAUC_THREADS), 0, s, a);
        MAMDR_LAUNCH(k_gauc_terms, dim3((unsigned)a.n_parts), dim3(GAUC_THREADS), 0, s, a);
    }
    MAMDR_LAUNCH(k_gauc_finish, dim3(1), dim3(GAUC_THREADS), 0, s, a);
}

}  // namespace mamdr
