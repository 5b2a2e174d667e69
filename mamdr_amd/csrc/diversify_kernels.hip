// Diversified re-ranking of candidate lists: greedy Maximal Marginal Relevance (mamdr_list_diversify; include/mamdr_hip.h).
// No reference counterpart: the reference never builds a list.
//
// k_list_div<W>   one workgroup of W waves per list: W = 1 for n <= 32, W = 4 beyond, as k_list_sim.
//   Phase 1 is k_list_sim's steps 1 - 3 (list_gram.h: compaction of the L valid entries, rows through LDS, upper-triangle
//   Gram tiles on v_mfma_f32_32x32x2_f32, squared norms from the diagonal) and its quotient ls_cos, so the cosine of a pair
//   a < b is the fp32 number mamdr_list_similarity forms for it.  Every lane writes its tile's cosines of the pairs
//   row < col < L to BOTH halves of an LDS matrix cosm[ROWS][ROWS + 1]; the diagonal and everything at or beyond L is never
//   written and never read.  The matrix ALIASES the staging tile: ls_gram ends behind a barrier that follows the tile's last
//   read.  LDS: 128 x 129 floats = 66,048 B (the staging tile's 34,816 B inside them) + 2.1 KiB of per-entry arrays for
//   W = 4; 8,704 B + 0.6 KiB for W = 1.  The odd row length puts the 32 lanes of a ds_write_b32 / ds_read_b32 group on 32
//   banks for all three accesses: cosm[row][col] and cosm[col][row] written with col = lane & 31, cosm[winner][c] read with
//   c = the thread.
//   Phase 2 is min(k, L) greedy steps.  Thread c holds entry c: its relevance, its running maximum m_c of cosines with
//   the picks so far, and whether it has been picked.  A step forms v_c = lambda rel_c - (1 - lambda) m_c in three
//   separately rounded operations (rel_c itself at step 0; the file is compiled without fma contraction), the key
//   rec_key(v_c, id_c) (rec_device.h; 0 = "no entry" once picked), and finds the largest (key, then the smaller c) with an
//   xor butterfly over the wave -- every lane ends with the winner -- and, when L > 64, one LDS exchange between waves 0 and
//   1 behind ONE barrier per step (the two slots alternate with the step's parity, so a step's writes never meet the
//   previous step's reads).  With L <= 64 waves 1 - 3 have no entry and leave before phase 2: no barrier at all, as in the
//   one-wave variant.  The winner writes its position and value; every unpicked thread reads cosm[winner][c].
// Every order depends on the list's own valid entries alone; integer maxima and one fp32 chain per value: a list's outputs
// are the same bits from run to run, wherever the list sits, whatever its neighbours hold, wherever its padding sits,
// whatever n the call has and whichever variant runs it.  No atomics.  Bounds come from L: no global read past the
// compacted rows, no LDS read of an unwritten cosine.
#include "list_gram.h"
#include "rec_device.h"

namespace mamdr {
namespace {

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_list_div(const ListDivArgs a) {
    constexpr int THREADS = LsShape<WAVES>::THREADS, ROWS = LsShape<WAVES>::ROWS, SLOTS = LsShape<WAVES>::SLOTS;
    constexpr int LD = ROWS + 1;                    // floats per row of the cosine matrix: odd -> bank-conflict free
    constexpr int SMEM = ROWS * LD > ROWS * LS_LD ? ROWS * LD : ROWS * LS_LD;
    __shared__ __attribute__((aligned(16))) float smem[SMEM];       // the staging tile, then the cosine matrix
    __shared__ int s_row[ROWS];
    __shared__ int s_pos[ROWS];
    __shared__ float s_rel[ROWS];
    __shared__ float s_n2[ROWS];
    __shared__ int s_cnt[2];
    __shared__ u64 s_wkey[2][2];                    // [step parity][wave 0 / 1]
    __shared__ int s_wc[2][2];
    float* const tile = smem;
    float* const cosm = smem;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t q = blockIdx.x;

    // the valid entries, in list order, with their positions and relevances
    int slot;
    const int L = ls_compact<WAVES>(a.ids, a.n, a.n_rows, q, s_row, s_cnt, slot);
    if (slot >= 0) {
        s_pos[slot] = tid;
        s_rel[slot] = a.rel[q * a.n + tid];
    }
    const int K = a.k < L ? a.k : L;                // picks
    for (int t = K + tid; t < a.k; t += THREADS) {  // behind a short list
        a.pos_out[q * a.k + t] = -1;
        if (a.value_out) a.value_out[q * a.k + t] = 0.f;
    }
    if (L == 0) return;                             // (uniform)
    __syncthreads();

    // phase 1: the cosines of the pairs row < col < L, into both halves of the matrix
    if (L >= 2) {                                   // (uniform)
        LsTiles<WAVES> T;
        ls_gram<WAVES>(a.rows, a.emb_dim, L, s_row, tile, s_n2, T);
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (!T.live[s]) continue;
            const int col = 32 * T.tj[s] + r;
            const float nb = s_n2[col];
            const float sb = sqrtf(nb);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = 32 * T.ti[s] + ls_acc_row(g, h);
                const float na = s_n2[row];                         // (row < 32 n_t: written, or a zero row's zero)
                const float cosv = ls_cos(T.acc[s][g], na, nb, sb);
                if (row < col && col < L) {
                    cosm[row * LD + col] = cosv;
                    cosm[col * LD + row] = cosv;
                }
            }
        }
        __syncthreads();
    }
    const bool cross = WAVES > 1 && L > 64;         // entries on waves 0 and 1
    if (WAVES > 1 && !cross && w > 0) return;       // (wave-uniform; no barrier follows for this workgroup)

    // phase 2: the greedy picks
    const int c = tid;
    const bool mine = c < L;
    const float rel = mine ? s_rel[c] : 0.f;
    const int id = mine ? s_row[c] : 0;
    const int pos = mine ? s_pos[c] : 0;
    const float oml = __fsub_rn(1.0f, a.lambda);
    bool picked = !mine;
    float m = 0.f;
    for (int t = 0; t < K; ++t) {
        float v = rel;
        if (t) v = __fsub_rn(__fmul_rn(a.lambda, rel), __fmul_rn(oml, m));
        u64 key = picked ? 0ull : rec_key(v, id);
        int win = c;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const uint32_t olo = __shfl_xor((uint32_t)key, x, 64), ohi = __shfl_xor((uint32_t)(key >> 32), x, 64);
            const int oc = __shfl_xor(win, x, 64);
            const u64 okey = ((u64)ohi << 32) | olo;
            if (okey > key || (okey == key && oc < win)) {
                key = okey;
                win = oc;
            }
        }
        if (cross) {                                // (uniform)
            const int p = t & 1;
            if (lane == 0 && w < 2) {
                s_wkey[p][w] = key;
                s_wc[p][w] = win;
            }
            __syncthreads();
            const u64 k0 = s_wkey[p][0], k1 = s_wkey[p][1];
            win = k1 > k0 ? s_wc[p][1] : s_wc[p][0];                // (wave 0's entries are the smaller c)
        }
        if (!picked && c == win) {
            picked = true;
            a.pos_out[q * a.k + t] = pos;
            if (a.value_out) a.value_out[q * a.k + t] = v;
        }
        if (!picked && t + 1 < K) {                 // (win < L, c < L, c != win: written in phase 1)
            const float cosv = cosm[win * LD + c];
            m = t ? (cosv > m ? cosv : m) : cosv;
        }
    }
}

}  // namespace

void launch_list_div(const ListDivArgs& a, hipStream_t s) {
    if (a.n <= 32) MAMDR_LAUNCH(k_list_div<1>, dim3((unsigned)a.n_list), dim3(64), 0, s, a);
    else MAMDR_LAUNCH(k_list_div<4>, dim3((unsigned)a.n_list), dim3(256), 0, s, a);
}

}  // namespace mamdr
