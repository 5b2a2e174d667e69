// Generic-layer engine, device side 6 / 6: retrieval from the single-output towers (mamdr_graph_recommend, _recommend_domain,
// _rank_domain, _rank_slates; include/mamdr_hip.h).  After graph_towers.h (wave_sum, head_logit, HeadArgs).
// Included by graph_engine.hip alone (see the map at its head): the unnamed namespace is that one translation unit's.
//
// These towers do not separate into a query term and an item term, so every (user, item, domain) pair is one row of an
// ordinary inference batch: k_graph_pair_rows writes the batch's uid / pid / dom columns into a workspace of the handle, the
// engine's own gather and tower run over them, and k_graph_head_keys ends the head in the family's 64-bit key (rec_device.h)
// instead of the loss.  Endings: k_graph_tile_topk (a wave sorts a 64-key tile; the step engine's k_rec_merge keeps the
// running best 128), k_graph_rank_count (ballot + popcount against the query's target keys, integer atomics), or the step
// engine's k_slate_order over the keys of the list form.  Wave64 throughout, integers in every ending, no float atomics.
#pragma once
#include "mamdr_kernels.h"
#include "rec_device.h"

namespace {
using namespace mamdr;

struct PairArgs {
    // the forward batch's columns (what launch_gather reads as a SplitData) and what the head needs per row
    int32_t *uid, *pid, *dom;
    float* label;
    int32_t* rowq;              // the row's query within the block; -1: a padding row of the grid form (key 0)
    int rows;                   // rows of this forward batch
    int n_user, n_item, n_domain;
    const int32_t* q_uid;       // [n_query] of the block
    const int32_t* q_dom;       // per-query domains, or null: every query in dom_all
    int dom_all, n_query;
    const int32_t* ids;         // grid form: the candidate list (null: candidate at position p is item p); list form: the flat list
    // grid form: row r of the batch is pair R = row_base + r of the block's [n_query][chunk_pad] grid, query-major
    int64_t row_base, c_base;
    int chunk_pad, n_chunk;
    // list form: row r is entry list_base + r of the call's flat list; its query from the block's CSR (absolute offsets)
    const int64_t* off;
    int64_t list_base;
};
// grid form (LIST = false) and list form (LIST = true): one thread per row
template <bool LIST>
__global__ __launch_bounds__(256) void k_graph_pair_rows(const PairArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    int q, id;
    bool in = true;
    if (LIST) {
        const int64_t j = a.list_base + r;
        int lo = 0, hi = a.n_query - 1;                 // first q with off[q + 1] > j (queries without entries are stepped over)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.off[mid + 1] <= j) lo = mid + 1; else hi = mid;
        }
        q = lo;
        id = a.ids[j];
    } else {
        const int64_t R = a.row_base + r;
        q = (int)(R / a.chunk_pad);
        const int p = (int)(R - (int64_t)q * a.chunk_pad);
        in = p < a.n_chunk;
        id = in ? (a.ids ? a.ids[a.c_base + p] : (int)(a.c_base + p)) : 0;
    }
    a.uid[r] = clampi(a.q_uid[q], 0, a.n_user - 1);
    a.pid[r] = clampi(id, 0, a.n_item - 1);
    a.dom[r] = clampi(a.q_dom ? a.q_dom[q] : a.dom_all, 0, a.n_domain - 1);
    a.label[r] = 0.f;
    a.rowq[r] = in ? q : -1;
}

struct KeyArgs {
    HeadArgs h;                 // act, ld, t_col, n_t, w, gb, extra, rows: the inference head's operands
    const int32_t *pid, *rowq;
    // grid form
    const int64_t* excl_off;    // nullable CSR of the block's queries, ids ascending
    const int32_t* excl_ids;
    float* scores_all;          // nullable [n_query][n_cand] of the block
    int64_t n_cand, c_base, row_base;
    int chunk_pad;
    u64* keys;                  // [rows] of this forward batch
    // list form
    u64* tkey;                  // [entries of the call]
    float* score_out;           // nullable
    int64_t list_base;
};
// the inference head with a key ending, one wave per row as k_graph_head
template <bool LIST>
__global__ __launch_bounds__(256) void k_graph_head_keys(const KeyArgs a) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.h.rows) return;
    float logit = head_logit(a.h, r, lane);
    logit += 0.f;                                   // -0 -> +0: equal logits are equal keys
    if (lane != 0) return;
    const int id = a.pid[r];
    if (LIST) {
        a.tkey[a.list_base + r] = rec_key(logit, id);
        if (a.score_out) a.score_out[a.list_base + r] = rec_sigmoid(logit);
        return;
    }
    const int q = a.rowq[r];
    bool valid = q >= 0;
    if (valid && a.excl_off) {
        int64_t lo = a.excl_off[q], hi = a.excl_off[q + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.excl_ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo < a.excl_off[q + 1] && a.excl_ids[lo] == id) valid = false;
    }
    if (q >= 0 && a.scores_all) {
        const int64_t R = a.row_base + r;
        a.scores_all[(size_t)q * a.n_cand + a.c_base + (R - (int64_t)q * a.chunk_pad)] = valid ? rec_sigmoid(logit) : 0.f;
    }
    a.keys[r] = valid ? rec_key(logit, id) : 0ull;
}

struct TileArgs {
    const u64* keys;            // [64 n_tiles] of this forward batch
    int n_tiles;
    int64_t row_base;           // the batch's first pair in the block's grid (a multiple of 64)
    int chunk_pad;
    // top-K
    u64* part;                  // [n_query][tiles_cap][kt]
    int tiles_cap, kt;
    // ranks
    const int64_t* tgt_off;     // the block's CSR (absolute positions into tkey / rank_out)
    const u64* tkey;
    int32_t* rank_out;
    int32_t* live_out;          // [n_query] of the block
};
// one wave per 64-key tile: its keys sorted, the first kt to the (query, tile) list that k_rec_merge reads
__global__ __launch_bounds__(256) void k_graph_tile_topk(const TileArgs a) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= a.n_tiles) return;
    const int64_t R = a.row_base + 64 * (int64_t)t;
    const int q = (int)(R / a.chunk_pad), tile = (int)((R - (int64_t)q * a.chunk_pad) >> 6);
    const u64 key = rec_wave_sort(a.keys[64 * t + lane], lane);
    if (lane < a.kt) a.part[((size_t)q * a.tiles_cap + tile) * a.kt + lane] = key;
}
// one wave per 64-key tile: the tile's live candidates, and for every target of its query the keys above the target's
__global__ __launch_bounds__(256) void k_graph_rank_count(const TileArgs a) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= a.n_tiles) return;
    const int64_t R = a.row_base + 64 * (int64_t)t;
    const int q = (int)(R / a.chunk_pad);
    const u64 key = a.keys[64 * t + lane];
    const int live = __popcll(__ballot(key != 0ull));
    if (lane == 0 && live) atomicAdd(a.live_out + q, live);
    const int64_t t1 = a.tgt_off[q + 1];
    for (int64_t j = a.tgt_off[q]; j < t1; ++j) {
        const int cnt = __popcll(__ballot(key > a.tkey[j]));      // (a key of 0 is above no target: tkey >= 1 << 32)
        if (lane == 0 && cnt) atomicAdd(a.rank_out + j, cnt);
    }
}

}  // namespace
