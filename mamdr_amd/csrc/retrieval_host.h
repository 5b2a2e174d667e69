// What a retrieval call IS, for both engines: retrieval_call holds the argument contracts of top-K, exact ranks and per-query
// slates with their error texts, the read-back of the CSR offsets, the chunk rule and the loop nest -- query blocks of
// REC_QBLOCK; per block the list pass over its targets / entries, then the candidate chunks or the order inside the slates.
// An entry point fills a RetCall field by field; its engine's backend B only says how it scores pairs (StepRetrieval in
// step_queries.hip, GraphRetrieval in graph_engine.hip).  B's data: err (ErrBuf&), n_item, n_domain, rec_chunk.  B's members:
// ready() (!= 0: explained in err); read_back(host, dev, n): n int64 from the device, waited for; fill(dev, byte, bytes) on
// its stream; prepare(call): state up to date, workspaces sized; begin_block(block); list_pass(j0, j1): keys (and scores) of
// entries [j0, j1) of list_ids; cand_pass(c0, n_chunk, tiles, first, last): a chunk of candidates x the block's queries, merged
// into the block's top-K or counted against its target keys; slate_order(max_len, any_short); finish().  The int ones return
// MAMDR_OK or the code err explains.  No HIP here: tests/host/retrieval_plan_check.cpp drives the template.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_base.h"

namespace mamdr {

enum RetKind { RET_TOPK, RET_RANK, RET_SLATES };

// a call's arguments as its entry point received them (what a form does not have stays null / 0).  A backend sees it twice:
// whole in prepare(), and per block in begin_block() with n_query the block's and the per-query pointers (uid, dom, excl_off,
// ids_out, scores_out, scores_all, list_off, live_out) offset to the block's first query
struct RetCall {
    RetKind kind;
    const char* fn;
    bool per_query = false;                                             // mamdr_recommend's form: query q in dom[q],
    int32_t domain = -1, n_query = 0;                                   // `domain` left at -1
    const int32_t *uid = nullptr, *dom = nullptr, *cand = nullptr;
    int64_t n_cand = 0;                                                 // no list given: the catalogue's size, set here
    int chunk = 0;                                                      // candidates per pass, set here
    const int64_t* excl_off = nullptr;
    const int32_t* excl_ids = nullptr;
    int32_t k = 0, *ids_out = nullptr;                                  // top-K
    float *scores_out = nullptr, *scores_all = nullptr;
    const int64_t* list_off = nullptr;                                  // ranks: the targets; slates: their entries
    const int32_t* list_ids = nullptr;
    int64_t n_list = 0;                                                 // set here, from the offsets
    float* score_out = nullptr;
    int32_t *rank_out = nullptr, *live_out = nullptr, *pos_out = nullptr, *order_out = nullptr;     // ranks | slates
};

// candidates per pass of a call over n_cand candidates
inline int retrieval_chunk(int rec_chunk, int64_t n_cand) {
    return (int)std::min<int64_t>(rec_chunk, (n_cand + REC_TILE - 1) / REC_TILE * REC_TILE);
}

// the queries [qb, qb + REC_QBLOCK) of a call
inline RetCall retrieval_block(RetCall r, int32_t qb) {
    const size_t q = (size_t)qb;
    r.n_query = std::min<int32_t>(REC_QBLOCK, r.n_query - qb);
    r.uid += q;
    if (r.dom) r.dom += q;
    if (r.excl_off) r.excl_off += q;
    if (r.ids_out) r.ids_out += q * r.k;
    if (r.scores_out) r.scores_out += q * r.k;
    if (r.scores_all) r.scores_all += q * r.n_cand;
    if (r.list_off) r.list_off += q;
    if (r.live_out) r.live_out += q;
    return r;
}

template <class B>
int retrieval_call(B& b, RetCall r) {
    ErrBuf& err = b.err;
    const char* fn = r.fn;
    const bool topk = r.kind == RET_TOPK, slates = r.kind == RET_SLATES;
    // ---- the contract.  A pointer that a form does not have is null, and null is aligned
    if (!r.per_query && (r.domain < 0 || r.domain >= b.n_domain))
        return err.fail(MAMDR_EINVAL, "%s: domain %d outside [0, %d)", fn, r.domain, b.n_domain);
    if (r.n_query <= 0) return err.fail(MAMDR_EINVAL, "%s: n_query %d must be positive", fn, r.n_query);
    if (topk && (r.k < 1 || r.k > REC_KMAX)) return err.fail(MAMDR_EINVAL, "%s: k %d outside [1, %d]", fn, r.k, REC_KMAX);
    if (r.cand && r.n_cand <= 0) return err.fail(MAMDR_EINVAL, "%s: n_cand %lld with a candidate list given", fn, (long long)r.n_cand);
    if (topk && (!r.uid || (r.per_query && !r.dom) || !r.ids_out || !r.scores_out))
        return err.fail(MAMDR_EINVAL, r.per_query ? "%s: null uid / domain / output pointer" : "%s: null uid / output pointer", fn);
    if (r.kind == RET_RANK && (!r.uid || !r.list_off || !r.rank_out || !r.live_out))
        return err.fail(MAMDR_EINVAL, "%s: null uid / target offsets / rank / live output pointer", fn);
    if (slates && (!r.uid || !r.list_off || !r.pos_out))
        return err.fail(MAMDR_EINVAL, "%s: null uid / slate offsets / position output pointer", fn);
    if (misaligned(3, r.uid, r.dom, r.cand, r.excl_ids, r.ids_out, r.scores_out, r.scores_all, r.list_ids, r.score_out, r.rank_out,
                   r.live_out, r.pos_out, r.order_out) || misaligned(7, r.excl_off, r.list_off))
        return err.fail(MAMDR_EINVAL, "%s: a pointer is not aligned to its element size", fn);
    if ((r.excl_off == nullptr) != (r.excl_ids == nullptr))
        return err.fail(MAMDR_EINVAL, "%s: the exclusion lists need both their offsets and their ids", fn);
    if (b.ready()) return MAMDR_ESTATE;
    // ---- the CSR offsets of the targets / slate entries size the launches and the key workspace: read back once (the
    // call's one synchronisation of the handle's stream) and held to their contract here, so that no kernel indexes past the list
    std::vector<int64_t> off;
    if (!topk) {
        const char* what = slates ? "slate" : "target";
        off.resize((size_t)r.n_query + 1);
        if (const int rc = b.read_back(off.data(), r.list_off, off.size())) return rc;
        if (off[0] != 0) return err.fail(MAMDR_EINVAL, "%s: the %s offsets start at %lld, not 0", fn, what, (long long)off[0]);
        for (int32_t q = 0; q < r.n_query; ++q)
            if (off[q + 1] < off[q]) return err.fail(MAMDR_EINVAL, "%s: the %s offsets descend at query %d", fn, what, q);
        for (int32_t q = 0; slates && q < r.n_query; ++q)
            if (off[q + 1] - off[q] > INT32_MAX)
                return err.fail(MAMDR_EINVAL, "%s: slate %d has %lld entries: positions are int32", fn, q, (long long)(off[q + 1] - off[q]));
        r.n_list = off[r.n_query];
        if (slates && r.n_list == 0) return MAMDR_OK;           // done before any workspace is touched
        if (r.n_list > 0 && !r.list_ids)
            return err.fail(MAMDR_EINVAL, "%s: %lld %s without their ids", fn, (long long)r.n_list, slates ? "entries" : "targets");
    }
    // ---- a slate is ranked against itself: no candidates, no candidate pass
    if (!slates) {
        if (!r.cand) r.n_cand = b.n_item;
        r.chunk = retrieval_chunk(b.rec_chunk, r.n_cand);
    }
    if (const int rc = b.prepare(r)) return rc;
    if (r.rank_out && r.n_list > 0)
        if (const int rc = b.fill(r.rank_out, 0, (size_t)r.n_list * sizeof(int32_t))) return rc;
    if (r.live_out)
        if (const int rc = b.fill(r.live_out, 0, (size_t)r.n_query * sizeof(int32_t))) return rc;
    if (r.order_out)
        if (const int rc = b.fill(r.order_out, 0xff, (size_t)r.n_list * sizeof(int32_t))) return rc;
    for (int32_t qb = 0; qb < r.n_query; qb += REC_QBLOCK) {
        const RetCall blk = retrieval_block(r, qb);
        const int32_t qe = qb + blk.n_query;
        if (slates && off[qe] == off[qb]) continue;             // a block of empty slates launches nothing
        b.begin_block(blk);
        // ranks: for a block without targets too, and its candidate passes all the same: live_out needs them
        if (!topk)
            if (const int rc = b.list_pass(off[qb], off[qe])) return rc;
        for (int64_t c0 = 0; c0 < r.n_cand; c0 += r.chunk) {
            const int n_chunk = (int)std::min<int64_t>(r.chunk, r.n_cand - c0);
            if (const int rc = b.cand_pass(c0, n_chunk, (n_chunk + REC_TILE - 1) / REC_TILE, c0 == 0, c0 + r.chunk >= r.n_cand)) return rc;
        }
        if (!slates) continue;
        int64_t max_len = 0;
        bool any_short = false;
        for (int32_t q = qb; q < qe; ++q) {
            const int64_t len = off[q + 1] - off[q];
            max_len = std::max(max_len, len);
            any_short = any_short || (len >= 1 && len <= SLATE_WAVE);
        }
        b.slate_order(max_len, any_short);
    }
    return b.finish();
}

}  // namespace mamdr
