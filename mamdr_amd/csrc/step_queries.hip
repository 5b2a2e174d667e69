// C ABI of libmamdr_hip.so, the queries of a step-kernel context: evaluation of a split (mamdr_eval_domain), the gathered
// input rows (mamdr_gather_rows), top-K retrieval (mamdr_recommend(_domain)), the exact ranks of target items
// (mamdr_rank_domain) and per-query candidate slates (mamdr_rank_slates).  (The metrics of predictions: eval_metrics.hip.)
// The four retrieval calls are retrieval_host.h's retrieval_call, shared with the generic-layer engine; this file holds the
// step engine's backend (StepRetrieval: the workspace and the launches of recommend_kernels.hip) and its own refusals.
#include <algorithm>

#include "step_ctx.h"
#include "retrieval_host.h"

extern "C" {

int mamdr_eval_domain(mamdr_ctx* c, int domain, int split, int32_t batch, float* d_loss_out, uint32_t* d_hist,
                      float* d_pred_out) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    SplitData* d = split_of(c, domain, split);
    if (!d || !d->bound) return fail(MAMDR_ESTATE, "split %d of domain %d is not bound", split, domain);
    if (!d_loss_out || !d_hist) return fail(MAMDR_EINVAL, "null output pointer");
    sync_tables(c);
    if (batch <= 0 || batch % TILE_ROWS != 0) return fail(MAMDR_EINVAL, "eval batch must be a positive multiple of %d", TILE_ROWS);
    if (d->n <= 0) return fail(MAMDR_EINVAL, "split %d of domain %d is empty", split, domain);
    HIP_TRY(hipMemsetAsync(d_hist, 0, 2 * 501 * sizeof(uint32_t), c->stream));
    TowerArgs ta;
    fill_tower_common(c, *d, ta);
    ta.perm = nullptr;
    ta.row_base = 0;
    ta.rows = (int)d->n;
    ta.batch = batch;
    ta.loss_part = c->eval_part.p;
    ta.hist = d_hist;
    ta.pred_out = d_pred_out;
    if (c->star) {
        // inference: domain `domain`'s moving statistics and merged kernels (partitioned_norm.py:143-165)
        StarPrepArgs pa;
        fill_star_prep(c, domain, pa);
        launch_star_prep(pa, c->stream);
        ta.dense = c->eff;
        ta.pn_aff = c->pn;
    }
    {
        Prof p(c, MAMDR_KERNEL_EVAL);
        launch_tower_eval(ta, c->stream);
    }
    if (c->cfg.emb_trainable) refresh_table_sumsq(c);
    EvalFinishArgs fa;
    fa.loss_part = c->eval_part.p;
    fa.n_rows = d->n;
    fa.batch = batch;
    fa.dense = c->params + c->table_floats;
    fa.dm_count = c->star ? 0 : c->cfg.n_domain * EMB;
    fa.l2_emb = c->star ? 0.f : c->cfg.l2_emb;
    fa.frozen_sumsq = c->frozen_sumsq;
    fa.ld_off = c->L.ld;
    fa.ld_count = c->L.ld_count;
    fa.l2_lin = c->cfg.l2_linear;
    fa.loss_out = d_loss_out;
    launch_eval_finish(fa, c->stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_gather_rows(mamdr_ctx* c, int domain, int split, const int32_t* d_perm, int64_t first_row,
                      int64_t n_rows, float* d_out) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    SplitData* d = split_of(c, domain, split);
    if (!d || !d->bound) return fail(MAMDR_ESTATE, "split %d of domain %d is not bound", split, domain);
    if (!d_out) return fail(MAMDR_EINVAL, "null output pointer");
    if (first_row < 0 || n_rows < 0 || first_row + n_rows > d->n) return fail(MAMDR_EINVAL, "row range outside the split");
    if (n_rows == 0) return MAMDR_OK;
    sync_tables(c);
    TowerArgs ta;
    fill_tower_common(c, *d, ta);
    ta.perm = d_perm;
    ta.row_base = first_row;
    ta.rows = (int)n_rows;
    {
        Prof p(c, MAMDR_KERNEL_GATHER);
        launch_gather(ta, d_out, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

}  // extern "C"

// ---- retrieval (recommend_kernels.hip), behind retrieval_host.h
static int grow_rec_workspace(mamdr_ctx* c, int chunk) {
    if (chunk <= c->rec_cap) return MAMDR_OK;
    c->dev.release(c->rec_P);
    c->dev.release(c->rec_lin);
    c->dev.release(c->rec_part);
    c->rec_P = c->rec_lin = nullptr;
    c->rec_part = nullptr;
    c->rec_cap = 0;
    c->dev.alloc(&c->rec_P, (size_t)chunk * H1);
    c->dev.alloc(&c->rec_lin, (size_t)chunk);
    c->dev.alloc(&c->rec_part, (size_t)REC_QBLOCK * chunk);
    if (!c->rec_q) c->dev.alloc(&c->rec_q, (size_t)REC_QBLOCK * (H1 + EMB + 4));
    if (!c->rec_best) c->dev.alloc(&c->rec_best, (size_t)REC_QBLOCK * REC_KMAX);
    if (const int rc = c->dev.check(g_err)) return rc;
    c->rec_cap = chunk;
    return MAMDR_OK;
}

// what every retrieval call does between its argument checks and its launches: tables brought up to date, the workspace
// for `chunk` candidates per pass, and the RecArgs fields that do not change inside the call
static int rec_prepare(mamdr_ctx* c, int32_t domain, const int32_t* d_cand, int64_t n_cand, const int32_t* d_excl_ids,
                       int chunk, RecArgs& a) {
    sync_tables(c);              // lagging table rows and lazily replayed per-domain slices: as mamdr_eval_domain
    prof_break(c);
    if (int e = grow_rec_workspace(c, chunk)) return e;
    memset(&a, 0, sizeof(a));
    a.user_tab = c->cfg.emb_trainable ? c->params : c->user_tab;
    a.item_tab = c->cfg.emb_trainable ? c->params + (size_t)c->cfg.n_user * EMB : c->item_tab;
    a.dense = c->params + c->table_floats;
    a.L = c->L;
    a.dom_all = domain;          // -1: query q in dom[q]
    if (c->star) {
        // inference in `domain`: its moving statistics and merged kernels, exactly as mamdr_eval_domain prepares them.
        // c->eff / c->pn are the training step's workspaces too: star_step rebuilds both at step 0 of every call
        StarPrepArgs pa;
        fill_star_prep(c, domain, pa);
        launch_star_prep(pa, c->stream);
        a.dense = c->eff;
        a.pn = c->pn;
    }
    a.n_user = c->cfg.n_user;
    a.n_item = c->cfg.n_item;
    a.n_domain = c->cfg.n_domain;
    a.mode = c->deepfm ? (c->cfg.tower == MAMDR_TOWER_WDL ? 2 : 1) : 0;
    if (c->deepfm && c->cfg.emb_trainable) {
        a.lin_user = c->params + c->lin_user_off;
        a.lin_item = c->params + c->lin_item_off;
    }
    a.cand = d_cand;
    a.n_cand = n_cand;
    a.excl_ids = d_excl_ids;
    a.tiles_cap = c->rec_cap / REC_TILE;
    a.P = c->rec_P;
    a.lin_i = c->rec_lin;
    a.q0 = c->rec_q;
    a.qud = c->rec_q + (size_t)REC_QBLOCK * H1;
    a.qs = a.qud + (size_t)REC_QBLOCK * EMB;
    a.part = c->rec_part;
    a.best = c->rec_best;
    return MAMDR_OK;
}

namespace {

// the step towers as retrieval_host.h's backend: layer 0 separates into a query term (k_rec_query_proj, once per block) and
// an item term (k_rec_item_proj, per pass), the rest of the tower runs per pair in k_rec_score / k_rec_pair
struct StepRetrieval : RetStream {
    mamdr_ctx* c;
    const int n_item = c->cfg.n_item, n_domain = c->cfg.n_domain, rec_chunk = c->rec_chunk;
    RetCall r{};
    RecArgs a;
    SlateArgs sa;

    int ready() { return ::ready(c); }
    // a slates call has no candidates: its entries are the list the workspace is sized from
    int prepare(const RetCall& call) {
        r = call;
        const int rc = r.kind == RET_SLATES ? rec_prepare(c, r.domain, r.list_ids, r.n_list, nullptr, retrieval_chunk(rec_chunk, r.n_list), a)
                                            : rec_prepare(c, r.domain, r.cand, r.n_cand, r.excl_ids, r.chunk, a);
        if (rc) return rc;
        if (const int e = c->rec_tkey.grow(c->dev, g_err, (size_t)r.n_list)) return e;     // (top-K: no list, no keys)
        a.k = r.k;
        a.kt = std::min<int>(r.k, REC_TILE);
        sa.tkey = a.tkey = r.list_off ? c->rec_tkey.p : nullptr;
        a.tscore_out = r.score_out;
        a.rank_out = r.rank_out;
        sa.pos_out = r.pos_out;
        sa.order_out = r.order_out;
        return MAMDR_OK;
    }
    void begin_block(const RetCall& b) {
        a.n_query = sa.n_query = b.n_query;
        a.uid = b.uid;
        a.dom = b.dom;
        a.excl_off = b.excl_off;
        a.ids_out = b.ids_out;
        a.scores_out = b.scores_out;
        a.scores_all = b.scores_all;
        a.tgt_off = sa.off = b.list_off;
        a.live_out = b.live_out;
        launch_rec_query_proj(a, c->stream);
        prof_break(c);          // (only the slates call times what follows)
    }
    // the item term of the entries, a workspace's worth at a time, then the pair tiles; timed in a slates call only
    int list_pass(int64_t j0, int64_t j1) {
        const bool timed = r.kind == RET_SLATES;
        a.cand = r.list_ids;
        for (int64_t t0 = j0; t0 < j1; t0 += c->rec_cap) {
            a.c_base = t0;
            a.n_chunk = (int)std::min<int64_t>(c->rec_cap, j1 - t0);
            {
                Prof p(c, MAMDR_KERNEL_GATHER, timed);
                launch_rec_item_proj(a, c->stream);
            }
            Prof p(c, MAMDR_KERNEL_EVAL, timed);
            if (!launch_rec_pair(a, c->stream))
                return fail(MAMDR_EHIP, "%s: k_rec_pair was refused its LDS limit (hipFuncSetAttribute)", r.fn);
        }
        return MAMDR_OK;
    }
    // the chunk's item term, then the pair tiles with the top-K ending and the merge, or with the counting ending (which
    // reports itself as k_rec_score too)
    int cand_pass(int64_t c0, int n_chunk, int tiles, bool first, bool last) {
        const bool topk = r.kind == RET_TOPK;
        a.cand = r.cand;
        a.c_base = c0;
        a.n_chunk = n_chunk;
        a.tiles = tiles;
        if (topk) a.first_chunk = first, a.last_chunk = last;
        launch_rec_item_proj(a, c->stream);
        if (!(topk ? launch_rec_score(a, c->stream) : launch_rec_count(a, c->stream)))
            return fail(MAMDR_EHIP, "%s: k_rec_score was refused its LDS limit (hipFuncSetAttribute)", r.fn);
        if (topk) launch_rec_merge(a, c->stream);
        return MAMDR_OK;
    }
    void slate_order(int64_t max_len, bool any_short) {
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_slate_order(sa, max_len, any_short, c->stream);
    }
    int finish() {
        prof_break(c);
        HIP_TRY(hipGetLastError());
        return MAMDR_OK;
    }
};

// an entry point's own part: the handle, the towers whose first layer does not separate into a query and an item term (and
// star where a domain comes per query); then the call
int step_retrieval(mamdr_ctx* c, RetCall& r) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->star && r.per_query)
        return fail(MAMDR_ENOTBUILT, "mamdr_recommend: the star tower is not built for retrieval with a domain per query (its "
                                     "first layer separates into a query and an item term per domain only: "
                                     "mamdr_recommend_domain); mlp, wdl and deepfm are");
    if (c->pnn || c->nfm)
        return fail(MAMDR_ENOTBUILT, "%s: the %s tower is not built for retrieval (its first layer does not separate into a query "
                                     "and an item term); %s are", r.fn, c->pnn ? "pnn" : "nfm",
                    r.per_query ? "mlp, wdl and deepfm" : "mlp, wdl, deepfm and star");
    StepRetrieval b{{c->stream, g_err}, c};
    return retrieval_call(b, r);
}

}  // namespace

extern "C" {

int mamdr_recommend(mamdr_ctx* c, int32_t n_query, const int32_t* d_uid, const int32_t* d_domain, const int32_t* d_cand,
                    int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out,
                    float* d_scores_out, float* d_scores_all) {
    RetCall r{RET_TOPK, __func__};
    r.per_query = true, r.n_query = n_query, r.uid = d_uid, r.dom = d_domain, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids;
    r.k = k, r.ids_out = d_ids_out, r.scores_out = d_scores_out, r.scores_all = d_scores_all;
    return step_retrieval(c, r);
}

int mamdr_recommend_domain(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                           int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k,
                           int32_t* d_ids_out, float* d_scores_out, float* d_scores_all) {
    RetCall r{RET_TOPK, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids;
    r.k = k, r.ids_out = d_ids_out, r.scores_out = d_scores_out, r.scores_all = d_scores_all;
    return step_retrieval(c, r);
}

int mamdr_rank_domain(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                      int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                      const int32_t* d_tgt_ids, int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out) {
    RetCall r{RET_RANK, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids, r.list_off = d_tgt_off, r.list_ids = d_tgt_ids;
    r.rank_out = d_rank_out, r.score_out = d_score_out, r.live_out = d_live_out;
    return step_retrieval(c, r);
}

int mamdr_rank_slates(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int64_t* d_slate_off,
                      const int32_t* d_slate_ids, float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out) {
    RetCall r{RET_SLATES, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.list_off = d_slate_off, r.list_ids = d_slate_ids;
    r.score_out = d_score_out, r.pos_out = d_pos_out, r.order_out = d_order_out;
    return step_retrieval(c, r);
}

}  // extern "C"
