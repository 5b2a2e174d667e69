// C ABI of libmamdr_hip.so, the queries of a step-kernel context: evaluation of a split (mamdr_eval_domain), the gathered
// input rows (mamdr_gather_rows), top-K retrieval (mamdr_recommend(_domain)), the exact ranks of target items
// (mamdr_rank_domain) and per-query candidate slates (mamdr_rank_slates).  (The metrics of predictions: eval_metrics.hip.)
#include <algorithm>

#include "step_ctx.h"

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
    ta.loss_part = c->eval_part;
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
    fa.loss_part = c->eval_part;
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

// ---- top-K retrieval (recommend_kernels.hip)
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

// what both retrieval bodies do between their argument checks and their launches: tables brought up to date, the workspace
// for `chunk` candidates per pass, and the RecArgs fields that do not change inside the call
static int rec_prepare(mamdr_ctx* c, int32_t domain, const int32_t* d_cand, int64_t& n_cand, const int32_t* d_excl_ids,
                       RecArgs& a, int& chunk) {
    const bool per_query = domain < 0;
    if (!d_cand) n_cand = c->cfg.n_item;
    sync_tables(c);              // lagging table rows and lazily replayed per-domain slices: as mamdr_eval_domain
    prof_break(c);
    chunk = (int)std::min<int64_t>(c->rec_chunk, (n_cand + REC_TILE - 1) / REC_TILE * REC_TILE);
    if (int e = grow_rec_workspace(c, chunk)) return e;
    memset(&a, 0, sizeof(a));
    a.user_tab = c->cfg.emb_trainable ? c->params : c->user_tab;
    a.item_tab = c->cfg.emb_trainable ? c->params + (size_t)c->cfg.n_user * EMB : c->item_tab;
    a.dense = c->params + c->table_floats;
    a.L = c->L;
    a.dom_all = per_query ? -1 : domain;
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

// the body of both entry points: `domain` < 0 = mamdr_recommend (query q in d_domain[q]), otherwise every query in `domain`
static int recommend_body(mamdr_ctx* c, const char* fn, int32_t domain, int32_t n_query, const int32_t* d_uid,
                          const int32_t* d_domain, const int32_t* d_cand, int64_t n_cand, const int64_t* d_excl_off,
                          const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out, float* d_scores_out, float* d_scores_all) {
    const bool per_query = domain < 0;
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d must be positive", fn, n_query);
    if (k < 1 || k > REC_KMAX) return fail(MAMDR_EINVAL, "%s: k %d outside [1, %d]", fn, k, REC_KMAX);
    if (d_cand && n_cand <= 0) return fail(MAMDR_EINVAL, "%s: n_cand %lld with a candidate list given", fn, (long long)n_cand);
    if (!d_uid || (per_query && !d_domain) || !d_ids_out || !d_scores_out)
        return fail(MAMDR_EINVAL, per_query ? "%s: null uid / domain / output pointer" : "%s: null uid / output pointer", fn);
    if (misaligned(3, d_uid, d_domain, d_cand, d_excl_ids, d_ids_out, d_scores_out, d_scores_all) || misaligned(7, d_excl_off))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned to its element size", fn);
    if ((d_excl_off == nullptr) != (d_excl_ids == nullptr))
        return fail(MAMDR_EINVAL, "%s: the exclusion lists need both their offsets and their ids", fn);
    if (ready(c)) return MAMDR_ESTATE;
    RecArgs a;
    int chunk;
    if (int e = rec_prepare(c, domain, d_cand, n_cand, d_excl_ids, a, chunk)) return e;
    a.k = k;
    a.kt = std::min<int>(k, REC_TILE);
    for (int32_t qb = 0; qb < n_query; qb += REC_QBLOCK) {
        a.n_query = std::min<int32_t>(REC_QBLOCK, n_query - qb);
        a.uid = d_uid + qb;
        a.dom = per_query ? d_domain + qb : nullptr;
        a.excl_off = d_excl_off ? d_excl_off + qb : nullptr;
        a.ids_out = d_ids_out + (size_t)qb * k;
        a.scores_out = d_scores_out + (size_t)qb * k;
        a.scores_all = d_scores_all ? d_scores_all + (size_t)qb * n_cand : nullptr;
        launch_rec_query_proj(a, c->stream);
        for (int64_t c0 = 0; c0 < n_cand; c0 += chunk) {
            a.c_base = c0;
            a.n_chunk = (int)std::min<int64_t>(chunk, n_cand - c0);
            a.tiles = (a.n_chunk + REC_TILE - 1) / REC_TILE;
            a.first_chunk = c0 == 0;
            a.last_chunk = c0 + chunk >= n_cand;
            launch_rec_item_proj(a, c->stream);
            if (!launch_rec_score(a, c->stream))
                return fail(MAMDR_EHIP, "%s: k_rec_score was refused its LDS limit (hipFuncSetAttribute)", fn);
            launch_rec_merge(a, c->stream);
        }
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_recommend(mamdr_ctx* c, int32_t n_query, const int32_t* d_uid, const int32_t* d_domain, const int32_t* d_cand,
                    int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out,
                    float* d_scores_out, float* d_scores_all) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->star)
        return fail(MAMDR_ENOTBUILT, "mamdr_recommend: the star tower is not built for retrieval with a domain per query (its "
                                     "first layer separates into a query and an item term per domain only: "
                                     "mamdr_recommend_domain); mlp, wdl and deepfm are");
    if (c->pnn || c->nfm)
        return fail(MAMDR_ENOTBUILT, "mamdr_recommend: the %s tower is not built for retrieval (its first layer does not separate "
                                     "into a query and an item term); mlp, wdl and deepfm are", c->pnn ? "pnn" : "nfm");
    return recommend_body(c, "mamdr_recommend", -1, n_query, d_uid, d_domain, d_cand, n_cand, d_excl_off, d_excl_ids, k,
                          d_ids_out, d_scores_out, d_scores_all);
}

int mamdr_recommend_domain(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                           int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k,
                           int32_t* d_ids_out, float* d_scores_out, float* d_scores_all) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->pnn || c->nfm)
        return fail(MAMDR_ENOTBUILT, "mamdr_recommend_domain: the %s tower is not built for retrieval (its first layer does not "
                                     "separate into a query and an item term); mlp, wdl, deepfm and star are", c->pnn ? "pnn" : "nfm");
    if (domain < 0 || domain >= c->cfg.n_domain)
        return fail(MAMDR_EINVAL, "mamdr_recommend_domain: domain %d outside [0, %d)", domain, c->cfg.n_domain);
    return recommend_body(c, "mamdr_recommend_domain", domain, n_query, d_uid, nullptr, d_cand, n_cand, d_excl_off, d_excl_ids,
                          k, d_ids_out, d_scores_out, d_scores_all);
}

// the CSR offsets of a call's targets / slate entries (`what` names them in the errors) size its launches and its key
// workspace: read back once (the call's one synchronisation of the context's stream) and held to their contract here, so
// that no kernel indexes past the list
static int read_offsets(mamdr_ctx* c, const char* fn, const char* what, const int64_t* d_off, int32_t n_query,
                        std::vector<int64_t>& off) {
    off.resize((size_t)n_query + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), d_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (off[0] != 0) return fail(MAMDR_EINVAL, "%s: the %s offsets start at %lld, not 0", fn, what, (long long)off[0]);
    for (int32_t q = 0; q < n_query; ++q)
        if (off[q + 1] < off[q]) return fail(MAMDR_EINVAL, "%s: the %s offsets descend at query %d", fn, what, q);
    return MAMDR_OK;
}

// the key workspace (k_rec_pair's tkey) for n keys
static int grow_rec_tkey(mamdr_ctx* c, int64_t n) {
    if (n <= c->rec_tkey_cap) return MAMDR_OK;
    c->dev.release(c->rec_tkey);
    c->rec_tkey = nullptr;
    c->rec_tkey_cap = 0;
    c->dev.alloc(&c->rec_tkey, (size_t)n);
    if (const int rc = c->dev.check(g_err)) return rc;
    c->rec_tkey_cap = n;
    return MAMDR_OK;
}

// ---- exact ranks of target items among a candidate list: the retrieval phases with the counting ending
int mamdr_rank_domain(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                      int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                      const int32_t* d_tgt_ids, int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out) {
    const char* fn = "mamdr_rank_domain";
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->pnn || c->nfm)
        return fail(MAMDR_ENOTBUILT, "mamdr_rank_domain: the %s tower is not built for retrieval (its first layer does not "
                                     "separate into a query and an item term); mlp, wdl, deepfm and star are", c->pnn ? "pnn" : "nfm");
    if (domain < 0 || domain >= c->cfg.n_domain)
        return fail(MAMDR_EINVAL, "mamdr_rank_domain: domain %d outside [0, %d)", domain, c->cfg.n_domain);
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d must be positive", fn, n_query);
    if (d_cand && n_cand <= 0) return fail(MAMDR_EINVAL, "%s: n_cand %lld with a candidate list given", fn, (long long)n_cand);
    if (!d_uid || !d_tgt_off || !d_rank_out || !d_live_out)
        return fail(MAMDR_EINVAL, "%s: null uid / target offsets / rank / live output pointer", fn);
    if (misaligned(3, d_uid, d_cand, d_excl_ids, d_tgt_ids, d_rank_out, d_score_out, d_live_out) || misaligned(7, d_excl_off, d_tgt_off))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned to its element size", fn);
    if ((d_excl_off == nullptr) != (d_excl_ids == nullptr))
        return fail(MAMDR_EINVAL, "%s: the exclusion lists need both their offsets and their ids", fn);
    if (ready(c)) return MAMDR_ESTATE;
    std::vector<int64_t> off;
    if (int e = read_offsets(c, fn, "target", d_tgt_off, n_query, off)) return e;
    const int64_t n_tgt = off[n_query];
    if (n_tgt > 0 && !d_tgt_ids) return fail(MAMDR_EINVAL, "%s: %lld targets without their ids", fn, (long long)n_tgt);
    RecArgs a;
    int chunk;
    if (int e = rec_prepare(c, domain, d_cand, n_cand, d_excl_ids, a, chunk)) return e;
    if (int e = grow_rec_tkey(c, n_tgt)) return e;
    a.tkey = c->rec_tkey;
    a.tscore_out = d_score_out;
    a.rank_out = d_rank_out;
    if (n_tgt > 0) HIP_TRY(hipMemsetAsync(d_rank_out, 0, (size_t)n_tgt * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(d_live_out, 0, (size_t)n_query * sizeof(int32_t), c->stream));
    for (int32_t qb = 0; qb < n_query; qb += REC_QBLOCK) {
        a.n_query = std::min<int32_t>(REC_QBLOCK, n_query - qb);
        a.uid = d_uid + qb;
        a.excl_off = d_excl_off ? d_excl_off + qb : nullptr;
        a.tgt_off = d_tgt_off + qb;
        a.live_out = d_live_out + qb;
        launch_rec_query_proj(a, c->stream);
        // the block's target keys first: the item term of the flat target list, then the pair tiles
        a.cand = d_tgt_ids;
        for (int64_t t0 = off[qb]; t0 < off[qb + a.n_query]; t0 += c->rec_cap) {
            a.c_base = t0;
            a.n_chunk = (int)std::min<int64_t>(c->rec_cap, off[qb + a.n_query] - t0);
            launch_rec_item_proj(a, c->stream);
            if (!launch_rec_pair(a, c->stream))
                return fail(MAMDR_EHIP, "%s: k_rec_pair was refused its LDS limit (hipFuncSetAttribute)", fn);
        }
        a.cand = d_cand;
        for (int64_t c0 = 0; c0 < n_cand; c0 += chunk) {
            a.c_base = c0;
            a.n_chunk = (int)std::min<int64_t>(chunk, n_cand - c0);
            a.tiles = (a.n_chunk + REC_TILE - 1) / REC_TILE;
            launch_rec_item_proj(a, c->stream);
            if (!launch_rec_count(a, c->stream))
                return fail(MAMDR_EHIP, "%s: k_rec_score was refused its LDS limit (hipFuncSetAttribute)", fn);
        }
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

// ---- per-query candidate slates: mamdr_rank_domain's target pre-pass over the slates' entries, then the order inside
// each slate (k_slate_order).  No candidate pass: a slate is ranked against itself
int mamdr_rank_slates(mamdr_ctx* c, int32_t domain, int32_t n_query, const int32_t* d_uid, const int64_t* d_slate_off,
                      const int32_t* d_slate_ids, float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out) {
    const char* fn = "mamdr_rank_slates";
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->pnn || c->nfm)
        return fail(MAMDR_ENOTBUILT, "mamdr_rank_slates: the %s tower is not built for retrieval (its first layer does not "
                                     "separate into a query and an item term); mlp, wdl, deepfm and star are", c->pnn ? "pnn" : "nfm");
    if (domain < 0 || domain >= c->cfg.n_domain)
        return fail(MAMDR_EINVAL, "mamdr_rank_slates: domain %d outside [0, %d)", domain, c->cfg.n_domain);
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d must be positive", fn, n_query);
    if (!d_uid || !d_slate_off || !d_pos_out) return fail(MAMDR_EINVAL, "%s: null uid / slate offsets / position output pointer", fn);
    if (misaligned(3, d_uid, d_slate_ids, d_score_out, d_pos_out, d_order_out) || misaligned(7, d_slate_off))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned to its element size", fn);
    if (ready(c)) return MAMDR_ESTATE;
    std::vector<int64_t> off;
    if (int e = read_offsets(c, fn, "slate", d_slate_off, n_query, off)) return e;
    for (int32_t q = 0; q < n_query; ++q)
        if (off[q + 1] - off[q] > INT32_MAX)
            return fail(MAMDR_EINVAL, "%s: slate %d has %lld entries: positions are int32", fn, q, (long long)(off[q + 1] - off[q]));
    int64_t n_ent = off[n_query];
    if (n_ent == 0) return MAMDR_OK;
    if (!d_slate_ids) return fail(MAMDR_EINVAL, "%s: %lld entries without their ids", fn, (long long)n_ent);
    RecArgs a;
    int chunk;
    if (int e = rec_prepare(c, domain, d_slate_ids, n_ent, nullptr, a, chunk)) return e;
    if (int e = grow_rec_tkey(c, n_ent)) return e;
    a.tkey = c->rec_tkey;
    a.tscore_out = d_score_out;
    SlateArgs sa;
    sa.tkey = c->rec_tkey;
    sa.pos_out = d_pos_out;
    sa.order_out = d_order_out;
    if (d_order_out) HIP_TRY(hipMemsetAsync(d_order_out, 0xff, (size_t)n_ent * sizeof(int32_t), c->stream));
    for (int32_t qb = 0; qb < n_query; qb += REC_QBLOCK) {
        a.n_query = std::min<int32_t>(REC_QBLOCK, n_query - qb);
        if (off[qb + a.n_query] == off[qb]) continue;           // a block of empty slates
        a.uid = d_uid + qb;
        a.tgt_off = d_slate_off + qb;
        launch_rec_query_proj(a, c->stream);
        prof_break(c);
        // the block's keys: the item term of its entries, a workspace's worth at a time, then the pair tiles
        for (int64_t t0 = off[qb]; t0 < off[qb + a.n_query]; t0 += c->rec_cap) {
            a.c_base = t0;
            a.n_chunk = (int)std::min<int64_t>(c->rec_cap, off[qb + a.n_query] - t0);
            {
                Prof p(c, MAMDR_KERNEL_GATHER);
                launch_rec_item_proj(a, c->stream);
            }
            Prof p(c, MAMDR_KERNEL_EVAL);
            if (!launch_rec_pair(a, c->stream))
                return fail(MAMDR_EHIP, "%s: k_rec_pair was refused its LDS limit (hipFuncSetAttribute)", fn);
        }
        int64_t max_len = 0;
        bool any_short = false;
        for (int32_t q = qb; q < qb + a.n_query; ++q) {
            const int64_t len = off[q + 1] - off[q];
            max_len = std::max(max_len, len);
            any_short = any_short || (len >= 1 && len <= SLATE_WAVE);
        }
        sa.off = d_slate_off + qb;
        sa.n_query = a.n_query;
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_slate_order(sa, max_len, any_short, c->stream);
    }
    prof_break(c);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

}  // extern "C"
