// C ABI of libmamdr_hip.so (declared in include/mamdr_hip.h): the training call of the step kernels.
//
// Host-side state is tiny: bound pointers, the Adam step count with its fp32
// running beta powers (TF keeps them as beta1_power / beta2_power variables), the
// global inner-step counter that indexes the dropout stream, and a private
// workspace sized for max_batch.  Everything numeric runs in the kernels of
// step_kernels.hip / outer_kernels.hip on the context's stream.  The context itself, the queries and the stateless
// entry points live in step_context.hip, step_queries.hip, eval_metrics.hip and step_stateless.hip (map: step_ctx.h).
#include <algorithm>
#include <cmath>

#include "step_ctx.h"

void fill_tower_common(const mamdr_ctx* c, const SplitData& d, TowerArgs& a) {
    memset(&a, 0, sizeof(a));
    a.user_tab = c->cfg.emb_trainable ? c->params : c->user_tab;
    a.item_tab = c->cfg.emb_trainable ? c->params + (size_t)c->cfg.n_user * EMB : c->item_tab;
    a.dense = c->params + c->table_floats;
    a.L = c->L;
    a.n_user = c->cfg.n_user;
    a.n_item = c->cfg.n_item;
    a.n_domain = c->cfg.n_domain;
    a.uid = d.uid;
    a.pid = d.pid;
    a.dom = d.dom;
    a.label = d.label;
    a.n_rows_split = d.n;
    a.thresholds = c->thresholds;
    a.deepfm = c->nfm ? 4 : (c->deepfm ? (c->cfg.tower == MAMDR_TOWER_WDL ? 2 : 1) : (c->pnn ? 3 : 0));
    a.ipbuf = c->ipbuf;
    a.uw_off = -1;
    if (c->deepfm && c->cfg.emb_trainable) {
        a.lin_user = c->params + c->lin_user_off;
        a.lin_item = c->params + c->lin_item_off;
    }
}

// Star: the StarPrepArgs of domain `domain` for inference (its moving statistics and merged kernels); a training step
// adds its statistics' partials and sets `train`
void fill_star_prep(const mamdr_ctx* c, int domain, StarPrepArgs& pa) {
    memset(&pa, 0, sizeof(pa));
    pa.blk = c->params + c->table_floats;
    pa.SL = c->SL;
    pa.L = c->L;
    pa.n_domain = c->cfg.n_domain;
    pa.d = domain;
    pa.eff = c->eff;
    pa.pn = c->pn;
    pa.aux = c->aux;
    pa.AL = c->AL;
}

// trainable tables: the regulariser of a reported loss needs the current tables' sums of squares
void refresh_table_sumsq(mamdr_ctx* c) {
    launch_sumsq(c->params, (int64_t)c->cfg.n_user * EMB, c->sumsq_partials, c->frozen_sumsq + 0, c->stream);
    launch_sumsq(c->params + (size_t)c->cfg.n_user * EMB, (int64_t)c->cfg.n_item * EMB, c->sumsq_partials,
                 c->frozen_sumsq + 1, c->stream);
    if (c->deepfm) {
        launch_sumsq(c->params + c->lin_user_off, c->cfg.n_user, c->sumsq_partials, c->frozen_sumsq + 2, c->stream);
        launch_sumsq(c->params + c->lin_item_off, c->cfg.n_item, c->sumsq_partials, c->frozen_sumsq + 3, c->stream);
    }
}

// the optimiser sextet of a step: the kernel structs spell it out one by one under the same six names (OptArgsLite inside
// EmbStepArgs / StarUpdateArgs; FusedArgs, DmStep and UpdateArgs themselves)
template <typename T>
static void fill_opt(const mamdr_ctx* c, int32_t optimizer, float alpha, float omb1, float omb2, float two_l2, T& o) {
    o.optimizer = optimizer;
    o.alpha = alpha;
    o.omb1 = omb1;
    o.omb2 = omb2;
    o.eps = c->cfg.adam_eps;
    o.two_l2 = two_l2;
}


// ---- trainable user / item tables: shared by the mlp / deepfm and the Star step
// (no regulariser on the Star tower's tables; its row gradients come 384 wide)
static void fill_emb_args(const mamdr_ctx* c, int32_t optimizer, float alpha, float omb1, float omb2, int rows, EmbStepArgs& ea) {
    memset(&ea, 0, sizeof(ea));
    float* slot_m = optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m;
    ea.p = c->params;
    ea.m = slot_m;
    ea.v = c->adam_v;
    ea.dxe = c->dxe;
    ea.dx_ld = c->star ? XDIM : 2 * EMB;
    ea.dlogit = c->dlogit;
    ea.rows = rows;
    ea.two_l2_lin = 2.0f * c->cfg.l2_linear;
    fill_opt(c, optimizer, alpha, omb1, omb2, c->star ? 0.f : 2.0f * c->cfg.l2_emb, ea.opt);
    ea.alpha_log = c->alpha_log;
    ea.log_mask = c->log_cap - 1;
    ea.t_now = (int)c->adam_t;
    EmbTable& tu = ea.t[0];
    EmbTable& ti = ea.t[1];
    tu.n_rows = c->cfg.n_user;
    tu.brow = c->urow;
    tu.map = c->map_u;
    tu.gbuf = c->gbuf_u;
    tu.hasdup = c->hasdup_u;
    tu.last = c->last_u;
    tu.dx_off = 0;
    ti.n_rows = c->cfg.n_item;
    ti.brow = c->irow;
    ti.map = c->map_i;
    ti.gbuf = c->gbuf_i;
    ti.hasdup = c->hasdup_i;
    ti.last = c->last_i;
    ti.dx_off = EMB;
    if (c->deepfm) {
        tu.lin_p = c->params + c->lin_user_off;
        tu.lin_m = slot_m + c->lin_user_off;
        tu.lin_v = c->adam_v + c->lin_user_off;
        tu.glin = c->glin_u;
        ti.lin_p = c->params + c->lin_item_off;
        ti.lin_m = slot_m + c->lin_item_off;
        ti.lin_v = c->adam_v + c->lin_item_off;
        ti.glin = c->glin_i;
    }
}


// materialise a domain-table step the k_wgrad_adam path left pending
void finish_dm(mamdr_ctx* c) {
    if (!c->dm_pending.snap) return;
    float* const m = (c->dm_pending.optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m) + c->table_floats + c->L.dm;
    {
        Prof p(c, MAMDR_KERNEL_UPDATE);
        launch_dm_finish(c->dm_pending, c->params + c->table_floats + c->L.dm, m, c->adam_v + c->table_floats + c->L.dm,
                         c->stream);
    }
    c->dm_pending.snap = nullptr;
}

// the live state current and about to be read or replaced from outside: the pending domain-table step applied, every
// table row at adam_t (no-op when nothing lags); the transposed weight copies can no longer be trusted
void sync_tables(mamdr_ctx* c) {
    finish_dm(c);
    c->wT_valid = false;
    if (!c->tables_dirty) return;
    EmbStepArgs ea;
    fill_emb_args(c, MAMDR_OPT_ADAM, 0.f, 1.0f - c->cfg.adam_beta1, 1.0f - c->cfg.adam_beta2, 0, ea);
    {
        Prof p(c, MAMDR_KERNEL_FLUSH);
        launch_emb_flush(ea, c->stream);
    }
    c->tables_dirty = false;
    c->flush_t = c->adam_t;
    c->n_flush += 1;
}

// k_emb_rows arguments of the batch at row_base for Adam step `t` (alt: into the other half of the double buffer)
static void fill_rows_args(const mamdr_ctx* c, const SplitData& d, const int32_t* d_perm, int64_t row_base, int rows,
                           int rows_pad, float alpha, int64_t t, bool alt, EmbRowsArgs& ra) {
    memset(&ra, 0, sizeof(ra));
    ra.uid = d.uid;
    ra.pid = d.pid;
    ra.perm = d_perm;
    ra.row_base = row_base;
    ra.n_rows_split = d.n;
    ra.rows = rows;
    ra.rows_pad = rows_pad;
    ra.n_user = c->cfg.n_user;
    ra.n_item = c->cfg.n_item;
    ra.urow = alt ? c->urow_alt : c->urow;
    ra.irow = alt ? c->irow_alt : c->irow;
    ra.map_u = alt ? c->map_u_alt : c->map_u;
    ra.map_i = alt ? c->map_i_alt : c->map_i;
    ra.alpha_log = c->alpha_log;
    ra.log_idx = (int)(t & (c->log_cap - 1));
    ra.alpha = alpha;
}

// lazy mode, before the tower of Adam step adam_t (already incremented): row ids + representatives of the
// batch, alpha of this step into the ring, rows of the batch brought up to adam_t - 1
static void emb_pre_step(mamdr_ctx* c, const SplitData& d, const int32_t* d_perm, int64_t row_base, int rows,
                         int rows_pad, float alpha, float omb1, float omb2) {
    // the ring must not wrap over a lagging row's range; and a bounded gap keeps the per-row serial replay of
    // k_emb_catchup short (the flush replays the same steps at full occupancy)
    if (c->adam_t - c->flush_t >= c->log_cap - 2 || c->adam_t - c->flush_t > c->flush_every) {
        c->adam_t -= 1;
        if (c->tables_dirty) c->n_flush_forced += 1;
        sync_tables(c);
        c->adam_t += 1;
    }
    if (!c->rows_ready) {
        EmbRowsArgs ra;
        fill_rows_args(c, d, d_perm, row_base, rows, rows_pad, alpha, c->adam_t, false, ra);
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_emb_rows(ra, c->stream);
    }
    c->rows_ready = false;
    if (!c->catchup_ready) {
        EmbStepArgs ea;
        fill_emb_args(c, MAMDR_OPT_ADAM, alpha, omb1, omb2, rows, ea);
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_emb_catchup(ea, c->stream);
    }
    c->catchup_ready = false;
    c->tables_dirty = true;
}

// after the tower / wgrad: scatter-add of the row gradients and the optimiser on the tables
static void emb_post_step(mamdr_ctx* c, int32_t optimizer, float alpha, float omb1, float omb2, int rows) {
    EmbStepArgs ea;
    fill_emb_args(c, optimizer, alpha, omb1, omb2, rows, ea);
    if (c->lazy && optimizer == MAMDR_OPT_ADAM) {
        // duplicates were flagged by the catch-up kernel; the reducing workgroup applies the step itself
        ea.flags_done = 1;
        ea.apply_now = 1;
        {
            Prof p(c, MAMDR_KERNEL_EMB_SWEEP);
            launch_emb_reduce(ea, c->stream);
        }
        if (c->deepfm) {
            Prof p(c, MAMDR_KERNEL_AUX);
            launch_lin_sweep(ea, c->stream);     // reads the row maps, then releases them
        }
        return;
    }
    launch_emb_reduce(ea, c->stream);
    prof_break(c);
    {
        Prof p(c, MAMDR_KERNEL_EMB_SWEEP);
        launch_emb_sweep(ea, c->stream);
    }
    if (c->deepfm) {
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_lin_sweep(ea, c->stream);
    }
}

// ---- the decisions of a training call, each made in one place (mamdr_step_path / mamdr_tower_tile report the same ones)
// a step's rows padded to whole 16-row tiles
int64_t pad_rows(int64_t rows) { return (rows + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS; }
// rows of the batch at row_base of a pass of pass_rows rows (the last batch of a pass may be short)
static int rows_at(int64_t pass_rows, int64_t row_base, int batch) { return (int)std::min<int64_t>(batch, pass_rows - row_base); }
// one path per call (the pending domain-table step lives across the steps of a call): k_wgrad_adam for batches up to
// fused_max_batch rows (measured: 27.3 vs 29.5 us / step at 1,024 rows, a tie at 4,096), k_wgrad -> slabs -> k_update above
bool takes_fused_path(const mamdr_ctx* c, int64_t batch) { return c->fused && pad_rows(batch) <= c->fused_max_batch; }
// forget every pass gathered ahead of its call, and the window the riders are working on
void drop_pregathered(mamdr_ctx* c) {
    c->pg.clear();
    c->ahead.on = false;
}
// rider workgroups a k_wgrad_adam launch can carry: the CUs its own workgroups leave idle (none on a smaller part)
static int ride_wgs(const mamdr_ctx* c, bool with_loss) {
    return std::max(0, std::min(FZ_RIDE_CAP, c->n_cu - wgrad_adam_own_wgs(with_loss)));
}
// small steps run the 4-row-tile tower (all CUs busy), the others the 16-row one (the only one of the Star tower)
bool takes_tower4(const mamdr_ctx* c, int64_t rows_pad) {
    return !c->star && c->tower_tile != 16 && (c->tower_tile == 4 || rows_pad <= c->tower4_max_rows);
}
// every k_tower4 launch this context can make reads W1 from its LDS image: the largest batch that tower takes (tile 4
// forced: any batch the context accepts) still fits one round of workgroups
bool w1t_unread_now(const mamdr_ctx* c) {
    if (!c->fused || c->tower_tile == 16) return false;
    const int64_t max4 = c->tower_tile == 4 ? c->rows_pad_max : std::min<int64_t>(c->tower4_max_rows, c->rows_pad_max);
    return tower4_never_streams(max4, c->t4_no_w1l);
}
// ... and every training call takes the k_wgrad_adam path over a pre-gathered pass, so that each of those launches can
// be the instance that reads W2 in place: no batch the context accepts goes to the slab path (whose towers read W2T)
bool w2t_unread_now(const mamdr_ctx* c) {
    return w1t_unread_now(c) && c->w2_direct_ok && c->use_pre && takes_fused_path(c, c->rows_pad_max);
}
// row groups of k_wgrad (= gradient slabs) of a step and the rows of each (measured: 1024 rows, 8 groups of 128: 31.0 us /
// step vs 32.0 with 4 of 256; batches of <= 512 rows keep 256-row groups: one or two slabs)
static int wgrad_groups(int rows_pad, int* rpg) {
    int r = rows_pad <= 512 ? 256 : (rows_pad <= 1024 ? 128 : (rows_pad <= 4096 ? 256 : 512));
    int groups = (rows_pad + r - 1) / r;
    if (groups > WGRAD_MAX_GROUPS) {
        r = ((rows_pad + WGRAD_MAX_GROUPS - 1) / WGRAD_MAX_GROUPS + 7) / 8 * 8;
        groups = (rows_pad + r - 1) / r;
    }
    *rpg = r;
    return groups;
}
// TF1 Adam's step size from the running beta powers
static float adam_alpha(float lr, float b1p, float b2p) { return lr * sqrtf(1.0f - b2p) / (1.0f - b1p); }
// the counters of the step about to run: Adam's step count and fp32 beta powers advance; returns the step's alpha (lr
// for SGD / accumulate)
static float advance_step(mamdr_ctx* c, int32_t optimizer, float lr) {
    if (optimizer != MAMDR_OPT_ADAM) return lr;
    c->adam_t += 1;
    c->b1p = c->b1p * c->cfg.adam_beta1;
    c->b2p = c->b2p * c->cfg.adam_beta2;
    return adam_alpha(lr, c->b1p, c->b2p);
}

// one mamdr_train_steps_n call: its arguments, then what is decided for it once, before its first launch (plan_call)
enum class StepPath { star, fused, slab };
struct CallPlan {
    const SplitData* d;
    int domain;
    const int32_t* perm;
    int64_t pass_rows, first_step, n_steps;
    int batch;
    int32_t optimizer;
    float lr, omb1, omb2;
    float* loss_out;            // nullable: [n_steps] the loss of every step
    uint32_t seed, drop_thresh;
    float keep_scale;
    int use_dropout;
    StepPath path = StepPath::slab;
    // lazy table Adam with fused tails: the table kernels ride in the dense launches, and the NEXT step's k_emb_rows /
    // k_emb_catchup in this step's (profiling runs keep them apart for per-kernel times; a reported loss reads the tables
    // between the two and keeps them apart too)
    bool tail = false;
    bool pre = false;           // k_wgrad_adam path: the rows of the whole call resolved and gathered once (k_pass_prep)
    bool pre_cached = false;    // ... by mamdr_pregather_passes ahead of the call: row pre_pos0 sits at pre_base
    int64_t pre_pos0 = 0, pre_n = 0, pre_base = 0;
    bool need_wT = false;       // a step of the call runs k_tower4, which reads the transposed W1 / W2 copies
    bool build_wT = false;      // ... which are built at the start of the call
    bool w2_direct = false;     // ... or not: the call's first tower reads W2 in place
    bool w2_all = false;        // ... as every tower of the call does (w2t_unread_now): the W2 copy is left alone
    bool star_lazy = false;     // Star: the other domains' slices are replayed by k_star_catchup, not stepped every step
};

static void plan_call(mamdr_ctx* c, CallPlan& P) {
    P.path = c->star ? StepPath::star : (takes_fused_path(c, P.batch) ? StepPath::fused : StepPath::slab);
    const bool fused = P.path == StepPath::fused;
    const bool accumulate = P.optimizer == MAMDR_OPT_ACCUMULATE;
    P.tail = c->tail_fuse && c->cfg.emb_trainable && c->lazy && P.optimizer == MAMDR_OPT_ADAM && !c->profile && !P.loss_out;
    const int first_rows = rows_at(P.pass_rows, P.first_step * P.batch, P.batch);
    // the four-row tower needs transposed W1 / W2 copies: refreshed at the start of a call because the caller may have
    // assigned new weights, kept current by k_update -- only when a step of THIS call is small enough for that tower (the
    // rows of a pass's steps never grow: the last one is the smallest); a 4,096-row call over a domain without a short last
    // batch needs no copies at all
    P.need_wT = takes_tower4(c, pad_rows(rows_at(P.pass_rows, (P.first_step + P.n_steps - 1) * P.batch, P.batch)));
    // on the k_wgrad_adam path the rows of the whole call are resolved and gathered once (frozen tables; 4-row tower)
    P.pre_pos0 = P.first_step * P.batch;
    P.pre_n = std::min<int64_t>((P.first_step + P.n_steps) * P.batch, P.pass_rows) - P.pre_pos0;
    P.pre = fused && c->use_pre && P.pre_n > 0;
    // the transposed copies: built at the start of the call unless the previous call's steps left them current (no
    // sync_tables since).  On the k_wgrad_adam path with the W1 image (k_tower4<.., W1L, PRE>) only W2T is read, and only
    // the call's FIRST tower can find it stale -- k_wgrad_adam rewrites every copy a tower can read with the step -- so
    // that tower reads W2 itself (w2_direct: 32 B runs of 128 rows, four loads per lane) and nothing is transposed at all
    P.build_wT = P.need_wT && !c->wT_valid;
    if (P.build_wT && P.pre && c->w2_direct_ok && !accumulate && !c->t4_no_w1l && c->tower_tile != 16 && tower4_w1l_ready() &&
        tower4_takes_w1l(first_rows, c->t4_no_w1l)) {
        P.build_wT = false;
        P.w2_direct = true;
    }
    // ... and in a context all of whose towers are W1-image instances over pre-gathered rows (w2t_unread_now) EVERY tower
    // of the call reads W2 in place, whether the copies are current or not and in accumulate calls too: nothing is built,
    // k_wgrad_adam leaves W2T alone as it does W1T, and the call leaves the copies stale (wT_valid, mamdr_train_steps_n)
    if (P.need_wT && P.pre && c->w2t_unread) {
        P.build_wT = false;
        P.w2_direct = P.w2_all = true;
    }
    // ... and a call whose FIRST step runs the 16-row tower (which reads no copy) needs none built either: k_update
    // rewrites the copy of every element it steps, so they are current from the call's second step on -- before the
    // short last batch that runs the four-row tower
    if (P.build_wT && !accumulate && !fused && !c->star && !takes_tower4(c, pad_rows(first_rows)) && P.n_steps > 1)
        P.build_wT = false;
    // ... unless mamdr_pregather_passes gathered this pass ahead of the call: entries are consumed in order (an entry
    // stays current while calls keep working on its pass); a call that matches none drops them all
    if (P.pre) {
        for (size_t k = c->pg_pos; k < c->pg.size(); ++k) {
            const mamdr_ctx::PgEntry& e = c->pg[k];
            if (e.domain == P.domain && e.perm == P.perm && e.n == P.pass_rows && e.batch == P.batch) {
                c->pg_pos = k;
                P.pre_base = e.off + P.pre_pos0;
                P.pre_cached = true;
                c->pg_hits += 1;
                break;
            }
        }
        if (!P.pre_cached) drop_pregathered(c);
    }
    // Star tower: a batch carries one domain, so D - 1 of the D slices of every per-domain tensor see a zero gradient
    // and only decay -- TF1's dense Adam still moves them every step (star_kernels.hip).  Inside a call those steps are
    // postponed: k_star_update covers the live slice only and logs the step's alpha, k_star_catchup replays the
    // skipped steps when the call ends (the same arithmetic in the same order: bit-identical; one sweep of the 13
    // slices per call instead of one per step).  Calls of a single step gain nothing and sweep as before.
    P.star_lazy = c->star && P.optimizer == MAMDR_OPT_ADAM && P.n_steps >= 2 && !P.loss_out && !c->star_dense_slices &&
                  c->cfg.n_domain > 1;
}

// the NEXT step of this call (Adam step adam_t + 1, its batch at row_base), lazy table Adam with fused tails: its row ids
// and maps are resolved into the alternate buffers in this step's k_wgrad launch (nr), its catch-up runs in this step's
// last launch (nea)
static void fill_next_step(const mamdr_ctx* c, const CallPlan& P, int64_t row_base, EmbRowsArgs& nr, EmbStepArgs& nea) {
    const int rows = rows_at(P.pass_rows, row_base, P.batch);
    const float alpha = adam_alpha(P.lr, c->b1p * c->cfg.adam_beta1, c->b2p * c->cfg.adam_beta2);
    fill_rows_args(c, *P.d, P.perm, row_base, rows, (int)pad_rows(rows), alpha, c->adam_t + 1, true, nr);
    fill_emb_args(c, MAMDR_OPT_ADAM, alpha, P.omb1, P.omb2, rows, nea);
    nea.t_now = (int)c->adam_t + 1;
    nea.t[0].brow = c->urow_alt;
    nea.t[0].map = c->map_u_alt;
    nea.t[1].brow = c->irow_alt;
    nea.t[1].map = c->map_i_alt;
}

// ... and once those launches are issued, the alternate buffers hold the rows of the step about to run, caught up
static void take_next_rows(mamdr_ctx* c) {
    std::swap(c->urow, c->urow_alt);
    std::swap(c->irow, c->irow_alt);
    std::swap(c->map_u, c->map_u_alt);
    std::swap(c->map_i, c->map_i_alt);
    c->rows_ready = true;
    c->catchup_ready = true;
    c->tables_dirty = true;
}

// the WgradArgs fields that the Star step and the slab path's step fill alike, over the dense block the step's tower read
// (the live one, or Star's effective block); the caller adds what differs.  -> the step's row groups (= gradient slabs)
static int fill_wgrad_common(const mamdr_ctx* c, const float* dense, int rows, int rows_pad, float* loss_out, WgradArgs& wa) {
    memset(&wa, 0, sizeof(wa));
    wa.acts = c->acts;
    wa.dz = c->dz;
    wa.dlogit = c->dlogit;
    wa.domrow = c->domrow;
    wa.tiles = c->tiles;
    wa.n_tiles = c->n_tiles;
    wa.rows_pad = rows_pad;
    int rpg = 0;
    const int groups = wgrad_groups(rows_pad, &rpg);
    wa.n_groups = groups;
    wa.rows_per_group = rpg;
    wa.slabs = c->slabs;
    wa.slab_ld = c->slab_ld;
    wa.w0dom = dense + c->L.w0 + (size_t)(2 * EMB) * H1;
    wa.w0dom_copy = c->w0dom_copy;
    wa.loss_part = c->loss_part;
    wa.rows = rows;
    wa.dense = dense;
    wa.frozen_sumsq = c->frozen_sumsq;
    wa.loss_out = loss_out;
    return groups;
}

// ---- Star tower: step s of a call (star.py:70-97; kernels in star_kernels.hip)
static int star_step(mamdr_ctx* c, const CallPlan& P, int64_t s, float alpha) {
    const SplitData& d = *P.d;
    const int domain = P.domain;
    const int32_t optimizer = P.optimizer;
    const float omb1 = P.omb1, omb2 = P.omb2;
    float* const loss_out = P.loss_out ? P.loss_out + s : nullptr;
    const int64_t row_base = (P.first_step + s) * P.batch;
    const int rows = rows_at(P.pass_rows, row_base, P.batch);
    const int rows_pad = (int)pad_rows(rows);
    const int chunks = (rows + STAR_CHUNK - 1) / STAR_CHUNK;
    // lazy slices: only slice `domain` of the per-domain tensors is stepped and the step's alpha is logged at lazy_idx
    const int lazy_idx = (int)(s & (STAR_ALPHA_CAP - 1));
    const bool next = P.tail && s + 1 < P.n_steps;
    EmbRowsArgs nr;
    EmbStepArgs nea;
    if (next) fill_next_step(c, P, row_base + P.batch, nr, nea);
    float* blk = c->params + c->table_floats;
    TowerArgs ta;
    fill_tower_common(c, d, ta);
    ta.perm = P.perm;
    ta.row_base = row_base;
    ta.rows = rows;
    ta.batch = rows;
    if (c->cfg.emb_trainable && c->lazy && optimizer == MAMDR_OPT_ADAM)
        emb_pre_step(c, d, P.perm, row_base, rows, rows_pad, alpha, omb1, omb2);
    StarPrepArgs pa;
    fill_star_prep(c, domain, pa);
    pa.part = c->star_part;
    pa.n_chunks = chunks;
    pa.rows = rows;
    pa.train = 1;
    pa.skip_eff = P.star_lazy && s > 0 ? 1 : 0;     // (the previous step of this call wrote it: k_star_update, eff_out)
    {
        Prof p(c, MAMDR_KERNEL_AUX);            // k_star_stats + k_star_prep as one timed group
        // forward statistics read the raw rows (domain table straight from the flat vector: SL.dm == L.dm == 0)
        launch_star_stats(ta, c->star_part, c->aux + c->AL.steps + domain, c->stream);
        launch_star_prep(pa, c->stream);
    }

    ta.dense = c->eff;
    ta.pn_aff = c->pn;
    ta.pn_part = c->star_part;    // PartitionedNorm backward: per-tile sums in the tower's tail
    ta.use_dropout = 0;
    ta.keep_scale = 1.0f;
    ta.acts = c->acts;
    ta.dz = c->dz;
    ta.dlogit = c->dlogit;
    ta.domrow = c->domrow;
    ta.dxe = c->dxe;
    ta.dx_ld = XDIM;
    ta.urow = c->urow;
    ta.irow = c->irow;
    ta.map_u = c->map_u;          // null with frozen tables
    ta.map_i = c->map_i;
    ta.loss_part = c->loss_part;
#ifdef MAMDR_STAMPS
    ta.stamps = c->stamps;
#endif
    {
        Prof p(c, MAMDR_KERNEL_FWD_BWD);
        launch_tower_train(ta, c->stream);
    }
    WgradArgs wa;
    const int groups = fill_wgrad_common(c, c->eff, rows, rows_pad, loss_out, wa);
    wa.n_loss_tiles = rows_pad / TILE_ROWS;
    wa.dm_count = 0;              // no regularisers in this tower: loss = mean BCE
    wa.l2_emb = 0.f;
    StarPnBwdArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.user_tab = ta.user_tab;
    ba.item_tab = ta.item_tab;
    ba.dm_row = blk + c->SL.dm + (size_t)domain * EMB;
    ba.urow = c->urow;
    ba.irow = c->irow;
    ba.rows = rows;
    ba.n_chunks = chunks;
    ba.dxe = c->dxe;
    ba.pn = c->pn;
    ba.part = c->star_part;
    ba.sums = c->star_sums;
    ba.dmpart = c->star_dmpart;
    ba.dmsum = c->star_sums + 2 * XDIM;
    ba.means = c->star_sums + 2 * XDIM + EMB;
    // lazy table Adam with fused tails: PartitionedNorm's backward first (it only needs the tower's outputs), then
    // [k_wgrad + k_emb_reduce(t) + k_emb_rows(t+1)], then [k_star_update + k_emb_catchup(t+1)]
    // ... and (round 6) without k_star_pnb_apply when a catch-up launch follows: the table rows take PartitionedNorm's
    // backward inside k_emb_reduce, the domain columns' partial sums ride in k_wgrad_reduce and are finished and stepped
    // in k_star_update_catchup (StarPnBwdArgs::fused == 2; the same roundings in the same order as the launch it replaces)
    const bool no_apply = next;
    ba.fused = no_apply ? 2 : 0;
    if (P.tail) {
        {
            Prof p(c, MAMDR_KERNEL_AUX);
            launch_star_pn_bwd(ba, false, c->stream);   // (its last kernel, the domain-row column sums, rides below)
        }
        EmbStepArgs tea;
        fill_emb_args(c, optimizer, alpha, omb1, omb2, rows, tea);
        tea.flags_done = 1;
        tea.apply_now = 1;
        if (no_apply) {
            tea.pn_sums = c->star_sums;
            tea.pn_means = c->star_sums + 2 * XDIM + EMB;
            tea.pn = c->pn;
        }
        Prof p(c, MAMDR_KERNEL_WGRAD);
        launch_wgrad_reduce(wa, tea, next ? &nr : nullptr, &ba, c->stream);
    } else {
        {
            Prof p(c, MAMDR_KERNEL_WGRAD);
            launch_wgrad(wa, c->stream);
        }
        Prof p(c, MAMDR_KERNEL_AUX);                  // PartitionedNorm's backward: 4 launches as one timed group
        launch_star_pn_bwd(ba, true, c->stream);
    }

    float* slot_m = optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m;
    StarUpdateArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.p = blk;
    ua.m = slot_m + c->table_floats;
    ua.v = c->adam_v + c->table_floats;
    ua.SL = c->SL;
    ua.L = c->L;
    ua.n_domain = c->cfg.n_domain;
    ua.d = domain;
    ua.slabs = c->slabs;
    ua.n_groups = groups;
    ua.slab_ld = c->slab_ld;
    ua.sums = c->star_sums;
    ua.dmsum = c->star_sums + 2 * XDIM;
    ua.xdom = c->lin_w0dom ? c->pn + PN_XDOM_OFF : nullptr;
    fill_opt(c, optimizer, alpha, omb1, omb2, 0.f, ua.opt);
    if (P.star_lazy) {
        ua.only_live = 1;
        ua.alpha_log = c->star_alpha;
        ua.log_idx = lazy_idx;
        if (s + 1 < P.n_steps) ua.eff_out = c->eff;
    }
    {
        Prof p(c, MAMDR_KERNEL_UPDATE);
        ua.dm_elsewhere = no_apply ? 1 : 0;
        if (next) launch_star_update_catchup(ua, nea, no_apply ? &ba : nullptr, c->stream);
        else launch_star_update(ua, c->stream);
    }
    if (next) take_next_rows(c);
    if (c->cfg.emb_trainable && !P.tail) emb_post_step(c, optimizer, alpha, omb1, omb2, rows);
    c->global_step += 1;
    // the other slices catch up: alpha log full / call over
    if (P.star_lazy && (lazy_idx + 1 == STAR_ALPHA_CAP || s + 1 == P.n_steps)) {
        StarCatchArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.p = c->params + c->table_floats;
        ca.m = c->adam_m + c->table_floats;
        ca.v = c->adam_v + c->table_floats;
        ca.SL = c->SL;
        ca.n_domain = c->cfg.n_domain;
        ca.d_live = domain;
        ca.alpha_log = c->star_alpha;
        ca.first_idx = 0;
        ca.n_steps = lazy_idx + 1;
        ca.log_mask = STAR_ALPHA_CAP - 1;
        ca.omb1 = omb1;
        ca.omb2 = omb2;
        ca.eps = c->cfg.adam_eps;
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_star_catchup(ca, c->stream);
    }
    return MAMDR_OK;
}

// ---- the mlp-family towers (mlp / deepfm / wdl / pnn / nfm): the tower launch of step s, shared by both paths
static void fill_step_tower(const mamdr_ctx* c, const CallPlan& P, int64_t row_base, int rows, TowerArgs& ta) {
    fill_tower_common(c, *P.d, ta);
    ta.perm = P.perm;
    ta.row_base = row_base;
    ta.rows = rows;
    ta.batch = rows;
    ta.seed = P.seed;
    ta.step = c->global_step;
    ta.drop_thresh = P.drop_thresh;
    ta.keep_scale = P.keep_scale;
    ta.use_dropout = P.use_dropout;
    ta.acts = c->acts;
    ta.dz = c->dz;
    ta.dlogit = c->dlogit;
    ta.domrow = c->domrow;
    ta.dxe = c->dxe;
    ta.dx_ld = 2 * EMB;
    ta.urow = c->urow;
    ta.irow = c->irow;
    ta.map_u = c->map_u;
    ta.map_i = c->map_i;
    ta.loss_part = c->loss_part;
    ta.fmq = c->fmq;
    if (c->L.lv_count > 0) ta.uw_off = c->L.lv + P.domain;
#ifdef MAMDR_STAMPS
    ta.stamps = c->stamps ? c->stamps + (c->global_step & 1) * 16384 : nullptr;      // two steps side by side
#endif
    ta.wT = c->wT;
    ta.no_w1l = c->t4_no_w1l;
}

static int run_step_tower(mamdr_ctx* c, const TowerArgs& ta, bool use4, int64_t s) {
    if ((c->pnn || c->nfm) && !use4)
        return fail(MAMDR_ENOTBUILT, "pnn / nfm tower: a training step of %d rows needs the four-row tower (MAMDR_TOWER_TILE=16?)", ta.rows);
    Prof p(c, MAMDR_KERNEL_FWD_BWD);
#ifdef MAMDR_TOWER_TWICE
    // diagnostic build (tools/stamp_tower.py with MAMDR_DIAG_FLAGS=-DMAMDR_TOWER_TWICE): the same tower launch twice in a
    // row -- idempotent (the pending domain-table step is formed from its snapshot, every output is overwritten) -- so that
    // the stamps of the SECOND launch show the kernel with its own code and data still where the first left them
    if (use4) (void)launch_tower4_train(ta, c->stream);
#endif
    const int t4e = use4 ? launch_tower4_train(ta, c->stream) : (launch_tower_train(ta, c->stream), 0);
    if (t4e == T4_E_W2D_LDS) return fail(MAMDR_EHIP, "k_tower4<W2D> was refused its LDS limit (hipFuncSetAttribute)");
    if (t4e) return fail(MAMDR_ESTATE, "w2_direct without the W1-image instance of k_tower4 (step %lld of the call)", (long long)s);
    return MAMDR_OK;
}

// the riders of one k_wgrad_adam launch: the next slice of the announced window (pregather_plan.h), one rider per
// FZ_RIDE_ROWS positions, into the ahead set of the pass buffer
static void attach_riders(mamdr_ctx* c, FusedArgs& fa) {
    mamdr_ctx::Ahead& h = c->ahead;
    const int riders = ride_wgs(c, fa.loss_out != nullptr);
    if (riders <= 0) return;
    const PrePlanSlice sl = pre_plan_next(h.rows.data(), (int)h.rows.size(), h.cur, (int64_t)riders * FZ_RIDE_ROWS);
    if (sl.count() <= 0) return;
    RideArgs& g = fa.ride;
    g.user_tab = c->user_tab;
    g.item_tab = c->item_tab;
    g.xpre = c->xpre_ahead;
    g.pdom = c->pdom_ahead;
    g.plabel = c->plabel_ahead;
    g.n_user = c->cfg.n_user;
    g.n_item = c->cfg.n_item;
    g.n_wg = (int)((sl.count() + FZ_RIDE_ROWS - 1) / FZ_RIDE_ROWS);
    for (int k = 0; k < sl.n_seg; ++k) {
        const PassPrepMultiArgs::Pass& p = h.args.p[sl.seg[k].pass];
        RideArgs::Seg& q = g.seg[k];
        q.uid = p.uid;
        q.pid = p.pid;
        q.dom = p.dom;
        q.label = p.label;
        q.perm = p.perm;
        q.out_off = p.out_off;
        q.n = (int)p.n;                          // (a split holds at most 2^31 - 1 rows: mamdr_bind_domain_data)
        q.n_rows_split = (int)p.n_rows_split;
        q.first = (int)sl.seg[k].first;
        q.count = (int)sl.seg[k].count;
        q.pad_dom = p.pad_dom;
    }
    c->pg_rider_rows += sl.count();
}

// ---- k_wgrad_adam path (frozen-table mlp): tower + weight gradients and optimiser step in one launch; the domain table's
// step stays pending (DmStep): the next step's tower kernel applies it
static int fused_step(mamdr_ctx* c, const CallPlan& P, int64_t s, float alpha) {
    const int32_t optimizer = P.optimizer;
    const int64_t row_base = (P.first_step + s) * P.batch;
    const int rows = rows_at(P.pass_rows, row_base, P.batch);
    const int rows_pad = (int)pad_rows(rows);
    const bool use4 = takes_tower4(c, rows_pad);
    DmStep& dm_pending = c->dm_pending;
    float* const dense_m = (optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m) + c->table_floats;
    TowerArgs ta;
    fill_step_tower(c, P, row_base, rows, ta);
    c->dm_cur ^= 1;
    ta.dms = dm_pending;                       // the previous step of this call (snap == null: none)
    ta.dm_hint = P.domain;
    if (P.pre) {
        const int64_t at = P.pre_base + row_base - P.pre_pos0;
        ta.xpre = c->xpre + (size_t)at * 2 * EMB;
        ta.pdom = c->pdom + at;
        ta.plabel = c->plabel + at;
    }
    ta.dm_live_p = c->params + c->table_floats + c->L.dm;
    ta.dm_live_m = dense_m + c->L.dm;
    ta.dm_live_v = c->adam_v + c->table_floats + c->L.dm;
    ta.dm_snap_out = c->dmsnap[c->dm_cur];
    ta.w2_direct = (P.w2_direct && (s == 0 || P.w2_all) && use4) ? 1 : 0;
    if (int rc = run_step_tower(c, ta, use4, s)) return rc;
    FusedArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.acts = c->acts;
    fa.dz = c->dz;
    fa.dlogit = c->dlogit;
    fa.domrow = c->domrow;
    fa.xa = ta.xpre ? ta.xpre : c->acts;
    fa.xa_ld = ta.xpre ? 2 * EMB : ACT_LD;
    fa.rows_pad = rows_pad;
    fa.rows = rows;
    fa.p = c->params + c->table_floats;
    fa.m = dense_m;
    fa.v = c->adam_v + c->table_floats;
    fa.L = c->L;
    fa.n_domain = c->cfg.n_domain;
    fa.dm_snap = c->dmsnap[c->dm_cur];         // p plane: the domain table as this step's forward pass saw it
    fa.pdm = c->pdm;
    fa.wT = (P.need_wT && optimizer != MAMDR_OPT_ACCUMULATE) ? c->wT : nullptr;
    fa.flags = (c->w1t_unread ? FZ_F_W1T_UNREAD : 0) | (P.w2_all ? FZ_F_W2T_UNREAD : 0) | (c->fz_s_inorder ? FZ_F_S_INORDER : 0) |
               (c->fz_deal_residue || c->fz_s_inorder ? FZ_F_DEAL_RESIDUE : 0);
    c->fused_flags = fa.flags;
    fill_opt(c, optimizer, alpha, P.omb1, P.omb2, 2.0f * c->cfg.l2_emb, fa);
    fa.loss_part = c->loss_part;
    fa.n_loss_tiles = use4 ? rows_pad / 4 : rows_pad / TILE_ROWS;
    fa.frozen_sumsq = c->frozen_sumsq;
    fa.l2_emb = c->cfg.l2_emb;
    fa.loss_out = P.loss_out ? P.loss_out + s : nullptr;
#ifdef MAMDR_STAMPS
    fa.stamps = c->stamps ? c->stamps + 65536 + (c->global_step & 1) * 4096 : nullptr;
#endif
    // riders: the next slice of the window announced by mamdr_pregather_ahead (not in a profiled run: it times every kernel
    // on its own, k_pass_prep_multi among them)
    if (c->ahead.on && !c->profile) attach_riders(c, fa);
    {
        Prof p(c, MAMDR_KERNEL_WGRAD);
        launch_wgrad_adam(fa, c->stream);
    }
    // the domain table's step stays pending: the next step's tower kernel applies it, the last one of the call is
    // materialised below
    dm_pending.snap = c->dmsnap[c->dm_cur];
    dm_pending.pdm = c->pdm;
    dm_pending.n_part = DM_PARTS;
    dm_pending.n_domain = c->cfg.n_domain;
    fill_opt(c, optimizer, alpha, P.omb1, P.omb2, 2.0f * c->cfg.l2_emb, dm_pending);
    // (an Adam call leaves its last step pending for the next call's first tower / the next sync_tables)
    if (c->dm_finish_each || (s + 1 == P.n_steps && (optimizer != MAMDR_OPT_ADAM || c->dm_finish_call))) finish_dm(c);
    c->global_step += 1;
    return MAMDR_OK;
}

// ---- slab path: tower, k_wgrad (row groups -> gradient slabs), k_update (sums the slabs in order, optimiser step)
static int slab_step(mamdr_ctx* c, const CallPlan& P, int64_t s, float alpha) {
    const SplitData& d = *P.d;
    const int32_t optimizer = P.optimizer;
    const float omb1 = P.omb1, omb2 = P.omb2;
    const int64_t row_base = (P.first_step + s) * P.batch;
    const int rows = rows_at(P.pass_rows, row_base, P.batch);
    const int rows_pad = (int)pad_rows(rows);
    const bool use4 = takes_tower4(c, rows_pad);
    if (c->cfg.emb_trainable && c->lazy && optimizer == MAMDR_OPT_ADAM)
        emb_pre_step(c, d, P.perm, row_base, rows, rows_pad, alpha, omb1, omb2);
    TowerArgs ta;
    fill_step_tower(c, P, row_base, rows, ta);
    if (int rc = run_step_tower(c, ta, use4, s)) return rc;

    if (c->cfg.emb_trainable && P.loss_out) {
        prof_break(c);
        refresh_table_sumsq(c);
    }
    WgradArgs wa;
    const int groups = fill_wgrad_common(c, c->params + c->table_floats, rows, rows_pad, P.loss_out ? P.loss_out + s : nullptr, wa);
    wa.fmq = c->fmq;
    wa.ipbuf = c->ipbuf;
    wa.ld_off = c->L.ld;
    wa.ld_count = c->L.ld_count;
    wa.l2_lin = c->cfg.l2_linear;
    wa.lv_off = c->L.lv;
    wa.lv_count = c->L.lv_count;
    wa.uw_d = P.domain;
    wa.dm_copy = c->lin_w0dom ? c->dm_copy : nullptr;
    wa.n_loss_tiles = use4 ? rows_pad / 4 : rows_pad / TILE_ROWS;
    wa.dm_count = c->cfg.n_domain * EMB;
    wa.l2_emb = c->cfg.l2_emb;
#ifdef MAMDR_STAMPS
    wa.stamps = c->stamps ? c->stamps + 65536 : nullptr;
#endif
    // lazy table Adam: k_emb_reduce (and DeepFM's k_lin_sweep) only need the tower's outputs and write state no dense
    // kernel touches -> they ride in k_wgrad's / k_update's launches
    EmbStepArgs tea, nea;
    EmbRowsArgs nr;
    const bool next = P.tail && s + 1 < P.n_steps;
    if (P.tail) {
        fill_emb_args(c, optimizer, alpha, omb1, omb2, rows, tea);
        tea.flags_done = 1;
        tea.apply_now = 1;
    }
    if (next) fill_next_step(c, P, row_base + P.batch, nr, nea);
    // frozen tables, another step of this call follows on the 16-row tower: its gather is touched by riders in k_wgrad's
    // launch (GatherPf, mamdr_kernels.h; round 5: in k_update's launch, bound by what it pulls over the fabric, it lost 0.42 us
    // without them, k_wgrad gains 0.13 -- profiles/r05_ab_riders_place.txt)
    GatherPf pf;
    memset(&pf, 0, sizeof(pf));
    if (!P.tail && !c->cfg.emb_trainable && s + 1 < P.n_steps) {
        const int64_t nb = row_base + P.batch;
        const int nrows = rows_at(P.pass_rows, nb, P.batch);
        const int npad = (int)pad_rows(nrows);
        if (nrows > 0 && !takes_tower4(c, npad)) {
            pf.perm = P.perm;
            pf.uid = d.uid;
            pf.pid = d.pid;
            pf.dom = d.dom;
            pf.label = d.label;
            pf.user_tab = c->user_tab;
            pf.item_tab = c->item_tab;
            pf.row_base = nb;
            pf.n_rows_split = d.n;
            pf.rows = nrows;
            pf.n_user = c->cfg.n_user;
            pf.n_item = c->cfg.n_item;
            pf.n_tiles = npad / TILE_ROWS;
            pf.sink = c->loss_part;
        }
    }
    {
        Prof p(c, MAMDR_KERNEL_WGRAD);
        if (P.tail) launch_wgrad_reduce(wa, tea, next ? &nr : nullptr, nullptr, c->stream);
        else launch_wgrad(wa, c->stream, &pf);
    }

    UpdateArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.p = c->params + c->table_floats;
    ua.m = (optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m) + c->table_floats;
    ua.v = c->adam_v + c->table_floats;
    ua.slabs = c->slabs;
    ua.n_groups = groups;
#ifdef MAMDR_STAMPS
    ua.stamps = c->stamps ? c->stamps + 65536 + 8192 : nullptr;
#endif
    ua.slab_ld = c->slab_ld;
    ua.s_off = c->L.alloc;
    ua.w0dom_copy = c->w0dom_copy;
    ua.dm_copy = c->lin_w0dom ? c->dm_copy : nullptr;
    ua.n_domain = c->cfg.n_domain;
    ua.count4 = c->L.alloc / 4;
    ua.dm_count = c->cfg.n_domain * EMB;
    ua.s2_off = c->s2_off;
    ua.ld_off = c->L.ld;
    ua.ld_count = c->L.ld_count;
    ua.two_l2_lin = 2.0f * c->cfg.l2_linear;
    fill_opt(c, optimizer, alpha, omb1, omb2, 2.0f * c->cfg.l2_emb, ua);
    ua.wT = (P.need_wT && optimizer != MAMDR_OPT_ACCUMULATE) ? c->wT : nullptr;
    ua.w1_off = c->L.w1;
    ua.w2_off = c->L.w2;
    ua.w0_off = c->L.w0;
    ua.w0t = (c->cfg.emb_trainable && !c->nfm) ? 1 : 0;
    ua.no_sdm = c->nfm ? 1 : 0;
    {
        Prof p(c, MAMDR_KERNEL_UPDATE);
        if (P.tail) launch_update_lin(ua, tea, c->deepfm, next ? &nea : nullptr, c->stream);
        else launch_update(ua, c->stream);
    }
    if (next) take_next_rows(c);
    if (c->cfg.emb_trainable && !P.tail) emb_post_step(c, optimizer, alpha, omb1, omb2, rows);
    c->global_step += 1;
    return MAMDR_OK;
}

extern "C" {

// a set of the pass buffer holds at least `rows` positions (its contents are lost when it grows; the other set stays)
static int grow_pass_set(DevAllocs& dev, float*& xpre, int32_t*& pdom, float*& plabel, int64_t& have, int64_t rows) {
    if (rows <= have) return MAMDR_OK;
    const int64_t cap = rows + rows / 4 + 1024;
    dev.release(xpre); dev.release(pdom); dev.release(plabel);
    xpre = nullptr; pdom = nullptr; plabel = nullptr; have = 0;
    dev.alloc(&xpre, (size_t)cap * 2 * EMB);
    dev.alloc(&pdom, (size_t)cap);
    dev.alloc(&plabel, (size_t)cap);
    if (const int rc = dev.check(g_err)) return rc;
    have = cap;
    return MAMDR_OK;
}
// the current set: what was gathered ahead is dropped with it
static int grow_pass_buffer(mamdr_ctx* c, int64_t rows) {
    if (rows <= c->pre_cap) return MAMDR_OK;
    drop_pregathered(c);
    return grow_pass_set(c->dev, c->xpre, c->pdom, c->plabel, c->pre_cap, rows);
}

int64_t mamdr_pregather_hits(const mamdr_ctx* c) { return c ? c->pg_hits : 0; }
int64_t mamdr_pregather_launches(const mamdr_ctx* c) { return c ? c->pg_launches : 0; }
int64_t mamdr_pregather_rider_rows(const mamdr_ctx* c) { return c ? c->pg_rider_rows : 0; }
int64_t mamdr_pregather_remainder_rows(const mamdr_ctx* c) { return c ? c->pg_remainder_rows : 0; }

// a pass list as both hints lay it out: pass k's n + 16 positions at row off (a multiple of 4) of a set of the pass buffer,
// one workgroup of k_pass_prep_multi per 4 positions.  -> the rows the set must hold
static int lay_out_passes(mamdr_ctx* c, int32_t n_passes, const int32_t* h_domains, const int32_t* const* h_d_perms,
                          const int64_t* h_pass_rows, int32_t batch, PassPrepMultiArgs& a, std::vector<mamdr_ctx::PgEntry>& list,
                          int64_t& total) {
    memset(&a, 0, sizeof(a));
    list.clear();
    int64_t off = 0;
    int wgs = 0;
    for (int k = 0; k < n_passes; ++k) {
        SplitData* d = split_of(c, h_domains[k], MAMDR_SPLIT_TRAIN);
        if (!d || !d->bound) return fail(MAMDR_ESTATE, "pregather: train split of domain %d is not bound", h_domains[k]);
        int64_t n = h_pass_rows ? h_pass_rows[k] : -1;
        if (n < 0) n = d->n;
        if (n > d->n) return fail(MAMDR_EINVAL, "pregather: pass of %lld rows exceeds the %lld rows of domain %d", (long long)n,
                                  (long long)d->n, h_domains[k]);
        PassPrepMultiArgs::Pass& p = a.p[k];
        p.uid = d->uid;
        p.pid = d->pid;
        p.dom = d->dom;
        p.label = d->label;
        p.perm = h_d_perms ? h_d_perms[k] : nullptr;
        p.n = n;
        p.n_rows_split = d->n;
        p.out_off = off;
        p.pad_dom = h_domains[k];
        const int64_t w = n > 0 ? (n + PREP_PAD + 3) / 4 : 0;      // (an empty pass has no steps: nothing to gather)
        wgs += (int)w;
        a.wg_end[k] = wgs;
        list.push_back(mamdr_ctx::PgEntry{h_domains[k], p.perm, n, off, batch});
        off += 4 * w;
    }
    a.n_pass = n_passes;
    a.user_tab = c->user_tab;
    a.item_tab = c->item_tab;
    a.n_user = c->cfg.n_user;
    a.n_item = c->cfg.n_item;
    a.n_domain = c->cfg.n_domain;
    total = off;
    return MAMDR_OK;
}
// where a hint has an effect: where a call would gather its pass itself (frozen tables, k_wgrad_adam path)
static bool pregather_applies(const mamdr_ctx* c, int32_t n_passes, int32_t batch) {
    return n_passes > 0 && batch > 0 && batch <= c->cfg.max_batch && c->use_pre && takes_fused_path(c, batch);
}

int mamdr_pregather_passes(mamdr_ctx* c, int32_t n_passes, const int32_t* h_domains, const int32_t* const* h_d_perms,
                           const int64_t* h_pass_rows, int32_t batch) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    if (n_passes < 0 || (n_passes > 0 && !h_domains)) return fail(MAMDR_EINVAL, "pregather: bad pass list");
    const bool had_ahead = c->ahead.on;
    drop_pregathered(c);
    c->pg_pos = 0;
    if (!pregather_applies(c, n_passes, batch)) return MAMDR_OK;
    if (n_passes > PREP_MAX_PASSES) n_passes = PREP_MAX_PASSES;      // the later ones gather themselves
    PassPrepMultiArgs a;
    std::vector<mamdr_ctx::PgEntry> list;
    int64_t total = 0;
    if (int rc = lay_out_passes(c, n_passes, h_domains, h_d_perms, h_pass_rows, batch, a, list, total)) return rc;
    if (total == 0) {
        c->pg = list;
        return MAMDR_OK;
    }
    // the window announced by mamdr_pregather_ahead: its set takes over and only what the riders did not reach is gathered now
    mamdr_ctx::Ahead& h = c->ahead;
    bool adopt = had_ahead && h.list.size() == list.size();
    for (size_t k = 0; adopt && k < list.size(); ++k)
        adopt = h.list[k].domain == list[k].domain && h.list[k].perm == list[k].perm && h.list[k].n == list[k].n &&
                h.list[k].batch == list[k].batch;
    if (adopt) {
        std::swap(c->xpre, c->xpre_ahead);
        std::swap(c->pdom, c->pdom_ahead);
        std::swap(c->plabel, c->plabel_ahead);
        std::swap(c->pre_cap, c->pre_cap_ahead);
        pre_plan_settle(h.rows.data(), n_passes, h.cur);
        int wgs = 0;
        int64_t left = 0;
        for (int k = 0; k < n_passes; ++k) {
            const int64_t from = k < h.cur.pass ? pre_plan_positions(h.rows[k]) : (k == h.cur.pass ? h.cur.pos : 0);
            const int64_t todo = pre_plan_positions(h.rows[k]) - from;
            a.p[k].i0 = from;
            wgs += (int)((todo + 3) / 4);
            a.wg_end[k] = wgs;
            left += todo;
        }
        if (left == 0) a.n_pass = 0;
        c->pg_remainder_rows += left;
    } else if (int rc = grow_pass_buffer(c, total)) {
        return rc;
    }
    c->pg = list;
    a.xpre = c->xpre;
    a.pdom = c->pdom;
    a.plabel = c->plabel;
    c->pg_launches++;
    if (a.n_pass > 0) {              // (0: the riders gathered the whole window)
        prof_break(c);
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_pass_prep_multi(a, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_pregather_ahead(mamdr_ctx* c, int32_t n_passes, const int32_t* h_domains, const int32_t* const* h_d_perms,
                          const int64_t* h_pass_rows, int32_t batch, int64_t spread_steps) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    if (n_passes < 0 || (n_passes > 0 && !h_domains)) return fail(MAMDR_EINVAL, "pregather: bad pass list");
    mamdr_ctx::Ahead& h = c->ahead;
    h.on = false;
    // a hint about a hint: nothing where mamdr_pregather_passes does nothing, nothing without riders or steps to carry them
    if (!pregather_applies(c, n_passes, batch) || spread_steps <= 0 || !c->ride_on || c->profile || ride_wgs(c, false) <= 0)
        return MAMDR_OK;
    if (n_passes > PREP_MAX_PASSES) n_passes = PREP_MAX_PASSES;
    int64_t total = 0;
    if (int rc = lay_out_passes(c, n_passes, h_domains, h_d_perms, h_pass_rows, batch, h.args, h.list, total)) return rc;
    if (total == 0) return MAMDR_OK;
    if (int rc = grow_pass_set(c->dev, c->xpre_ahead, c->pdom_ahead, c->plabel_ahead, c->pre_cap_ahead, total)) return rc;
    h.rows.clear();
    for (const mamdr_ctx::PgEntry& e : h.list) h.rows.push_back(e.n);
    h.cur = PrePlanCursor();
    h.on = true;
    return MAMDR_OK;
}

int mamdr_train_steps(mamdr_ctx* c, int domain, const int32_t* d_perm, int64_t first_step, int64_t n_steps,
                      int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr, float* d_loss_out) {
    return mamdr_train_steps_n(c, domain, d_perm, -1, first_step, n_steps, batch, dropout_seed, optimizer, lr, d_loss_out);
}

int mamdr_train_steps_n(mamdr_ctx* c, int domain, const int32_t* d_perm, int64_t pass_rows, int64_t first_step,
                        int64_t n_steps, int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr,
                        float* d_loss_out) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    SplitData* d = split_of(c, domain, MAMDR_SPLIT_TRAIN);
    if (const int rc = check_train_call(g_err, d, domain, batch, c->cfg.max_batch, optimizer, c->accum, "mamdr_bind_accumulator",
                                        first_step, n_steps, &pass_rows))
        return rc;
    if (const int rc = check_step_range(g_err, domain, pass_rows, batch, first_step, n_steps)) return rc;
    if (n_steps == 0) return MAMDR_OK;      // an empty pass (empty domain, meta_train_step window of nothing): no launch, no state change

    const float rate = c->cfg.dropout;
    double thr = (double)rate * 4294967296.0;
    const uint32_t drop_thresh = thr >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(int64_t)thr;
    const float keep_scale = (float)(1.0 / (1.0 - (double)rate));
    const float omb1 = 1.0f - c->cfg.adam_beta1, omb2 = 1.0f - c->cfg.adam_beta2;
    // the meta pass runs with the Keras learning phase at its default (0): dropout off
    const int use_dropout = (rate > 0.f && optimizer != MAMDR_OPT_ACCUMULATE) ? 1 : 0;
    CallPlan P{d, domain, d_perm, pass_rows, first_step, n_steps, batch, optimizer, lr, omb1, omb2, d_loss_out,
               dropout_seed, drop_thresh, keep_scale, use_dropout};
    // SGD / accumulate steps update the tables densely: bring every lagging row up to date first
    if (optimizer != MAMDR_OPT_ADAM) sync_tables(c);
    plan_call(c, P);

    c->rows_ready = false;
    c->catchup_ready = false;
    prof_break(c);
    // k_wgrad_adam path: the domain table's step of the previous step -- of this call or, between two Adam calls, of
    // the previous call (c->dm_pending); every other kind of call starts from the materialised table
    if (!(P.path == StepPath::fused && optimizer == MAMDR_OPT_ADAM)) finish_dm(c);
    if (P.pre && P.pre_cached) {
        if (P.build_wT) launch_transpose_w(c->params + c->table_floats, c->L, c->wT, c->stream);
    } else if (P.pre) {
        if (int rc = grow_pass_buffer(c, P.pre_n + 16)) return rc;
        PassPrepArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.user_tab = c->user_tab;
        pa.item_tab = c->item_tab;
        pa.uid = d->uid;
        pa.pid = d->pid;
        pa.dom = d->dom;
        pa.label = d->label;
        pa.perm = d_perm;
        pa.pos0 = P.pre_pos0;
        pa.n = P.pre_n;
        pa.n_rows_split = d->n;
        pa.n_user = c->cfg.n_user;
        pa.n_item = c->cfg.n_item;
        pa.n_domain = c->cfg.n_domain;
        pa.pad_dom = domain;
        pa.xpre = c->xpre;
        pa.pdom = c->pdom;
        pa.plabel = c->plabel;
        if (P.build_wT) {                // ... in k_pass_prep's launch (one launch less per call)
            pa.tw_dense = c->params + c->table_floats;
            pa.tw_L = c->L;
            pa.tw_wT = c->wT;
        }
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_pass_prep(pa, c->stream);
    } else if (P.build_wT) {
        launch_transpose_w(c->params + c->table_floats, c->L, c->wT, c->stream);
    }
    // (what the call's steps leave behind: k_wgrad_adam / k_update keep the copies of what they step current when the
    // call uses them; steps without them make them stale; accumulate steps change no weight)
    if (P.w2_all) c->wT_valid = false;         // (W2T is not kept: a later call that reads it builds it)
    else if (optimizer != MAMDR_OPT_ACCUMULATE) c->wT_valid = P.need_wT;
    else if (P.build_wT) c->wT_valid = true;
    for (int64_t s = 0; s < n_steps; ++s) {
        // the reported loss carries l2 * sum(table^2) over EVERY row: bring lagging rows up to date first
        // (only callers that ask for the per-step loss pay this flush; the meta loops do not)
        if (d_loss_out) sync_tables(c);
        const float alpha = advance_step(c, optimizer, lr);
        const int rc = P.path == StepPath::star    ? star_step(c, P, s, alpha)
                       : P.path == StepPath::fused ? fused_step(c, P, s, alpha)
                                                   : slab_step(c, P, s, alpha);
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

}  // extern "C"
