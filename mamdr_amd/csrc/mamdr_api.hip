// C ABI of libmamdr_hip.so (declared in include/mamdr_hip.h).
//
// Host-side state is tiny: bound pointers, the Adam step count with its fp32
// running beta powers (TF keeps them as beta1_power / beta2_power variables), the
// global inner-step counter that indexes the dropout stream, and a private
// workspace sized for max_batch.  Everything numeric runs in the kernels of
// step_kernels.hip / outer_kernels.hip on the context's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mamdr_hip.h"
#include "mamdr_kernels.h"
#include "env_registry.h"

using namespace mamdr;

namespace mamdr {
thread_local hipEvent_t g_prof_stop = nullptr;
}

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(MAMDR_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct SplitData {
    const int32_t* uid = nullptr;
    const int32_t* pid = nullptr;
    const int32_t* dom = nullptr;
    const float* label = nullptr;
    int64_t n = 0;
    bool bound = false;     // an EMPTY split (n = 0, null columns) is bound too: a pass over it has no steps
};

struct EventPair {
    hipEvent_t a, b;
    bool own_a = true;         // false: `a` is the previous kernel's stop event (owned by that pair)
};

}  // namespace

struct mamdr_ctx {
    mamdr_config cfg;
    hipStream_t stream = nullptr;
    DenseLayout L;
    int64_t table_floats = 0;   // trainable user+item floats in front of the dense block
    bool deepfm = false;
    bool nfm = false;           // linear tables + DNN over the bi-interaction (MAMDR_TOWER_NFM): FM instances, mode 4
    bool pnn = false;           // the mlp tower + three inner-product inputs (MAMDR_TOWER_PNN): FM instances of the towers, mode 3
    float* ipbuf = nullptr;     // PNN: [rows_pad][4] the batch's inner products (A operand of dW0x's tiles)
    bool star = false;
    StarLayout SL;
    StarAuxLayout AL;
    int64_t n_meta = 0;
    float* aux = nullptr;           // bound PartitionedNorm state (Star)
    float* eff = nullptr;           // Star: effective dense block of the step's domain
    float* pn = nullptr;            // Star: [PN_WS_FLOATS]
    float* star_part = nullptr;     // Star: [chunks][2][384] partials (forward statistics as doubles, then backward sums as floats)
    float* star_sums = nullptr;     // Star: [2][384] PN sums + [128] domain-row gradient
    float* star_dmpart = nullptr;   // Star: [chunks][EMB]
    int64_t lin_user_off = 0;   // DeepFM + trainable tables: 1-d linear tables behind the embedding tables
    int64_t lin_item_off = 0;
    int64_t n_params = 0;       // floats of the flat vector (incl. padding)
    // bound state
    float* params = nullptr;
    float* adam_m = nullptr;
    float* adam_v = nullptr;
    float* accum = nullptr;         // meta-gradient accumulator (MAMDR_OPT_ACCUMULATE)
    const float* user_tab = nullptr;
    const float* item_tab = nullptr;
    std::vector<SplitData> data;   // [domain*3 + split]
    // optimiser / stream counters (host side)
    int64_t adam_t = 0;
    float b1p = 1.0f, b2p = 1.0f;
    uint32_t global_step = 0;
    // workspace
    int rows_pad_max = 0;
    float* acts = nullptr;
    float* dz = nullptr;
    float* dlogit = nullptr;
    float* w0dom_copy = nullptr;    // slab path only: k_wgrad's pre-update snapshot of W0[256:384, :] for k_update
    float* dm_copy = nullptr;       // pre-update snapshot of the domain table (dW0[256:384] by linearity)
    bool lin_w0dom = false;         // k_wgrad carries no tiles for W0[256:384]: k_update rebuilds that gradient from S
    float* wT = nullptr;            // transposed W1 / W2 (k_tower4)
    // mlp tower with frozen tables: weight gradients + optimiser step in one launch (k_wgrad_adam) + k_dm_finish
    // instead of k_wgrad -> slabs -> k_update (MAMDR_FUSED=0 keeps the slab path)
    bool fused = false;
    float* star_alpha = nullptr;    // Star tower: alphas of the current call's steps (lazy replay of the other domains' slices)
    int star_dense_slices = 0;      // MAMDR_STAR_DENSE_SLICES=1: every slice swept every step (diagnostic; same bits)
    int t4_no_w1l = 0;              // MAMDR_T4_NO_W1L=1: k_tower4 without the W1 image in LDS (diagnostic)
    int fused_max_batch = 1024;     // batches up to this size take the fused path (MAMDR_FUSED=2: every batch size):
                                    // 4 rows x the CU count, set at mamdr_create
    int tower4_max_rows = 2048;     // steps of up to this many (padded) rows run k_tower4, see mamdr_create
    float* pdm = nullptr;           // [32][n_domain][EMB] partial domain-table gradients
    // the domain table's step stays pending until the next tower kernel applies it (DmStep, mamdr_kernels.h):
    // two snapshots [3][n_domain][EMB] of (p, m, v) alternate between steps
    // the rows of a call pre-gathered once (k_pass_prep): [cap][2 EMB] + domain / label per position, grown on demand
    float* xpre = nullptr;
    int32_t* pdom = nullptr;
    float* plabel = nullptr;
    int64_t pre_cap = 0;
    // passes gathered ahead of their calls (mamdr_pregather_passes): entry k's rows sit at [off, off + n + 16) of xpre
    struct PgEntry { int domain; const int32_t* perm; int64_t n, off; int batch; };
    std::vector<PgEntry> pg;
    size_t pg_pos = 0;
    int64_t pg_hits = 0;            // calls served from an entry (mamdr_pregather_hits)
    int64_t pg_launches = 0;        // hints whose window was gathered ahead of its calls (mamdr_pregather_launches)
    // the second set of the pass buffer: the window announced by mamdr_pregather_ahead is gathered here, slice by slice, by
    // the riders of k_wgrad_adam while the steps of the current window read the first set; mamdr_pregather_passes with the
    // same pass list swaps the sets and launches k_pass_prep_multi over what the riders did not reach.  Each set has its
    // own capacity and growing one never frees the other
    float* xpre_ahead = nullptr;
    int32_t* pdom_ahead = nullptr;
    float* plabel_ahead = nullptr;
    int64_t pre_cap_ahead = 0;
    struct Ahead {
        bool on = false;
        std::vector<PgEntry> list;      // the announced passes, laid out as mamdr_pregather_passes lays them out
        std::vector<int64_t> rows;      // ... their row counts (the planner's view)
        PassPrepMultiArgs args;         // ... and their columns
        PrePlanCursor cur;              // first position no rider gathered yet
    } ahead;
    int n_cu = 0;                   // CUs of the device: k_wgrad_adam's riders fill what its own workgroups leave idle
    bool ride_on = true;            // MAMDR_NO_PREGATHER_RIDE=1: no riders (mamdr_pregather_ahead does nothing)
    int64_t pg_rider_rows = 0;      // positions gathered by riders / by the remainder launches of adopted windows
    int64_t pg_remainder_rows = 0;
    bool use_pre = true;            // MAMDR_NO_PREGATHER=1: the towers gather through perm / uid / pid every step
    float* dmsnap[2] = {nullptr, nullptr};
    int dm_cur = 0;
    // ... ACROSS calls too (round 4): an Adam call leaves its last step pending; the first tower of the next fused Adam
    // call applies it, anything else that reads or replaces the live state materialises it first (finish_dm, from
    // sync_tables -- the contract of mamdr_sync_tables).  MAMDR_DM_EACH=1 / MAMDR_DM_CALL=1: after every step / call.
    DmStep dm_pending{};
    bool dm_finish_call = false;
    // the transposed copies in wT hold the live W1 / W2 (/ W0[0:256]): true after a call whose steps kept them current,
    // false once the live state may have been replaced from outside (sync_tables) or stepped without them
    bool wT_valid = false;
    // ... except W1T in a context none of whose tower launches can read it (w1t_unread_now: every k_tower4 grid takes the
    // W1 image): k_wgrad_adam skips those 128 KB of strided stores per step.  A function of the context's configuration;
    // mamdr_set_tower_tile, which can change it, drops wT_valid
    bool w1t_unread = false;
    // ... and W2T in a context every training call of which runs pre-gathered on the k_wgrad_adam path with the W1 image
    // (w2t_unread_now): every tower then reads W2 in place (k_tower4<.., W2D>), k_wgrad_adam skips those 32 KB of
    // strided stores per step, and the copies are never built or called current (MAMDR_NO_W2_DIRECT=1: built and kept)
    bool w2t_unread = false;
    int fused_flags = -1;           // FZ_F_* of the latest k_wgrad_adam launch (mamdr_fused_flags)
    bool fz_s_inorder = false;      // MAMDR_FZ_S_INORDER=1: k_wgrad_adam's S workgroups take their column blocks in grid order
    bool fz_deal_residue = false;   // MAMDR_FZ_DEAL_RESIDUE=1 (implied by the switch above): the residue dealing, not the one by matrix
    bool w2_direct_ok = true;       // MAMDR_NO_W2_DIRECT=1: always build the copies at the start of a call (k_transpose_w)
    bool dm_finish_each = false;    // MAMDR_DM_EACH=1: materialise after every step (k_dm_finish per step; A/B measurements)
    int tower_tile = 0;             // 0 auto, 4 / 16 forced (env MAMDR_TOWER_TILE)
    // trainable user / item tables
    float* dxe = nullptr;
    int32_t* urow = nullptr;
    int32_t* irow = nullptr;
    int32_t* map_u = nullptr;
    int32_t* map_i = nullptr;
    float* gbuf_u = nullptr;
    float* gbuf_i = nullptr;
    int32_t* hasdup_u = nullptr;
    int32_t* hasdup_i = nullptr;
    // lazy dense Adam over the trainable tables (emb_kernels.hip); MAMDR_DENSE_ADAM=1 keeps the per-step sweep
    bool lazy = false;
    bool tables_dirty = false;      // some rows lag behind adam_t
    int32_t* last_u = nullptr;      // [n_user] / [n_item] Adam step each row is current at
    int32_t* last_i = nullptr;
    float* alpha_log = nullptr;     // ring of the per-step alpha
    int log_cap = 1 << 16;
    // Adam steps between forced flushes.  Every missed step is replayed exactly once either way; the flush
    // replays at full occupancy, the per-row catch-up before a gather is a serial chain per row, so short gaps
    // win until the flush's own table traffic shows (Amazon-6, 10 % rows: 7.7 K domain-steps/s without a period,
    // 11.6 K at 16, 12.1 K at 32, 12.0 K at 64, 10.9 K at 256).  MAMDR_LAZY_FLUSH_EVERY overrides.
    int flush_every = 32;
    int64_t flush_t = 0;            // adam_t of the last flush
    int64_t n_flush = 0;            // k_emb_flush launches so far / those forced by the flush period (mamdr_table_flushes)
    int64_t n_flush_forced = 0;
    float* fmq = nullptr;           // DeepFM: [rows_pad][EMB]
    float* glin_u = nullptr;        // DeepFM + trainable tables: [rows_pad]
    float* glin_i = nullptr;
    int32_t* domrow = nullptr;
    float* loss_part = nullptr;     // train: per tile of a batch
    float* eval_part = nullptr;     // eval: per tile of a split (grown on bind)
    int64_t eval_part_cap = 0;
    float* slabs = nullptr;         // [WGRAD_MAX_GROUPS][slab_ld]
    bool tail_fuse = true;      // MAMDR_NO_TAILFUSE=1: k_emb_reduce / k_lin_sweep as launches of their own
    // the other half of the row / map double buffer: the NEXT step's k_emb_rows rides in this step's last launch
    int32_t* urow_alt = nullptr;
    int32_t* irow_alt = nullptr;
    int32_t* map_u_alt = nullptr;
    int32_t* map_i_alt = nullptr;
    bool rows_ready = false;    // the current buffers already hold the rows of the step about to run
    bool catchup_ready = false; // ... and those rows were already brought up to the previous step
    int slab_ld = 0;            // dense block + S region ([n_domain][256]) (+ DeepFM S2 region [n_domain][128])
    int s2_off = 0;
    TileDesc* tiles = nullptr;
    int n_tiles = 0;
    float* thresholds = nullptr;
    float* frozen_sumsq = nullptr;  // [4] user, item table; DeepFM linear user, item table
    float* sumsq_partials = nullptr;
    // mamdr_recommend's workspace (RecArgs, mamdr_kernels.h): allocated on first use for chunks of up to rec_cap candidates
    int rec_chunk = 16384;          // candidates per pass (MAMDR_REC_CHUNK)
    int rec_cap = 0;
    float* rec_P = nullptr;
    float* rec_lin = nullptr;
    float* rec_q = nullptr;         // q0 | qud | qs
    unsigned long long* rec_part = nullptr;
    unsigned long long* rec_best = nullptr;
#ifdef MAMDR_STAMPS
    unsigned long long* stamps = nullptr;
#endif
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;    // recycled profiling events
    void ev_pool_push(hipEvent_t e) { ev_pool.push_back(e); }
    // a kernel's time = its stop event minus the stop event of the kernel launched right before it on the stream
    // (start markers of their own, attached or recorded, run ahead of the previous kernel's completion when the
    // host is ahead, or add a packet between the kernels); chain_ok: prev_b is that immediately preceding event
    hipEvent_t prev_b = nullptr;
    bool chain_ok = false;
    std::vector<EventPair> ev[MAMDR_KERNEL_COUNT];
};

namespace {

std::vector<TileDesc> build_tiles(const DenseLayout& L, int n_domain, bool deepfm, int s2_off, bool lin_w0dom, bool star,
                                  bool pnn = false, bool nfm = false) {
    std::vector<TileDesc> t;
    struct G { int a_off, M, b_off, N, dst; };
    // dW0 = x^T dz1, dW1 = h1^T dz2, dW2 = h2^T dz3
    const G gemms[3] = {{0, XDIM, 0, H1, L.w0}, {XDIM, H1, H1, H2, L.w1}, {XDIM + H1, H2, H1 + H2, H3, L.w2}};
    // (64x64 tiles first: the kernel stages their operands through LDS)
    // (lin_w0dom: rows 256..383 of x are per-domain constants, their part of dW0 follows from S in k_update)
    // (NFM: rows 0..255 of W0 meet the raw user / item rows of the tile but are no parameters -- they stay zero: no tiles)
    for (const G& g : gemms)
        for (int m0 = (nfm && g.dst == L.w0) ? 2 * EMB : 0; m0 < ((lin_w0dom && g.dst == L.w0) ? 2 * EMB : g.M); m0 += 64)
            for (int n0 = 0; n0 < g.N; n0 += 64)
                t.push_back(TileDesc{0, g.a_off + m0, 0, g.b_off + n0, g.dst + m0 * g.N + n0, g.N, 64, 64, 1});
    // biases = column sums of dz (A = ones in row 0)
    const int boff[3] = {L.b0, L.b1, L.b2}, bn[3] = {H1, H2, H3}, zoff[3] = {0, H1, H1 + H2};
    for (int l = 0; l < 3; ++l)
        for (int n0 = 0; n0 < bn[l]; n0 += 32) t.push_back(TileDesc{1, 0, 0, zoff[l] + n0, boff[l] + n0, 0, 1, 32});
    // output unit: dwo = h3^T dlogit, dgb = sum dlogit
    for (int m0 = 0; m0 < H3; m0 += 32) t.push_back(TileDesc{0, XDIM + H1 + H2 + m0, 1, 0, L.wo + m0, 1, 32, 1});
    t.push_back(TileDesc{1, 0, 1, 0, L.gb, 0, 1, 1});
    // domain table, by linearity: S = onehot(domain)^T dz1 ([n_domain][256], behind the dense block in
    // the slab); k_update turns it into dDm = S . W0[256:384,:]^T
    // (not for the Star tower: its domain-row gradient comes through PartitionedNorm's backward)
    for (int m0 = 0; m0 < (star ? 0 : n_domain); m0 += 32)
        for (int n0 = 0; n0 < H1; n0 += 32) {
            const int mv = n_domain - m0 < 32 ? n_domain - m0 : 32;
            t.push_back(TileDesc{2, m0, 0, n0, L.alloc + m0 * H1 + n0, H1, mv, 32});
        }
    if (deepfm || pnn)
        for (int m0 = 0; m0 < n_domain; m0 += 32) {
            const int mv = n_domain - m0 < 32 ? n_domain - m0 : 32;
            // per-row part of the domain-table gradient: S2 = onehot(domain)^T fmq (DeepFM: dlogit * (u + i); PNN: the
            // inner products' chain rule, dip_ud * u + dip_id * i)
            for (int n0 = 0; n0 < EMB; n0 += 32) t.push_back(TileDesc{2, m0, 2, n0, s2_off + m0 * EMB + n0, EMB, mv, 32});
            // linear domain table: onehot(domain)^T dlogit
            if (deepfm) t.push_back(TileDesc{2, m0, 1, 0, L.ld + m0, 1, mv, 1});
        }
    // PNN: the three extra rows of the first kernel, dW0x = ip^T dz1 (A = the batch's inner products, ipbuf [B][4])
    if (pnn)
        for (int n0 = 0; n0 < H1; n0 += 32) t.push_back(TileDesc{3, 0, 0, n0, L.wx + n0, H1, 3, 32});
    return t;
}

int check_ctx(const mamdr_ctx* c) {
    if (!c) return fail(MAMDR_EINVAL, "null context");
    return MAMDR_OK;
}

SplitData* split_of(mamdr_ctx* c, int domain, int split) {
    if (domain < 0 || domain >= c->cfg.n_domain || split < 0 || split > 2) return nullptr;
    return &c->data[(size_t)domain * 3 + split];
}

// per-kernel device time from stop events chained along the stream (see mamdr_ctx::prev_b)
struct Prof {
    mamdr_ctx* c;
    int k;
    EventPair e{nullptr, nullptr, true};
    Prof(mamdr_ctx* c_, int k_, bool = false) : c(c_), k(k_) {
        if (!c->profile || c->ev[k].size() >= 200000) return;
        auto take = [&]() {
            hipEvent_t ev = nullptr;
            if (!c->ev_pool.empty()) {          // (pool refilled by mamdr_profile_reset: no event creation per launch)
                ev = c->ev_pool.back();
                c->ev_pool.pop_back();
            } else {
                (void)hipEventCreate(&ev);
            }
            return ev;
        };
        e.b = take();
        if (c->chain_ok && c->prev_b) {
            e.a = c->prev_b;
            e.own_a = false;
        } else {                                // nothing timed right before: an explicit start marker
            e.a = take();
            (void)hipEventRecord(e.a, c->stream);
        }
        g_prof_stop = e.b;                      // the launch issued inside this scope carries it (MAMDR_LAUNCH)
    }
    ~Prof() {
        if (!e.b) return;
        if (g_prof_stop) {                      // no launch took it (should not happen): record it the plain way
            g_prof_stop = nullptr;
            (void)hipEventRecord(e.b, c->stream);
        }
        c->ev[k].push_back(e);
        c->prev_b = e.b;
        c->chain_ok = true;
    }
};
// a launch that is not timed went out: the next timed kernel needs a start marker of its own
static inline void prof_break(mamdr_ctx* c) { c->chain_ok = false; }

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

int ready(const mamdr_ctx* c) {
    if (!c->params) return fail(MAMDR_ESTATE, "mamdr_bind_state has not been called");
    if (c->star && !c->aux) return fail(MAMDR_ESTATE, "Star tower: mamdr_bind_aux has not been called");
    if (!c->cfg.emb_trainable && (!c->user_tab || !c->item_tab))
        return fail(MAMDR_ESTATE, "frozen user/item tables are not bound (mamdr_bind_table)");
    return MAMDR_OK;
}

}  // namespace


// ---- trainable user / item tables: shared by the mlp / deepfm and the Star step
static void fill_emb_args(const mamdr_ctx* c, int32_t optimizer, float alpha, float omb1, float omb2, float two_l2,
                          int rows, int dx_ld, EmbStepArgs& ea) {
    memset(&ea, 0, sizeof(ea));
    float* slot_m = optimizer == MAMDR_OPT_ACCUMULATE ? c->accum : c->adam_m;
    ea.p = c->params;
    ea.m = slot_m;
    ea.v = c->adam_v;
    ea.dxe = c->dxe;
    ea.dx_ld = dx_ld;
    ea.dlogit = c->dlogit;
    ea.rows = rows;
    ea.two_l2_lin = 2.0f * c->cfg.l2_linear;
    ea.opt.optimizer = optimizer;
    ea.opt.alpha = alpha;
    ea.opt.omb1 = omb1;
    ea.opt.omb2 = omb2;
    ea.opt.eps = c->cfg.adam_eps;
    ea.opt.two_l2 = two_l2;
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

constexpr int STAR_ALPHA_CAP = 1 << 12;      // steps between two replays of the lagging Star slices (power of two)
constexpr int WGRAD_MAX_GROUPS = 16;         // row groups of k_wgrad at most (= gradient slabs k_update sums)
static float table_two_l2(const mamdr_ctx* c) { return c->star ? 0.f : 2.0f * c->cfg.l2_emb; }

// materialise a domain-table step the k_wgrad_adam path left pending
static void finish_dm(mamdr_ctx* c) {
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
static void sync_tables(mamdr_ctx* c) {
    finish_dm(c);
    c->wT_valid = false;
    if (!c->tables_dirty) return;
    EmbStepArgs ea;
    fill_emb_args(c, MAMDR_OPT_ADAM, 0.f, 1.0f - c->cfg.adam_beta1, 1.0f - c->cfg.adam_beta2, table_two_l2(c), 0,
                  c->star ? XDIM : 2 * EMB, ea);
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
        fill_emb_args(c, MAMDR_OPT_ADAM, alpha, omb1, omb2, table_two_l2(c), rows, c->star ? XDIM : 2 * EMB, ea);
        Prof p(c, MAMDR_KERNEL_AUX);
        launch_emb_catchup(ea, c->stream);
    }
    c->catchup_ready = false;
    c->tables_dirty = true;
}

// after the tower / wgrad: scatter-add of the row gradients and the optimiser on the tables
static void emb_post_step(mamdr_ctx* c, int32_t optimizer, float alpha, float omb1, float omb2, int rows) {
    EmbStepArgs ea;
    fill_emb_args(c, optimizer, alpha, omb1, omb2, table_two_l2(c), rows, c->star ? XDIM : 2 * EMB, ea);
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
static int64_t pad_rows(int64_t rows) { return (rows + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS; }
// rows of the batch at row_base of a pass of pass_rows rows (the last batch of a pass may be short)
static int rows_at(int64_t pass_rows, int64_t row_base, int batch) { return (int)std::min<int64_t>(batch, pass_rows - row_base); }
// one path per call (the pending domain-table step lives across the steps of a call): k_wgrad_adam for batches up to
// fused_max_batch rows (measured: 27.3 vs 29.5 us / step at 1,024 rows, a tie at 4,096), k_wgrad -> slabs -> k_update above
static bool takes_fused_path(const mamdr_ctx* c, int64_t batch) { return c->fused && pad_rows(batch) <= c->fused_max_batch; }
// forget every pass gathered ahead of its call, and the window the riders are working on
static void drop_pregathered(mamdr_ctx* c) {
    c->pg.clear();
    c->ahead.on = false;
}
// rider workgroups a k_wgrad_adam launch can carry: the CUs its own workgroups leave idle (none on a smaller part)
static int ride_wgs(const mamdr_ctx* c, bool with_loss) {
    return std::max(0, std::min(FZ_RIDE_CAP, c->n_cu - wgrad_adam_own_wgs(with_loss)));
}
// small steps run the 4-row-tile tower (all CUs busy), the others the 16-row one (the only one of the Star tower)
static bool takes_tower4(const mamdr_ctx* c, int64_t rows_pad) {
    return !c->star && c->tower_tile != 16 && (c->tower_tile == 4 || rows_pad <= c->tower4_max_rows);
}
// every k_tower4 launch this context can make reads W1 from its LDS image: the largest batch that tower takes (tile 4
// forced: any batch the context accepts) still fits one round of workgroups
static bool w1t_unread_now(const mamdr_ctx* c) {
    if (!c->fused || c->tower_tile == 16) return false;
    const int64_t max4 = c->tower_tile == 4 ? c->rows_pad_max : std::min<int64_t>(c->tower4_max_rows, c->rows_pad_max);
    return tower4_never_streams(max4, c->t4_no_w1l);
}
// ... and every training call takes the k_wgrad_adam path over a pre-gathered pass, so that each of those launches can
// be the instance that reads W2 in place: no batch the context accepts goes to the slab path (whose towers read W2T)
static bool w2t_unread_now(const mamdr_ctx* c) {
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
    fill_emb_args(c, MAMDR_OPT_ADAM, alpha, P.omb1, P.omb2, table_two_l2(c), rows, c->star ? XDIM : 2 * EMB, nea);
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
    memset(&pa, 0, sizeof(pa));
    pa.blk = blk;
    pa.SL = c->SL;
    pa.L = c->L;
    pa.n_domain = c->cfg.n_domain;
    pa.d = domain;
    pa.eff = c->eff;
    pa.pn = c->pn;
    pa.part = c->star_part;
    pa.n_chunks = chunks;
    pa.rows = rows;
    pa.aux = c->aux;
    pa.AL = c->AL;
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
    wa.w0dom = c->eff + c->L.w0 + (size_t)(2 * EMB) * H1;
    wa.w0dom_copy = c->w0dom_copy;
    wa.loss_part = c->loss_part;
    wa.n_loss_tiles = rows_pad / TILE_ROWS;
    wa.rows = rows;
    wa.dense = c->eff;
    wa.dm_count = 0;              // no regularisers in this tower: loss = mean BCE
    wa.l2_emb = 0.f;
    wa.frozen_sumsq = c->frozen_sumsq;
    wa.loss_out = loss_out;
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
        fill_emb_args(c, optimizer, alpha, omb1, omb2, table_two_l2(c), rows, XDIM, tea);
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
    ua.opt.optimizer = optimizer;
    ua.opt.alpha = alpha;
    ua.opt.omb1 = omb1;
    ua.opt.omb2 = omb2;
    ua.opt.eps = c->cfg.adam_eps;
    ua.opt.two_l2 = 0.f;
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
    fa.optimizer = optimizer;
    fa.alpha = alpha;
    fa.omb1 = P.omb1;
    fa.omb2 = P.omb2;
    fa.eps = c->cfg.adam_eps;
    fa.two_l2 = 2.0f * c->cfg.l2_emb;
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
    dm_pending.optimizer = optimizer;
    dm_pending.alpha = alpha;
    dm_pending.omb1 = P.omb1;
    dm_pending.omb2 = P.omb2;
    dm_pending.eps = c->cfg.adam_eps;
    dm_pending.two_l2 = 2.0f * c->cfg.l2_emb;
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
        // the regulariser of the reported loss needs the current tables' sums of squares
        launch_sumsq(c->params, (int64_t)c->cfg.n_user * EMB, c->sumsq_partials, c->frozen_sumsq + 0, c->stream);
        launch_sumsq(c->params + (size_t)c->cfg.n_user * EMB, (int64_t)c->cfg.n_item * EMB, c->sumsq_partials,
                     c->frozen_sumsq + 1, c->stream);
        if (c->deepfm) {
            launch_sumsq(c->params + c->lin_user_off, c->cfg.n_user, c->sumsq_partials, c->frozen_sumsq + 2, c->stream);
            launch_sumsq(c->params + c->lin_item_off, c->cfg.n_item, c->sumsq_partials, c->frozen_sumsq + 3, c->stream);
        }
    }
    WgradArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.acts = c->acts;
    wa.dz = c->dz;
    wa.dlogit = c->dlogit;
    wa.domrow = c->domrow;
    wa.fmq = c->fmq;
    wa.ipbuf = c->ipbuf;
    wa.ld_off = c->L.ld;
    wa.ld_count = c->L.ld_count;
    wa.l2_lin = c->cfg.l2_linear;
    wa.lv_off = c->L.lv;
    wa.lv_count = c->L.lv_count;
    wa.uw_d = P.domain;
    wa.tiles = c->tiles;
    wa.n_tiles = c->n_tiles;
    wa.rows_pad = rows_pad;
    int rpg = 0;
    const int groups = wgrad_groups(rows_pad, &rpg);
    wa.n_groups = groups;
    wa.rows_per_group = rpg;
    wa.slabs = c->slabs;
    wa.slab_ld = c->slab_ld;
    wa.w0dom = c->params + c->table_floats + c->L.w0 + (size_t)(2 * EMB) * H1;
    wa.w0dom_copy = c->w0dom_copy;
    wa.dm_copy = c->lin_w0dom ? c->dm_copy : nullptr;
    wa.loss_part = c->loss_part;
    wa.n_loss_tiles = use4 ? rows_pad / 4 : rows_pad / TILE_ROWS;
    wa.rows = rows;
    wa.dense = c->params + c->table_floats;
    wa.dm_count = c->cfg.n_domain * EMB;
    wa.l2_emb = c->cfg.l2_emb;
    wa.frozen_sumsq = c->frozen_sumsq;
    wa.loss_out = P.loss_out ? P.loss_out + s : nullptr;
#ifdef MAMDR_STAMPS
    wa.stamps = c->stamps ? c->stamps + 65536 : nullptr;
#endif
    // lazy table Adam: k_emb_reduce (and DeepFM's k_lin_sweep) only need the tower's outputs and write state no dense
    // kernel touches -> they ride in k_wgrad's / k_update's launches
    EmbStepArgs tea, nea;
    EmbRowsArgs nr;
    const bool next = P.tail && s + 1 < P.n_steps;
    if (P.tail) {
        fill_emb_args(c, optimizer, alpha, omb1, omb2, table_two_l2(c), rows, 2 * EMB, tea);
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
    ua.two_l2 = 2.0f * c->cfg.l2_emb;
    ua.s2_off = c->s2_off;
    ua.ld_off = c->L.ld;
    ua.ld_count = c->L.ld_count;
    ua.two_l2_lin = 2.0f * c->cfg.l2_linear;
    ua.optimizer = optimizer;
    ua.alpha = alpha;
    ua.omb1 = omb1;
    ua.omb2 = omb2;
    ua.eps = c->cfg.adam_eps;
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

extern char** environ;
namespace mamdr {
// once per process (thread-safe static initialiser): a MAMDR_* name in the environment that nobody reads is reported
int env_warn_unknown() {
    static const int unknown = []() {
        int n = 0;
        for (char** e = environ; e && *e; ++e) {
            if (strncmp(*e, "MAMDR_", 6) != 0) continue;
            const char* eq = strchr(*e, '=');
            const size_t len = eq ? (size_t)(eq - *e) : strlen(*e);
            bool known = false;
            for (int i = 0; i < kNumEnvSwitches && !known; ++i) {
                const char* k = kEnvSwitches[i].name;
                const size_t kl = strlen(k);
                if (kl && k[kl - 1] == '*') known = len >= kl - 1 && strncmp(*e, k, kl - 1) == 0;
                else known = len == kl && strncmp(*e, k, kl) == 0;
            }
            if (!known) {
                fprintf(stderr, "mamdr: environment variable %.*s is not a switch this build reads (mamdr_env_switches() lists them)\n",
                        (int)len, *e);
                n += 1;
            }
        }
        return n;
    }();
    return unknown;
}
}  // namespace mamdr

extern "C" {

const char* mamdr_last_error(void) { return g_err; }
int mamdr_abi_version(void) { return MAMDR_ABI_VERSION; }

// ---- environment switches: one table (env_registry.h), handed out and checked against the process environment
const char* mamdr_env_switches(void) {
    static const std::string table = []() {
        std::string t;
        for (int i = 0; i < kNumEnvSwitches; ++i)
            t += std::string(kEnvSwitches[i].name) + "\t" + kEnvSwitches[i].reader + "\t" + kEnvSwitches[i].effect + "\n";
        return t;
    }();
    return table.c_str();
}
int mamdr_env_unknown(void) { return mamdr::env_warn_unknown(); }


int mamdr_create(const mamdr_config* cfg, void* stream, mamdr_ctx** out) {
    (void)mamdr::env_warn_unknown();
    if (!cfg || !out) return fail(MAMDR_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->abi_version != MAMDR_ABI_VERSION)
        return fail(MAMDR_EINVAL, "abi_version %d != %d", cfg->abi_version, MAMDR_ABI_VERSION);
    if (cfg->tower != MAMDR_TOWER_MLP && cfg->tower != MAMDR_TOWER_DEEPFM && cfg->tower != MAMDR_TOWER_STAR &&
        cfg->tower != MAMDR_TOWER_WDL && cfg->tower != MAMDR_TOWER_PNN && cfg->tower != MAMDR_TOWER_NFM)
        return fail(MAMDR_EINVAL, "unknown tower kind %d", cfg->tower);
    if (cfg->emb_dim != EMB || cfg->hidden[0] != H1 || cfg->hidden[1] != H2 || cfg->hidden[2] != H3)
        return fail(MAMDR_EINVAL, "kernels are specialised for emb_dim 128 and hidden (256,128,64); got %d (%d,%d,%d)",
                    cfg->emb_dim, cfg->hidden[0], cfg->hidden[1], cfg->hidden[2]);
    if (cfg->n_user <= 0 || cfg->n_item <= 0 || cfg->n_domain <= 0)
        return fail(MAMDR_EINVAL, "n_user/n_item/n_domain must be positive");
    if (cfg->max_batch <= 0 || cfg->max_batch % TILE_ROWS != 0)
        return fail(MAMDR_EINVAL, "max_batch must be a positive multiple of %d", TILE_ROWS);
    if (cfg->max_batch > 16384) return fail(MAMDR_EINVAL, "max_batch %d exceeds 16384", cfg->max_batch);
    if (!(cfg->dropout >= 0.f && cfg->dropout < 1.f)) return fail(MAMDR_EINVAL, "dropout rate must be in [0,1)");
    if (cfg->uncertainty_weight && cfg->tower == MAMDR_TOWER_STAR)
        return fail(MAMDR_ENOTBUILT, "uncertainty weighting is built for the deepctr towers of the step kernels (mlp / deepfm / wdl / pnn / nfm)");
    if ((cfg->tower == MAMDR_TOWER_PNN || cfg->tower == MAMDR_TOWER_NFM) && cfg->max_batch > 2048)
        return fail(MAMDR_ENOTBUILT, "the pnn / nfm towers' training step is built on the four-row tower: batches of up to 2,048 rows, "
                                     "not %d (the generic-layer engine, mamdr_graph_*, takes any batch size)", cfg->max_batch);

    mamdr_ctx* c = new (std::nothrow) mamdr_ctx();
    if (!c) return fail(MAMDR_EINVAL, "out of host memory");
    c->cfg = *cfg;
    c->stream = (hipStream_t)stream;
    c->nfm = cfg->tower == MAMDR_TOWER_NFM;
    c->deepfm = cfg->tower == MAMDR_TOWER_DEEPFM || cfg->tower == MAMDR_TOWER_WDL || c->nfm;   // linear tables (+ FM term)
    c->pnn = cfg->tower == MAMDR_TOWER_PNN;
    c->L = DenseLayout::make(cfg->n_domain, c->deepfm, cfg->uncertainty_weight != 0, c->pnn);
    c->table_floats = cfg->emb_trainable ? ((int64_t)cfg->n_user + cfg->n_item) * EMB : 0;
    if (c->deepfm && cfg->emb_trainable) {
        // each 1-d table padded to 4 floats so that the dense block stays 16-B aligned
        c->lin_user_off = c->table_floats;
        c->lin_item_off = c->lin_user_off + (((int64_t)cfg->n_user + 3) & ~(int64_t)3);
        c->table_floats = c->lin_item_off + (((int64_t)cfg->n_item + 3) & ~(int64_t)3);
    }
    c->star = cfg->tower == MAMDR_TOWER_STAR;
    c->SL = StarLayout::make(cfg->n_domain);
    c->AL = StarAuxLayout::make(cfg->n_domain);
    c->n_params = c->table_floats + (c->star ? c->SL.alloc : c->L.alloc);
    c->n_meta = c->star ? c->table_floats + c->SL.n_meta : c->n_params;
    c->data.resize((size_t)cfg->n_domain * 3);
    c->rows_pad_max = cfg->max_batch;
    if (const char* tt = getenv("MAMDR_TOWER_TILE")) c->tower_tile = atoi(tt);
    c->slab_ld = c->L.alloc + cfg->n_domain * H1;
    if (c->deepfm || c->pnn) {      // per-row terms of the domain-table gradient: S2 = onehot(domain)^T fmq
        c->s2_off = c->slab_ld;
        c->slab_ld += cfg->n_domain * EMB;
    }

    const size_t rp = (size_t)c->rows_pad_max;
    // dW0[256:384] without tiles: Dm^T . S in k_update, or (Star: one normalised domain row per batch) the
    // rank-1 form in k_star_update
    // (NFM: rows 256..383 of the input tile carry the bi-interaction, not the domain row: plain tiles)
    c->lin_w0dom = (c->star || cfg->n_domain <= 64) && !c->nfm;
    std::vector<TileDesc> tiles = build_tiles(c->L, cfg->n_domain, c->deepfm, c->s2_off, c->lin_w0dom, c->star, c->pnn, c->nfm);
    c->n_tiles = (int)tiles.size();
    float thr[500];
    thr[0] = (float)(0.0 - 1e-7);
    for (int i = 0; i < 498; ++i) thr[i + 1] = (float)((double)(i + 1) * 1.0 / (double)(500 - 1));
    thr[499] = (float)(1.0 + 1e-7);

#define ALLOC(ptr, bytes)                                                        \
    do {                                                                         \
        hipError_t e_ = hipMalloc((void**)&(ptr), (bytes));                      \
        if (e_ != hipSuccess) {                                                  \
            mamdr_destroy(c);                                                    \
            return fail(MAMDR_EHIP, "hipMalloc(%zu): %s", (size_t)(bytes), hipGetErrorString(e_)); \
        }                                                                        \
    } while (0)
    ALLOC(c->acts, rp * ACT_LD * sizeof(float));
    ALLOC(c->dz, rp * DZ_LD * sizeof(float));
    ALLOC(c->dlogit, rp * sizeof(float));
    ALLOC(c->w0dom_copy, (size_t)EMB * H1 * sizeof(float));
    ALLOC(c->dm_copy, (size_t)cfg->n_domain * EMB * sizeof(float));
    if (c->star) {
        const size_t chunks = (rp + STAR_CHUNK - 1) / STAR_CHUNK;
        ALLOC(c->eff, (size_t)c->L.alloc * sizeof(float));
        ALLOC(c->pn, (size_t)PN_WS_FLOATS * sizeof(float));
        ALLOC(c->star_alpha, (size_t)STAR_ALPHA_CAP * sizeof(float));
        if (const char* sd = getenv("MAMDR_STAR_DENSE_SLICES")) c->star_dense_slices = atoi(sd) != 0;
        ALLOC(c->star_part, chunks * 2 * XDIM * sizeof(double));    // forward: double sums; backward: float sums
        ALLOC(c->star_sums, (4 * XDIM + EMB) * sizeof(float));      // sums | domain-row gradient | s1 / B, s2 / B
        ALLOC(c->star_dmpart, chunks * EMB * sizeof(float));
    }
    if (cfg->emb_trainable || c->star) {
        ALLOC(c->dxe, rp * (c->star ? XDIM : 2 * EMB) * sizeof(float));
        ALLOC(c->urow, rp * sizeof(int32_t));
        ALLOC(c->irow, rp * sizeof(int32_t));
    }
    if (cfg->emb_trainable) {
        ALLOC(c->map_u, (size_t)cfg->n_user * sizeof(int32_t));
        ALLOC(c->map_i, (size_t)cfg->n_item * sizeof(int32_t));
        ALLOC(c->urow_alt, rp * sizeof(int32_t));
        ALLOC(c->irow_alt, rp * sizeof(int32_t));
        ALLOC(c->map_u_alt, (size_t)cfg->n_user * sizeof(int32_t));
        ALLOC(c->map_i_alt, (size_t)cfg->n_item * sizeof(int32_t));
        ALLOC(c->gbuf_u, rp * EMB * sizeof(float));
        ALLOC(c->gbuf_i, rp * EMB * sizeof(float));
        ALLOC(c->hasdup_u, rp * sizeof(int32_t));
        ALLOC(c->hasdup_i, rp * sizeof(int32_t));
        const char* dense_env = getenv("MAMDR_DENSE_ADAM");
        c->lazy = !(dense_env && atoi(dense_env) != 0);
        if (const char* fe = getenv("MAMDR_LAZY_FLUSH_EVERY")) c->flush_every = atoi(fe) > 0 ? atoi(fe) : c->flush_every;
        if (const char* cap_env = getenv("MAMDR_LAZY_LOG_CAP")) {      // tests: force the alpha ring to wrap
            const int cap = atoi(cap_env);
            if (cap >= 4 && (cap & (cap - 1)) == 0) c->log_cap = cap;
        }
        ALLOC(c->last_u, (size_t)cfg->n_user * sizeof(int32_t));
        ALLOC(c->last_i, (size_t)cfg->n_item * sizeof(int32_t));
        ALLOC(c->alpha_log, (size_t)c->log_cap * sizeof(float));
        if (c->deepfm) {
            ALLOC(c->glin_u, rp * sizeof(float));
            ALLOC(c->glin_i, rp * sizeof(float));
        }
    }
    if (c->deepfm || c->pnn) ALLOC(c->fmq, rp * EMB * sizeof(float));
    if (c->pnn) ALLOC(c->ipbuf, rp * 4 * sizeof(float));
    ALLOC(c->domrow, rp * sizeof(int32_t));
    ALLOC(c->loss_part, (rp / 4) * sizeof(float));
    ALLOC(c->wT, (size_t)WT_FLOATS * sizeof(float));
    {
        if (const char* nw = getenv("MAMDR_T4_NO_W1L")) c->t4_no_w1l = atoi(nw) != 0;
        // Which tower for how many rows (frozen-table mlp, measured at 2,048 rows of Taobao-10, us / step): k_tower4 +
        // k_wgrad_adam 40.4 (512 four-row tiles: two rounds of workgroups, no W1 image), k_tower + k_wgrad_adam 39.0,
        // k_tower + k_wgrad + k_update 38.6 (128 sixteen-row tiles, the lean instance: 21.4 us against k_tower4's 26.9).
        // So the four-row tower and the fused path serve what fits ONE round of workgroups (4 rows x CUs = 1,024 rows);
        // with trainable tables or the DeepFM terms the four-row tower stays ahead up to 2,048 rows (Amazon-6 at
        // 2,048: 29.3 vs 34.2 us).
        {
            int dev = 0, n_cu = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                n_cu <= 0)
                n_cu = 256;
            c->n_cu = n_cu;
            const int one_round = std::min(2048, std::max(256, 4 * n_cu));
            c->fused_max_batch = one_round;
            if (cfg->tower == MAMDR_TOWER_MLP && !cfg->emb_trainable) c->tower4_max_rows = one_round;
        }
        const char* fe = getenv("MAMDR_FUSED");
        c->fused = cfg->tower == MAMDR_TOWER_MLP && !cfg->emb_trainable && !cfg->uncertainty_weight && c->lin_w0dom &&
                   cfg->n_domain <= 64 && !(fe && atoi(fe) == 0);
        if (c->fused && fe && atoi(fe) == 2) c->fused_max_batch = 1 << 30;
        if (c->fused) {
            ALLOC(c->pdm, (size_t)DM_PARTS * cfg->n_domain * EMB * sizeof(float));
            ALLOC(c->dmsnap[0], (size_t)3 * cfg->n_domain * EMB * sizeof(float));
            ALLOC(c->dmsnap[1], (size_t)3 * cfg->n_domain * EMB * sizeof(float));
            if (const char* de = getenv("MAMDR_DM_EACH")) c->dm_finish_each = atoi(de) != 0;
            if (const char* de = getenv("MAMDR_DM_CALL")) c->dm_finish_call = atoi(de) != 0;
            if (const char* de = getenv("MAMDR_NO_W2_DIRECT")) c->w2_direct_ok = atoi(de) == 0;
            if (const char* pe = getenv("MAMDR_NO_PREGATHER")) c->use_pre = atoi(pe) == 0;
            if (const char* pe = getenv("MAMDR_NO_PREGATHER_RIDE")) c->ride_on = atoi(pe) == 0;
            if (const char* se = getenv("MAMDR_FZ_S_INORDER")) c->fz_s_inorder = atoi(se) != 0;
            if (const char* se = getenv("MAMDR_FZ_DEAL_RESIDUE")) c->fz_deal_residue = atoi(se) != 0;
        }
        c->w1t_unread = w1t_unread_now(c);
        c->w2t_unread = w2t_unread_now(c);
    }
    if (const char* ev = getenv("MAMDR_NO_TAILFUSE")) c->tail_fuse = atoi(ev) == 0;
    if (const char* ev = getenv("MAMDR_REC_CHUNK"))
        if (atoi(ev) > 0) c->rec_chunk = (int)std::min<int64_t>(((int64_t)atoi(ev) + REC_TILE - 1) / REC_TILE * REC_TILE, 1 << 20);
    ALLOC(c->slabs, (size_t)WGRAD_MAX_GROUPS * c->slab_ld * sizeof(float));
    ALLOC(c->tiles, tiles.size() * sizeof(TileDesc));
    ALLOC(c->thresholds, sizeof(thr));
    ALLOC(c->frozen_sumsq, 4 * sizeof(float));
    ALLOC(c->sumsq_partials, 1024 * sizeof(float));
#undef ALLOC
    hipError_t e = hipMemsetAsync(c->slabs, 0, (size_t)WGRAD_MAX_GROUPS * c->slab_ld * sizeof(float), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->frozen_sumsq, 0, 4 * sizeof(float), c->stream);
    if (cfg->emb_trainable) {
        if (e == hipSuccess) e = hipMemsetAsync(c->hasdup_u, 0, rp * sizeof(int32_t), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->hasdup_i, 0, rp * sizeof(int32_t), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->last_u, 0, (size_t)cfg->n_user * sizeof(int32_t), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->last_i, 0, (size_t)cfg->n_item * sizeof(int32_t), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->alpha_log, 0, (size_t)c->log_cap * sizeof(float), c->stream);
        launch_emb_map_init(c->map_u, cfg->n_user, c->stream);
        launch_emb_map_init(c->map_i, cfg->n_item, c->stream);
        launch_emb_map_init(c->map_u_alt, cfg->n_user, c->stream);
        launch_emb_map_init(c->map_i_alt, cfg->n_item, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(c->tiles, tiles.data(), tiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->thresholds, thr, sizeof(thr), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // host staging buffers go out of scope
    if (e != hipSuccess) {
        mamdr_destroy(c);
        return fail(MAMDR_EHIP, "workspace initialisation: %s", hipGetErrorString(e));
    }
    *out = c;
    return MAMDR_OK;
}

int mamdr_destroy(mamdr_ctx* c) {
    if (!c) return MAMDR_OK;
    for (int k = 0; k < MAMDR_KERNEL_COUNT; ++k)
        for (EventPair& p : c->ev[k]) {
            if (p.own_a) (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    void* ptrs[] = {c->urow_alt, c->irow_alt, c->map_u_alt, c->map_i_alt, c->acts, c->dz, c->dlogit, c->w0dom_copy, c->dm_copy, c->wT, c->dxe, c->urow, c->irow, c->map_u, c->map_i, c->gbuf_u, c->gbuf_i, c->hasdup_u, c->hasdup_i, c->last_u, c->last_i, c->alpha_log, c->star_alpha, c->pdm, c->dmsnap[0], c->dmsnap[1], c->xpre, c->pdom, c->plabel, c->xpre_ahead, c->pdom_ahead, c->plabel_ahead, c->fmq, c->ipbuf, c->glin_u, c->glin_i, c->eff, c->pn, c->star_part, c->star_sums, c->star_dmpart, c->domrow, c->loss_part, c->eval_part, c->slabs,
                    c->rec_P, c->rec_lin, c->rec_q, c->rec_part, c->rec_best,
                    c->tiles, c->thresholds, c->frozen_sumsq, c->sumsq_partials};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete c;
    return MAMDR_OK;
}

int64_t mamdr_param_count(const mamdr_ctx* c) { return c ? c->n_params : 0; }
int64_t mamdr_meta_count(const mamdr_ctx* c) { return c ? c->n_meta : 0; }
int64_t mamdr_aux_count(const mamdr_ctx* c) { return (c && c->star) ? c->AL.count : 0; }

int mamdr_bind_aux(mamdr_ctx* c, float* d_aux) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (!c->star) return fail(MAMDR_ESTATE, "this tower has no auxiliary state");
    if (!d_aux || ((uintptr_t)d_aux & 15)) return fail(MAMDR_EINVAL, "aux pointer null or not 16-byte aligned");
    c->aux = d_aux;
    return MAMDR_OK;
}

int mamdr_param_segment(const mamdr_ctx* c, int seg, int64_t* offset, int64_t* count) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (!offset || !count) return fail(MAMDR_EINVAL, "null argument");
    const DenseLayout& L = c->L;
    const int64_t base = c->table_floats;
    int64_t off = 0, cnt = 0;
    if (c->star) {
        const StarLayout& S = c->SL;
        const int64_t D = c->cfg.n_domain;
        const bool tr = c->cfg.emb_trainable != 0;
        if (seg >= MAMDR_SEG_STAR_WS0 && seg <= MAMDR_SEG_STAR_WS2) {
            off = base + S.ws[seg - MAMDR_SEG_STAR_WS0]; cnt = StarLayout::ksize(seg - MAMDR_SEG_STAR_WS0);
        } else if (seg >= MAMDR_SEG_STAR_BS0 && seg <= MAMDR_SEG_STAR_BS2) {
            off = base + S.bs[seg - MAMDR_SEG_STAR_BS0]; cnt = StarLayout::bsize(seg - MAMDR_SEG_STAR_BS0);
        } else if (seg >= MAMDR_SEG_STAR_WD0 && seg <= MAMDR_SEG_STAR_WD2) {
            off = base + S.wd[seg - MAMDR_SEG_STAR_WD0]; cnt = D * StarLayout::ksize(seg - MAMDR_SEG_STAR_WD0);
        } else if (seg >= MAMDR_SEG_STAR_BD0 && seg <= MAMDR_SEG_STAR_BD2) {
            off = base + S.bd[seg - MAMDR_SEG_STAR_BD0]; cnt = D * StarLayout::bsize(seg - MAMDR_SEG_STAR_BD0);
        } else {
            switch (seg) {
                case MAMDR_SEG_USER_EMB: off = 0; cnt = tr ? (int64_t)c->cfg.n_user * EMB : 0; break;
                case MAMDR_SEG_ITEM_EMB: off = tr ? (int64_t)c->cfg.n_user * EMB : 0; cnt = tr ? (int64_t)c->cfg.n_item * EMB : 0; break;
                case MAMDR_SEG_DOMAIN_EMB: off = base + S.dm; cnt = D * EMB; break;
                case MAMDR_SEG_PN_GAMMA_SHARED: off = base + S.pgs; cnt = XDIM; break;
                case MAMDR_SEG_PN_BETA_SHARED: off = base + S.pbs; cnt = XDIM; break;
                case MAMDR_SEG_PN_GAMMA_SPEC: off = base + S.pgd; cnt = D * XDIM; break;
                case MAMDR_SEG_PN_BETA_SPEC: off = base + S.pbd; cnt = D * XDIM; break;
                case MAMDR_SEG_WO: off = base + S.wo; cnt = H3; break;
                case MAMDR_SEG_GB: off = base + S.gb; cnt = 1; break;
                default:
                    if (seg < 0 || seg >= MAMDR_SEG_COUNT) return fail(MAMDR_EINVAL, "unknown segment %d", seg);
                    off = 0; cnt = 0;      // a segment of another tower
            }
        }
        *offset = off;
        *count = cnt;
        return MAMDR_OK;
    }
    if (seg >= MAMDR_SEG_STAR_WS0 && seg <= MAMDR_SEG_STAR_BD2) {  // Star segments are absent from this tower
        *offset = 0;
        *count = 0;
        return MAMDR_OK;
    }
    switch (seg) {
        case MAMDR_SEG_USER_EMB: off = 0; cnt = c->cfg.emb_trainable ? (int64_t)c->cfg.n_user * EMB : 0; break;
        case MAMDR_SEG_ITEM_EMB:
            off = c->cfg.emb_trainable ? (int64_t)c->cfg.n_user * EMB : 0;
            cnt = c->cfg.emb_trainable ? (int64_t)c->cfg.n_item * EMB : 0;
            break;
        case MAMDR_SEG_DOMAIN_EMB: off = base + L.dm; cnt = (int64_t)c->cfg.n_domain * EMB; break;
        case MAMDR_SEG_W0:
            off = base + L.w0 + (c->nfm ? 2 * EMB * H1 : 0);
            cnt = c->nfm ? EMB * H1 : XDIM * H1;
            break;
        case MAMDR_SEG_W1: off = base + L.w1; cnt = H1 * H2; break;
        case MAMDR_SEG_W2: off = base + L.w2; cnt = H2 * H3; break;
        case MAMDR_SEG_B0: off = base + L.b0; cnt = H1; break;
        case MAMDR_SEG_B1: off = base + L.b1; cnt = H2; break;
        case MAMDR_SEG_B2: off = base + L.b2; cnt = H3; break;
        case MAMDR_SEG_WO: off = base + L.wo; cnt = H3; break;
        case MAMDR_SEG_GB: off = base + L.gb; cnt = 1; break;
        case MAMDR_SEG_LIN_USER:
            off = c->lin_user_off;
            cnt = (c->deepfm && c->cfg.emb_trainable) ? c->cfg.n_user : 0;
            break;
        case MAMDR_SEG_LIN_ITEM:
            off = c->lin_item_off;
            cnt = (c->deepfm && c->cfg.emb_trainable) ? c->cfg.n_item : 0;
            break;
        case MAMDR_SEG_LIN_DOMAIN: off = base + L.ld; cnt = L.ld_count; break;
        case MAMDR_SEG_LOG_VAR: off = base + L.lv; cnt = L.lv_count; break;
        case MAMDR_SEG_W0X: off = base + L.wx; cnt = L.wx_count; break;
        default: return fail(MAMDR_EINVAL, "unknown segment %d", seg);
    }
    *offset = off;
    *count = cnt;
    return MAMDR_OK;
}

int mamdr_bind_state(mamdr_ctx* c, float* d_params, float* d_adam_m, float* d_adam_v) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (!d_params || !d_adam_m || !d_adam_v) return fail(MAMDR_EINVAL, "null state pointer");
    if (((uintptr_t)d_params | (uintptr_t)d_adam_m | (uintptr_t)d_adam_v) & 15)
        return fail(MAMDR_EINVAL, "state pointers must be 16-byte aligned");
    if (c->params) sync_tables(c);
    c->params = d_params;
    c->adam_m = d_adam_m;
    c->adam_v = d_adam_v;
    return MAMDR_OK;
}

int mamdr_optimizer_reset(mamdr_ctx* c) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (!c->adam_m) return fail(MAMDR_ESTATE, "mamdr_bind_state has not been called");
    sync_tables(c);             // pending moves of the lagging rows belong to the old optimiser state
    if (c->last_u) {
        HIP_TRY(hipMemsetAsync(c->last_u, 0, (size_t)c->cfg.n_user * sizeof(int32_t), c->stream));
        HIP_TRY(hipMemsetAsync(c->last_i, 0, (size_t)c->cfg.n_item * sizeof(int32_t), c->stream));
    }
    c->flush_t = 0;
    HIP_TRY(hipMemsetAsync(c->adam_m, 0, (size_t)c->n_params * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->adam_v, 0, (size_t)c->n_params * sizeof(float), c->stream));
    c->adam_t = 0;
    c->b1p = 1.0f;
    c->b2p = 1.0f;
    return MAMDR_OK;
}

int64_t mamdr_optimizer_steps(const mamdr_ctx* c) { return c ? c->adam_t : 0; }

// Restore the two host-side counters of a run (a checkpoint's `beta1_power` / `beta2_power` variables and the position of
// the dropout stream): the live state is brought up to date first (pending domain-table step, lagging table rows), then
// every table row counts as current AT the new step count -- the caller supplies weights and slots that belong to it.
int mamdr_set_counters(mamdr_ctx* c, int64_t optimizer_steps, int64_t dropout_steps) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (optimizer_steps < 0 || optimizer_steps > (int64_t)0x7ffffff0 || dropout_steps < 0 || dropout_steps > (int64_t)0xffffffffLL)
        return fail(MAMDR_EINVAL, "mamdr_set_counters(%lld, %lld): out of range", (long long)optimizer_steps, (long long)dropout_steps);
    if (!c->adam_m) return fail(MAMDR_ESTATE, "mamdr_bind_state has not been called");
    sync_tables(c);
    if (c->last_u) {
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->last_u), (int)optimizer_steps, (size_t)c->cfg.n_user, c->stream));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->last_i), (int)optimizer_steps, (size_t)c->cfg.n_item, c->stream));
    }
    c->flush_t = optimizer_steps;
    c->adam_t = optimizer_steps;
    float b1 = 1.0f, b2 = 1.0f;                 // TF's running products, one fp32 rounding per step (as the step loop forms them)
    for (int64_t t = 0; t < optimizer_steps; ++t) {
        const float n1 = b1 * c->cfg.adam_beta1, n2 = b2 * c->cfg.adam_beta2;
        // both products at a fixed point: every further step leaves them as they are.  0.9 / 0.999 end on denormal fixed
        // points (4 and 500 x 2^-149) after ~1,000 / ~1.6e5 steps; beta = 1 keeps the product at 1 from the start
        if (n1 == b1 && n2 == b2) break;
        b1 = n1;
        b2 = n2;
    }
    c->b1p = b1;
    c->b2p = b2;
    c->global_step = (uint32_t)dropout_steps;
    return MAMDR_OK;
}
int64_t mamdr_table_flushes(const mamdr_ctx* c, int32_t forced_only) {
    return !c ? 0 : forced_only ? c->n_flush_forced : c->n_flush;
}

int mamdr_sync_tables(mamdr_ctx* c) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    sync_tables(c);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_bind_accumulator(mamdr_ctx* c, float* d_acc) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (!d_acc || ((uintptr_t)d_acc & 15)) return fail(MAMDR_EINVAL, "accumulator pointer null or not 16-byte aligned");
    c->accum = d_acc;
    return MAMDR_OK;
}

int mamdr_bind_table(mamdr_ctx* c, int seg, const float* d_rows, int64_t n_rows) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (c->cfg.emb_trainable) return fail(MAMDR_ESTATE, "tables are trainable: they live in the flat vector");
    if (!d_rows || ((uintptr_t)d_rows & 15)) return fail(MAMDR_EINVAL, "table pointer null or not 16-byte aligned");
    drop_pregathered(c);        // rows gathered ahead of their calls came from the old table
    if (seg == MAMDR_SEG_USER_EMB) {
        if (n_rows != c->cfg.n_user) return fail(MAMDR_EINVAL, "user table has %lld rows, config says %d", (long long)n_rows, c->cfg.n_user);
        c->user_tab = d_rows;
        launch_sumsq(d_rows, n_rows * EMB, c->sumsq_partials, c->frozen_sumsq + 0, c->stream);
    } else if (seg == MAMDR_SEG_ITEM_EMB) {
        if (n_rows != c->cfg.n_item) return fail(MAMDR_EINVAL, "item table has %lld rows, config says %d", (long long)n_rows, c->cfg.n_item);
        c->item_tab = d_rows;
        launch_sumsq(d_rows, n_rows * EMB, c->sumsq_partials, c->frozen_sumsq + 1, c->stream);
    } else {
        return fail(MAMDR_EINVAL, "segment %d is not a bindable table", seg);
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_bind_domain_data(mamdr_ctx* c, int domain, int split, const int32_t* d_uid, const int32_t* d_pid,
                           const int32_t* d_domain, const float* d_label, int64_t n_rows) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    SplitData* d = split_of(c, domain, split);
    if (!d) return fail(MAMDR_EINVAL, "domain %d / split %d out of range", domain, split);
    if (n_rows < 0 || n_rows > 0x7fffffff) return fail(MAMDR_EINVAL, "n_rows out of range");
    if (n_rows > 0 && (!d_uid || !d_pid || !d_domain || !d_label)) return fail(MAMDR_EINVAL, "null column pointer");
    d->bound = true;
    d->uid = d_uid;
    d->pid = d_pid;
    d->dom = d_domain;
    d->label = d_label;
    d->n = n_rows;
    drop_pregathered(c);        // (a pass gathered ahead of its call may have come from the old columns)
    const int64_t tiles = (n_rows + TILE_ROWS - 1) / TILE_ROWS;
    if (tiles > c->eval_part_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->eval_part) HIP_TRY(hipFree(c->eval_part));
        c->eval_part = nullptr;
        HIP_TRY(hipMalloc((void**)&c->eval_part, (size_t)tiles * sizeof(float)));
        c->eval_part_cap = tiles;
    }
    return MAMDR_OK;
}

// a set of the pass buffer holds at least `rows` positions (its contents are lost when it grows; the other set stays)
static int grow_pass_set(float*& xpre, int32_t*& pdom, float*& plabel, int64_t& have, int64_t rows) {
    if (rows <= have) return MAMDR_OK;
    const int64_t cap = rows + rows / 4 + 1024;
    if (xpre) { (void)hipFree(xpre); (void)hipFree(pdom); (void)hipFree(plabel); }
    xpre = nullptr; pdom = nullptr; plabel = nullptr; have = 0;
    HIP_TRY(hipMalloc((void**)&xpre, (size_t)cap * 2 * EMB * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&pdom, (size_t)cap * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&plabel, (size_t)cap * sizeof(float)));
    have = cap;
    return MAMDR_OK;
}
// the current set: what was gathered ahead is dropped with it
static int grow_pass_buffer(mamdr_ctx* c, int64_t rows) {
    if (rows <= c->pre_cap) return MAMDR_OK;
    drop_pregathered(c);
    return grow_pass_set(c->xpre, c->pdom, c->plabel, c->pre_cap, rows);
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
    if (int rc = grow_pass_set(c->xpre_ahead, c->pdom_ahead, c->plabel_ahead, c->pre_cap_ahead, total)) return rc;
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
    if (!d || !d->bound) return fail(MAMDR_ESTATE, "train split of domain %d is not bound", domain);
    if (batch <= 0 || batch > c->cfg.max_batch) return fail(MAMDR_EINVAL, "batch %d outside (0, max_batch=%d]", batch, c->cfg.max_batch);
    if (optimizer != MAMDR_OPT_ADAM && optimizer != MAMDR_OPT_SGD && optimizer != MAMDR_OPT_ACCUMULATE)
        return fail(MAMDR_EINVAL, "unknown optimizer %d", optimizer);
    if (optimizer == MAMDR_OPT_ACCUMULATE && !c->accum)
        return fail(MAMDR_ESTATE, "MAMDR_OPT_ACCUMULATE needs mamdr_bind_accumulator first");
    if (first_step < 0 || n_steps < 0) return fail(MAMDR_EINVAL, "negative step range");
    if (pass_rows < 0) pass_rows = d->n;                 // the whole split
    if (pass_rows > d->n) return fail(MAMDR_EINVAL, "pass of %lld rows exceeds the %lld rows of domain %d",
                                      (long long)pass_rows, (long long)d->n, domain);
    const int64_t pass_steps = (pass_rows + batch - 1) / batch;
    if (first_step + n_steps > pass_steps)
        return fail(MAMDR_EINVAL, "steps [%lld,%lld) exceed the %lld batches of domain %d", (long long)first_step,
                    (long long)(first_step + n_steps), (long long)pass_steps, domain);
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
        pa.train = 0;
        launch_star_prep(pa, c->stream);
        ta.dense = c->eff;
        ta.pn_aff = c->pn;
    }
    {
        Prof p(c, MAMDR_KERNEL_EVAL);
        launch_tower_eval(ta, c->stream);
    }
    if (c->cfg.emb_trainable) {
        launch_sumsq(c->params, (int64_t)c->cfg.n_user * EMB, c->sumsq_partials, c->frozen_sumsq + 0, c->stream);
        launch_sumsq(c->params + (size_t)c->cfg.n_user * EMB, (int64_t)c->cfg.n_item * EMB, c->sumsq_partials,
                     c->frozen_sumsq + 1, c->stream);
        if (c->deepfm) {
            launch_sumsq(c->params + c->lin_user_off, c->cfg.n_user, c->sumsq_partials, c->frozen_sumsq + 2, c->stream);
            launch_sumsq(c->params + c->lin_item_off, c->cfg.n_item, c->sumsq_partials, c->frozen_sumsq + 3, c->stream);
        }
    }
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
    void* old[] = {c->rec_P, c->rec_lin, c->rec_part};
    for (void* p : old)
        if (p) (void)hipFree(p);
    c->rec_P = c->rec_lin = nullptr;
    c->rec_part = nullptr;
    c->rec_cap = 0;
    HIP_TRY(hipMalloc((void**)&c->rec_P, (size_t)chunk * H1 * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->rec_lin, (size_t)chunk * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->rec_part, (size_t)REC_QBLOCK * chunk * sizeof(unsigned long long)));
    if (!c->rec_q) HIP_TRY(hipMalloc((void**)&c->rec_q, (size_t)REC_QBLOCK * (H1 + EMB + 4) * sizeof(float)));
    if (!c->rec_best) HIP_TRY(hipMalloc((void**)&c->rec_best, (size_t)REC_QBLOCK * REC_KMAX * sizeof(unsigned long long)));
    c->rec_cap = chunk;
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
    if ((((uintptr_t)d_uid | (uintptr_t)d_domain | (uintptr_t)d_cand | (uintptr_t)d_excl_ids | (uintptr_t)d_ids_out |
          (uintptr_t)d_scores_out | (uintptr_t)d_scores_all) & 3) || ((uintptr_t)d_excl_off & 7))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned to its element size", fn);
    if ((d_excl_off == nullptr) != (d_excl_ids == nullptr))
        return fail(MAMDR_EINVAL, "%s: the exclusion lists need both their offsets and their ids", fn);
    if (ready(c)) return MAMDR_ESTATE;
    if (!d_cand) n_cand = c->cfg.n_item;
    sync_tables(c);              // lagging table rows and lazily replayed per-domain slices: as mamdr_eval_domain
    prof_break(c);
    const int chunk = (int)std::min<int64_t>(c->rec_chunk, (n_cand + REC_TILE - 1) / REC_TILE * REC_TILE);
    if (int e = grow_rec_workspace(c, chunk)) return e;
    RecArgs a;
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
        pa.train = 0;
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
    a.k = k;
    a.kt = std::min<int>(k, REC_TILE);
    a.tiles_cap = c->rec_cap / REC_TILE;
    a.P = c->rec_P;
    a.lin_i = c->rec_lin;
    a.q0 = c->rec_q;
    a.qud = c->rec_q + (size_t)REC_QBLOCK * H1;
    a.qs = a.qud + (size_t)REC_QBLOCK * EMB;
    a.part = c->rec_part;
    a.best = c->rec_best;
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

// ---- per-user grouped AUC (gauc_kernels.hip): stateless, like the outer updates
int mamdr_group_auc(const float* d_pred, const float* d_label, const int32_t* d_order, int64_t n, const int64_t* d_group_off,
                    int64_t n_groups, const int32_t* d_tile_group, const int64_t* d_tile_first, int64_t n_tiles,
                    uint64_t* d_T, uint32_t* d_P, double* d_result, void* stream) {
    if (!d_result || !d_group_off) return fail(MAMDR_EINVAL, "mamdr_group_auc: null result / group offsets pointer");
    if (n < 0 || n > INT32_MAX) return fail(MAMDR_EINVAL, "mamdr_group_auc: n %lld outside [0, 2^31)", (long long)n);
    if (n_groups < 0 || n_groups > n)
        return fail(MAMDR_EINVAL, "mamdr_group_auc: %lld groups for %lld rows", (long long)n_groups, (long long)n);
    if (n > 0 && (!d_pred || !d_label || !d_order)) return fail(MAMDR_EINVAL, "mamdr_group_auc: null pred / label / order pointer");
    if (n_tiles < 0 || n_tiles > n) return fail(MAMDR_EINVAL, "mamdr_group_auc: n_tiles %lld for %lld rows", (long long)n_tiles, (long long)n);
    if (n_tiles == 0 && (d_tile_group || d_tile_first)) return fail(MAMDR_EINVAL, "mamdr_group_auc: a tile list given without tiles");
    if (n_tiles > 0 && (!d_tile_group || !d_tile_first)) return fail(MAMDR_EINVAL, "mamdr_group_auc: %lld tiles need both of their lists", (long long)n_tiles);
    if ((((uintptr_t)d_pred | (uintptr_t)d_label | (uintptr_t)d_order | (uintptr_t)d_tile_group | (uintptr_t)d_P) & 3) ||
        (((uintptr_t)d_group_off | (uintptr_t)d_tile_first | (uintptr_t)d_T | (uintptr_t)d_result) & 7))
        return fail(MAMDR_EINVAL, "mamdr_group_auc: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    GaucArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = d_pred;
    a.label = d_label;
    a.order = d_order;
    a.group_off = d_group_off;
    a.tile_group = d_tile_group;
    a.tile_first = d_tile_first;
    a.n = n;
    a.n_groups = n_groups;
    a.n_tiles = n_tiles;
    a.n_parts = gauc_parts(n_groups);
    a.result = d_result;
    // the call's own scratch, ordered on its stream: [T if not given | partial sums | P if not given]
    const size_t t_bytes = d_T ? 0 : (size_t)n_groups * sizeof(uint64_t);
    const size_t part_bytes = (size_t)a.n_parts * (sizeof(double) + 2 * sizeof(uint64_t));
    const size_t p_bytes = d_P ? 0 : (size_t)n_groups * sizeof(uint32_t);
    char* ws = nullptr;
    if (t_bytes + part_bytes + p_bytes) HIP_TRY(hipMallocAsync((void**)&ws, t_bytes + part_bytes + p_bytes, s));
    a.T = d_T ? reinterpret_cast<unsigned long long*>(d_T) : reinterpret_cast<unsigned long long*>(ws);
    a.part_num = reinterpret_cast<double*>(ws + t_bytes);
    a.part_rows = reinterpret_cast<unsigned long long*>(a.part_num + a.n_parts);
    a.part_valid = a.part_rows + a.n_parts;
    a.P = d_P ? d_P : reinterpret_cast<uint32_t*>(ws + t_bytes + part_bytes);
    hipError_t e = hipSuccess;
    if (n_groups > 0) {
        e = hipMemsetAsync(a.T, 0, (size_t)n_groups * sizeof(uint64_t), s);
        if (e == hipSuccess) e = hipMemsetAsync(a.P, 0, (size_t)n_groups * sizeof(uint32_t), s);
    }
    if (e == hipSuccess) {
        launch_gauc(a, s);
        e = hipGetLastError();
    }
    if (ws) {
        const hipError_t ef = hipFreeAsync(ws, s);
        if (e == hipSuccess) e = ef;
    }
    if (e != hipSuccess) return fail(MAMDR_EHIP, "mamdr_group_auc: %s", hipGetErrorString(e));
    return MAMDR_OK;
}

// ---- outer updates
static int check_vec(const void* p, const char* name) {
    if (!p) return fail(MAMDR_EINVAL, "%s is null", name);
    if ((uintptr_t)p & 15) return fail(MAMDR_EINVAL, "%s is not 16-byte aligned", name);
    return MAMDR_OK;
}
// (an empty vector -- n = 0 -- may be a null pointer: nothing is read or written)
#define CHECK_VEC(p) do { if (n != 0 && check_vec((p), #p)) return MAMDR_EINVAL; } while (0)

int mamdr_interp(float* d_dst, const float* d_a, const float* d_b, float scale, int64_t n, void* stream) {
    CHECK_VEC(d_dst); CHECK_VEC(d_a); CHECK_VEC(d_b);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    launch_interp(d_dst, d_a, d_b, scale, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_moving_average(float* d_unbiased, float* d_biased, const float* d_value, float decay, float denom, int64_t n,
                         void* stream) {
    CHECK_VEC(d_unbiased); CHECK_VEC(d_biased); CHECK_VEC(d_value);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    if (!(denom > 0.f)) return fail(MAMDR_EINVAL, "moving average: debias denominator %g (local step < 1?)", (double)denom);
    launch_moving_average(d_unbiased, d_biased, d_value, decay, denom, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_merge(float* d_dst, const float* d_theta, const float* d_phi, int32_t mode, int64_t n, void* stream) {
    CHECK_VEC(d_dst); CHECK_VEC(d_theta); CHECK_VEC(d_phi);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    if (mode != MAMDR_MERGE_PLUS && mode != MAMDR_MERGE_TIMES) return fail(MAMDR_EINVAL, "unknown merge mode %d", mode);
    launch_merge(d_dst, d_theta, d_phi, mode, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_dr_advance(float* d_phi, float* d_w, float* d_merged, const float* d_theta, float gamma, int32_t mode,
                     int32_t assign_model, int64_t n, void* stream) {
    CHECK_VEC(d_phi); CHECK_VEC(d_w); CHECK_VEC(d_merged); CHECK_VEC(d_theta);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    if (mode != MAMDR_MERGE_PLUS && mode != MAMDR_MERGE_TIMES) return fail(MAMDR_EINVAL, "unknown merge mode %d", mode);
    launch_dr_advance(d_phi, d_w, d_merged, d_theta, gamma, mode == MAMDR_MERGE_PLUS ? 0 : 1, assign_model != 0, n,
                      (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_dr_advance_live(mamdr_ctx* c, float* d_phi, float* d_merged, const float* d_theta, float gamma, int32_t mode,
                          int32_t assign_model, int64_t meta_off, int64_t n) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (ready(c)) return MAMDR_ESTATE;
    CHECK_VEC(d_phi); CHECK_VEC(d_merged); CHECK_VEC(d_theta);
    if (n < 0 || meta_off < 0 || (meta_off & 3) || meta_off + n > c->n_params)
        return fail(MAMDR_EINVAL, "range [%lld, %lld) outside the %lld live parameters (or not 16-byte aligned)",
                    (long long)meta_off, (long long)(meta_off + n), (long long)c->n_params);
    if (n == 0) return MAMDR_OK;
    if (mode != MAMDR_MERGE_PLUS && mode != MAMDR_MERGE_TIMES) return fail(MAMDR_EINVAL, "unknown merge mode %d", mode);
    float* const w = c->params + meta_off;
    const int64_t dm0 = c->table_floats + c->L.dm, dmn = (int64_t)c->cfg.n_domain * EMB;
    if (c->dm_pending.snap && c->dm_pending.optimizer == MAMDR_OPT_ADAM && dm0 >= meta_off && dm0 + dmn <= meta_off + n &&
        !c->tables_dirty && !c->dm_finish_call) {
        // the pending domain-table step is materialised by the lanes that own its elements (no k_dm_finish launch)
        prof_break(c);
        launch_dr_advance_dm(d_phi, w, d_merged, d_theta, gamma, mode == MAMDR_MERGE_PLUS ? 0 : 1, assign_model != 0, n,
                             c->dm_pending, c->adam_m + dm0, c->adam_v + dm0, (dm0 - meta_off) >> 2, (int)(dmn >> 2), c->stream);
        c->dm_pending.snap = nullptr;
        c->wT_valid = false;
    } else {
        sync_tables(c);
        prof_break(c);
        launch_dr_advance(d_phi, w, d_merged, d_theta, gamma, mode == MAMDR_MERGE_PLUS ? 0 : 1, assign_model != 0, n, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_sub(float* d_dst, const float* d_a, const float* d_b, int64_t n, void* stream) {
    CHECK_VEC(d_dst); CHECK_VEC(d_a); CHECK_VEC(d_b);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    launch_sub(d_dst, d_a, d_b, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_accumulate(float* d_acc, const float* d_a, const float* d_b, const float* d_shared, float divisor,
                     int64_t n, void* stream) {
    CHECK_VEC(d_acc); CHECK_VEC(d_a); CHECK_VEC(d_b);
    if (d_shared && ((uintptr_t)d_shared & 15)) return fail(MAMDR_EINVAL, "d_shared is not 16-byte aligned");
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    if (divisor == 0.f) return fail(MAMDR_EINVAL, "divisor must be non-zero");
    launch_accumulate(d_acc, d_a, d_b, d_shared, divisor, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_apply_accumulated(float* d_dst, float* d_acc, float divisor, float scale, int64_t n, void* stream) {
    CHECK_VEC(d_dst); CHECK_VEC(d_acc);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    launch_apply_accumulated(d_dst, d_acc, divisor, scale, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_adam_apply(float* d_p, float* d_m, float* d_v, const float* d_g, float grad_scale, float lr, float beta1,
                     float beta2, float eps, float beta1_power, float beta2_power, int64_t n, void* stream) {
    CHECK_VEC(d_p); CHECK_VEC(d_m); CHECK_VEC(d_v); CHECK_VEC(d_g);
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    const float alpha = lr * sqrtf(1.0f - beta2_power) / (1.0f - beta1_power);
    launch_adam_apply(d_p, d_m, d_v, d_g, grad_scale, alpha, 1.0f - beta1, 1.0f - beta2, eps, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_pcgrad_project(float* d_final, float* d_aux, const int64_t* h_offsets, const int64_t* h_rows,
                         const int32_t* h_cols, int32_t n_seg, void* stream) {
    if (!d_final || !d_aux || !h_offsets || !h_rows || !h_cols) return fail(MAMDR_EINVAL, "null pointer");
    if (n_seg < 0 || n_seg > PCG_MAX_SEG) return fail(MAMDR_EINVAL, "n_seg %d outside [0, %d]", n_seg, PCG_MAX_SEG);
    PcgArgs a;
    memset(&a, 0, sizeof(a));
    a.fin = d_final;
    a.aux = d_aux;
    a.n_seg = n_seg;
    for (int i = 0; i < n_seg; ++i) {
        if (h_offsets[i] < 0 || h_rows[i] < 0 || h_cols[i] <= 0 || h_cols[i] > 4096)
            return fail(MAMDR_EINVAL, "tensor %d: bad offset / rows / cols", i);
        a.off[i] = h_offsets[i];
        a.cols[i] = h_cols[i];
        a.row_start[i + 1] = a.row_start[i] + h_rows[i];
    }
    launch_pcgrad(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}
int mamdr_copy(float* d_dst, const float* d_src, int64_t n, void* stream) {
    if (!d_dst || !d_src) return fail(MAMDR_EINVAL, "null pointer");
    if (n < 0) return fail(MAMDR_EINVAL, "negative length");
    if (n == 0) return MAMDR_OK;
    if (n == 0) return MAMDR_OK;
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MAMDR_OK;
}

// ---- host helper: tf.data shuffle-buffer order (restated in oracle/rng.py)
int mamdr_shuffle_perm(int64_t n, int64_t buffer_size, uint64_t seed, int32_t* h_out) {
    if (n < 0 || n > 0x7fffffff) return fail(MAMDR_EINVAL, "n out of range");
    if (n == 0) return MAMDR_OK;
    if (!h_out) return fail(MAMDR_EINVAL, "null output");
    if (buffer_size < 1) buffer_size = 1;
    int64_t filled = n < buffer_size ? n : buffer_size;
    std::vector<int32_t> buf((size_t)filled);
    for (int64_t i = 0; i < filled; ++i) buf[(size_t)i] = (int32_t)i;
    int64_t next = filled;
    uint64_t state = seed;
    for (int64_t i = 0; i < n; ++i) {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        const uint64_t j = ((z >> 32) * (uint64_t)filled) >> 32;
        h_out[i] = buf[(size_t)j];
        if (next < n) {
            buf[(size_t)j] = (int32_t)next++;
        } else {
            buf[(size_t)j] = buf[(size_t)filled - 1];
            --filled;
        }
    }
    return MAMDR_OK;
}

int mamdr_shuffle_perms(int32_t n_passes, const int64_t* h_n, int64_t buffer_size, const uint64_t* h_seeds,
                        int32_t* h_out) {
    if (n_passes < 0 || (n_passes > 0 && (!h_n || !h_seeds))) return fail(MAMDR_EINVAL, "bad pass list");
    int64_t off = 0;
    for (int32_t k = 0; k < n_passes; ++k) {
        const int rc = mamdr_shuffle_perm(h_n[k], buffer_size, h_seeds[k], h_out ? h_out + off : nullptr);
        if (rc) return rc;
        off += h_n[k];
    }
    return MAMDR_OK;
}

#ifdef MAMDR_STAMPS
// diagnostic build only (tools/stamp_tower.py)
int mamdr_debug_set_stamps(mamdr_ctx* c, unsigned long long* d_stamps) {
    c->stamps = d_stamps;
    return MAMDR_OK;
}
#endif

// ---- profiling
int64_t mamdr_dropout_steps(const mamdr_ctx* c) { return c ? (int64_t)c->global_step : 0; }

int mamdr_step_path(const mamdr_ctx* c, int32_t batch) { return c && takes_fused_path(c, batch) ? 1 : 0; }
int mamdr_fused_flags(const mamdr_ctx* c) { return c ? c->fused_flags : -1; }

int mamdr_set_tower_tile(mamdr_ctx* c, int32_t rows) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (rows != 0 && rows != 4 && rows != 16) return fail(MAMDR_EINVAL, "tower tile of %d rows (0 = automatic, 4, 16)", rows);
    if (rows == 16 && (c->pnn || c->nfm)) return fail(MAMDR_EINVAL, "the pnn / nfm towers exist as four-row tiles only");
    if (rows != c->tower_tile) {
        c->tower_tile = rows;
        drop_pregathered(c);    // (passes gathered ahead were laid out for the step path of the old choice)
        c->w1t_unread = w1t_unread_now(c);
        c->w2t_unread = w2t_unread_now(c);
        c->wT_valid = false;    // (W1T / W2T may have been left alone under the old choice)
    }
    return MAMDR_OK;
}
int mamdr_tower_tile(const mamdr_ctx* c, int32_t batch) {
    if (!c || batch <= 0) return MAMDR_EINVAL;
    return takes_tower4(c, pad_rows(batch)) ? 4 : 16;
}
int mamdr_profile_enable(mamdr_ctx* c, int32_t enable) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    c->profile = enable != 0;
    return MAMDR_OK;
}
int mamdr_profile_reset(mamdr_ctx* c) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < MAMDR_KERNEL_COUNT; ++k) {
        for (EventPair& p : c->ev[k]) {        // kept for the next profiled run
            if (p.own_a) c->ev_pool_push(p.a);
            c->ev_pool_push(p.b);
        }
        c->ev[k].clear();
    }
    c->prev_b = nullptr;
    c->chain_ok = false;
    return MAMDR_OK;
}
int mamdr_profile_read(mamdr_ctx* c, int32_t kernel, double* total_ms, int64_t* launches) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (kernel < 0 || kernel >= MAMDR_KERNEL_COUNT || !total_ms || !launches) return fail(MAMDR_EINVAL, "bad argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    double sum = 0.0;
    for (EventPair& p : c->ev[kernel]) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        sum += ms;
    }
    *total_ms = sum;
    *launches = (int64_t)c->ev[kernel].size();
    return MAMDR_OK;
}

}  // extern "C"
