// Internal header of the step engine's host side: the context (mamdr_ctx), the profiling slots (Prof) and the few helpers
// that cross its five files --
//   step_context.hip    the context: create / destroy, counts, segments, bindings, counters, environment table, profiling
//                       slots, tile setters
//   mamdr_api.hip       the training call: its decisions, CallPlan / plan_call, the three step functions, the pre-gather
//                       entry points, mamdr_train_steps(_n)
//   step_queries.hip    the queries of a context: mamdr_eval_domain, mamdr_gather_rows, mamdr_recommend(_domain),
//                       mamdr_rank_domain, mamdr_rank_slates (the four retrieval calls through retrieval_host.h)
//   eval_metrics.hip    the metrics of an evaluation's predictions, no context: mamdr_group_auc, mamdr_exact_metrics,
//                       mamdr_auc_bootstrap(_bounded), mamdr_isotonic_fit(_bounded), mamdr_isotonic_apply, mamdr_score_sums
//   step_stateless.hip  the outer updates, mamdr_adam_apply, mamdr_pcgrad_project, mamdr_copy, mamdr_gram, the shuffle
// Helpers that one file uses stay static in it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/mamdr_hip.h"
#include "mamdr_kernels.h"
#include "host_common.h"

using namespace mamdr;       // (this header is private to the five host files above, each of which works in that namespace)

// mamdr_last_error's text (step_context.hip).  Like g_prof_stop it keeps default visibility, inside namespace mamdr: a hidden
// extern thread_local is reached through a weak init symbol that is absent for a constant-initialised object
namespace mamdr {
extern thread_local ErrBuf g_err;
}
// nothing else declared here leaves the library: the cross-file helpers and the profiling slots are hidden symbols (the
// exports are the extern "C" functions of include/mamdr_hip.h)
#pragma GCC visibility push(hidden)

template <typename... A>
int fail(int code, const char* fmt, A... a) { return g_err.fail(code, fmt, a...); }
#define HIP_TRY(expr) MAMDR_HIP_TRY(g_err, expr, #expr)

struct EventPair {
    hipEvent_t a, b;
    bool own_a = true;         // false: `a` is the previous kernel's stop event (owned by that pair)
};


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
    int fused_mode = 1;             // MAMDR_FUSED: 0 the slab path everywhere, 2 the k_wgrad_adam path for every batch size
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
    GrowBuf<float> eval_part;       // eval: per tile of a split (grown on bind)
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
    DevAllocs dev;                  // every device allocation of this context, the buffers grown on demand too: what mamdr_destroy frees
    // the retrieval calls' workspace (RecArgs, mamdr_kernels.h): allocated on first use for chunks of up to rec_cap candidates
    int rec_chunk = 16384;          // candidates per pass (MAMDR_REC_CHUNK)
    int rec_cap = 0;
    float* rec_P = nullptr;
    float* rec_lin = nullptr;
    float* rec_q = nullptr;         // q0 | qud | qs
    unsigned long long* rec_part = nullptr;
    unsigned long long* rec_best = nullptr;
    GrowBuf<unsigned long long> rec_tkey;        // mamdr_rank_domain / mamdr_rank_slates: the call's target / entry keys
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

inline int check_ctx(const mamdr_ctx* c) {
    if (!c) return fail(MAMDR_EINVAL, "null context");
    return MAMDR_OK;
}

// per-kernel device time from stop events chained along the stream (see mamdr_ctx::prev_b)
struct Prof {
    mamdr_ctx* c;
    int k;
    EventPair e{nullptr, nullptr, true};
    Prof(mamdr_ctx* c_, int k_, bool on = true) : c(c_), k(k_) {     // on = false: a scope that times nothing
        if (!on || !c->profile || c->ev[k].size() >= 200000) return;
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
inline void prof_break(mamdr_ctx* c) { c->chain_ok = false; }

constexpr int STAR_ALPHA_CAP = 1 << 12;      // steps between two replays of the lagging Star slices (power of two)
constexpr int WGRAD_MAX_GROUPS = 16;         // row groups of k_wgrad at most (= gradient slabs k_update sums)

// ---- step_context.hip
SplitData* split_of(mamdr_ctx* c, int domain, int split);
int ready(const mamdr_ctx* c);
// ---- mamdr_api.hip: the decisions of a training call (mamdr_step_path / mamdr_tower_tile / mamdr_create ask them too) ...
int64_t pad_rows(int64_t rows);
bool takes_fused_path(const mamdr_ctx* c, int64_t batch);
bool takes_tower4(const mamdr_ctx* c, int64_t rows_pad);
bool w1t_unread_now(const mamdr_ctx* c);
bool w2t_unread_now(const mamdr_ctx* c);
// ... and what every reader of the live state starts with
void fill_tower_common(const mamdr_ctx* c, const SplitData& d, TowerArgs& a);
void fill_star_prep(const mamdr_ctx* c, int domain, StarPrepArgs& pa);
void refresh_table_sumsq(mamdr_ctx* c);
void finish_dm(mamdr_ctx* c);
void sync_tables(mamdr_ctx* c);
void drop_pregathered(mamdr_ctx* c);

#pragma GCC visibility pop
