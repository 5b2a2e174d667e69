// C ABI of libmamdr_hip.so, the step-kernel context: mamdr_create in named steps (validate_config, read_switches, lay_out,
// alloc_workspace) and mamdr_destroy, the counts and segments of the flat vector, the bindings, the host-side counters, the
// table of environment switches, the tile setters and the profiling slots.
#include <algorithm>
#include <cstdlib>
#include <new>
#include <string>

#include "step_ctx.h"
#include "env_registry.h"

namespace mamdr {
thread_local hipEvent_t g_prof_stop = nullptr;
thread_local ErrBuf g_err;
}

static std::vector<TileDesc> build_tiles(const DenseLayout& L, int n_domain, bool deepfm, int s2_off, bool lin_w0dom, bool star,
                                         bool pnn, bool nfm) {
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

SplitData* split_of(mamdr_ctx* c, int domain, int split) {
    if (domain < 0 || domain >= c->cfg.n_domain || split < 0 || split > 2) return nullptr;
    return &c->data[(size_t)domain * 3 + split];
}

int ready(const mamdr_ctx* c) {
    if (!c->params) return fail(MAMDR_ESTATE, "mamdr_bind_state has not been called");
    if (c->star && !c->aux) return fail(MAMDR_ESTATE, "Star tower: mamdr_bind_aux has not been called");
    if (!c->cfg.emb_trainable && (!c->user_tab || !c->item_tab))
        return fail(MAMDR_ESTATE, "frozen user/item tables are not bound (mamdr_bind_table)");
    return MAMDR_OK;
}

// ---- mamdr_create in steps: validate_config, read_switches, lay_out, alloc_workspace
static int validate_config(const mamdr_config* cfg) {
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
    return MAMDR_OK;
}

// every environment switch of the step engine (env_registry.h), read once, at mamdr_create.  The Star and the
// trainable-table switches keep their condition (the configuration alone decides it); those of the k_wgrad_adam path are
// read in every context, because whether this one takes that path is only decided in lay_out -- every use of their fields
// sits behind c->fused: fused_step itself, P.pre in plan_call, w1t_unread_now in front of w2t_unread_now's other terms,
// takes_fused_path beside use_pre in pregather_applies (which mamdr_pregather_ahead asks before ride_on), and a pending
// domain-table step, which only fused_step leaves, in front of dm_finish_call in mamdr_dr_advance_live
static void read_switches(mamdr_ctx* c) {
    if (const char* tt = getenv("MAMDR_TOWER_TILE")) c->tower_tile = atoi(tt);
    if (const char* nw = getenv("MAMDR_T4_NO_W1L")) c->t4_no_w1l = atoi(nw) != 0;
    if (c->star)
        if (const char* sd = getenv("MAMDR_STAR_DENSE_SLICES")) c->star_dense_slices = atoi(sd) != 0;
    if (c->cfg.emb_trainable) {
        const char* dense_env = getenv("MAMDR_DENSE_ADAM");
        c->lazy = !(dense_env && atoi(dense_env) != 0);
        if (const char* fe = getenv("MAMDR_LAZY_FLUSH_EVERY")) c->flush_every = atoi(fe) > 0 ? atoi(fe) : c->flush_every;
        if (const char* cap_env = getenv("MAMDR_LAZY_LOG_CAP")) {      // tests: force the alpha ring to wrap
            const int cap = atoi(cap_env);
            if (cap >= 4 && (cap & (cap - 1)) == 0) c->log_cap = cap;
        }
    }
    if (const char* fe = getenv("MAMDR_FUSED")) c->fused_mode = atoi(fe);
    if (const char* de = getenv("MAMDR_DM_EACH")) c->dm_finish_each = atoi(de) != 0;
    if (const char* de = getenv("MAMDR_DM_CALL")) c->dm_finish_call = atoi(de) != 0;
    if (const char* de = getenv("MAMDR_NO_W2_DIRECT")) c->w2_direct_ok = atoi(de) == 0;
    if (const char* pe = getenv("MAMDR_NO_PREGATHER")) c->use_pre = atoi(pe) == 0;
    if (const char* pe = getenv("MAMDR_NO_PREGATHER_RIDE")) c->ride_on = atoi(pe) == 0;
    if (const char* se = getenv("MAMDR_FZ_S_INORDER")) c->fz_s_inorder = atoi(se) != 0;
    if (const char* se = getenv("MAMDR_FZ_DEAL_RESIDUE")) c->fz_deal_residue = atoi(se) != 0;
    if (const char* ev = getenv("MAMDR_NO_TAILFUSE")) c->tail_fuse = atoi(ev) == 0;
    if (const char* ev = getenv("MAMDR_REC_CHUNK"))
        if (atoi(ev) > 0) c->rec_chunk = (int)std::min<int64_t>(((int64_t)atoi(ev) + REC_TILE - 1) / REC_TILE * REC_TILE, 1 << 20);
}

// what follows from the configuration and the switches: the flat vector's layout, the gradient slabs and their tiles, and
// which path and which tower a step of how many rows takes.  -> the tile list alloc_workspace uploads
static std::vector<TileDesc> lay_out(mamdr_ctx* c) {
    const mamdr_config* cfg = &c->cfg;
    c->L = DenseLayout::make(cfg->n_domain, c->deepfm, cfg->uncertainty_weight != 0, c->pnn);
    c->table_floats = cfg->emb_trainable ? ((int64_t)cfg->n_user + cfg->n_item) * EMB : 0;
    if (c->deepfm && cfg->emb_trainable) {
        // each 1-d table padded to 4 floats so that the dense block stays 16-B aligned
        c->lin_user_off = c->table_floats;
        c->lin_item_off = c->lin_user_off + (((int64_t)cfg->n_user + 3) & ~(int64_t)3);
        c->table_floats = c->lin_item_off + (((int64_t)cfg->n_item + 3) & ~(int64_t)3);
    }
    c->SL = StarLayout::make(cfg->n_domain);
    c->AL = StarAuxLayout::make(cfg->n_domain);
    c->n_params = c->table_floats + (c->star ? c->SL.alloc : c->L.alloc);
    c->n_meta = c->star ? c->table_floats + c->SL.n_meta : c->n_params;
    c->data.resize((size_t)cfg->n_domain * 3);
    c->rows_pad_max = cfg->max_batch;
    c->slab_ld = c->L.alloc + cfg->n_domain * H1;
    if (c->deepfm || c->pnn) {      // per-row terms of the domain-table gradient: S2 = onehot(domain)^T fmq
        c->s2_off = c->slab_ld;
        c->slab_ld += cfg->n_domain * EMB;
    }
    // dW0[256:384] without tiles: Dm^T . S in k_update, or (Star: one normalised domain row per batch) the
    // rank-1 form in k_star_update
    // (NFM: rows 256..383 of the input tile carry the bi-interaction, not the domain row: plain tiles)
    c->lin_w0dom = (c->star || cfg->n_domain <= 64) && !c->nfm;
    std::vector<TileDesc> tiles = build_tiles(c->L, cfg->n_domain, c->deepfm, c->s2_off, c->lin_w0dom, c->star, c->pnn, c->nfm);
    c->n_tiles = (int)tiles.size();
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
    c->fused = cfg->tower == MAMDR_TOWER_MLP && !cfg->emb_trainable && !cfg->uncertainty_weight && c->lin_w0dom &&
               cfg->n_domain <= 64 && c->fused_mode != 0;
    if (c->fused && c->fused_mode == 2) c->fused_max_batch = 1 << 30;
    c->w1t_unread = w1t_unread_now(c);
    c->w2t_unread = w2t_unread_now(c);
    return tiles;
}

// every allocation goes through the context's record (DevAllocs, host_common.h) -- after the first failure nothing more is
// allocated -- then the memsets, the map initialisations and the two uploads, closed by one synchronise
static int alloc_workspace(mamdr_ctx* c, const std::vector<TileDesc>& tiles) {
    const mamdr_config* cfg = &c->cfg;
    DevAllocs& dev = c->dev;
    const size_t rp = (size_t)c->rows_pad_max;
    float thr[500];
    auc_thresholds(thr);
    dev.alloc(&c->acts, rp * ACT_LD);
    dev.alloc(&c->dz, rp * DZ_LD);
    dev.alloc(&c->dlogit, rp);
    dev.alloc(&c->w0dom_copy, (size_t)EMB * H1);
    dev.alloc(&c->dm_copy, (size_t)cfg->n_domain * EMB);
    if (c->star) {
        const size_t chunks = (rp + STAR_CHUNK - 1) / STAR_CHUNK;
        dev.alloc(&c->eff, (size_t)c->L.alloc);
        dev.alloc(&c->pn, (size_t)PN_WS_FLOATS);
        dev.alloc(&c->star_alpha, (size_t)STAR_ALPHA_CAP);
        dev.alloc(&c->star_part, chunks * 2 * XDIM * (sizeof(double) / sizeof(float)));    // forward: double sums; backward: float sums
        dev.alloc(&c->star_sums, (size_t)(4 * XDIM + EMB));         // sums | domain-row gradient | s1 / B, s2 / B
        dev.alloc(&c->star_dmpart, chunks * EMB);
    }
    if (cfg->emb_trainable || c->star) {
        dev.alloc(&c->dxe, rp * (c->star ? XDIM : 2 * EMB));
        dev.alloc(&c->urow, rp);
        dev.alloc(&c->irow, rp);
    }
    if (cfg->emb_trainable) {
        dev.alloc(&c->map_u, (size_t)cfg->n_user);
        dev.alloc(&c->map_i, (size_t)cfg->n_item);
        dev.alloc(&c->urow_alt, rp);
        dev.alloc(&c->irow_alt, rp);
        dev.alloc(&c->map_u_alt, (size_t)cfg->n_user);
        dev.alloc(&c->map_i_alt, (size_t)cfg->n_item);
        dev.alloc(&c->gbuf_u, rp * EMB);
        dev.alloc(&c->gbuf_i, rp * EMB);
        dev.alloc(&c->hasdup_u, rp);
        dev.alloc(&c->hasdup_i, rp);
        dev.alloc(&c->last_u, (size_t)cfg->n_user);
        dev.alloc(&c->last_i, (size_t)cfg->n_item);
        dev.alloc(&c->alpha_log, (size_t)c->log_cap);
        if (c->deepfm) {
            dev.alloc(&c->glin_u, rp);
            dev.alloc(&c->glin_i, rp);
        }
    }
    if (c->deepfm || c->pnn) dev.alloc(&c->fmq, rp * EMB);
    if (c->pnn) dev.alloc(&c->ipbuf, rp * 4);
    dev.alloc(&c->domrow, rp);
    dev.alloc(&c->loss_part, rp / 4);
    dev.alloc(&c->wT, (size_t)WT_FLOATS);
    if (c->fused) {
        dev.alloc(&c->pdm, (size_t)DM_PARTS * cfg->n_domain * EMB);
        dev.alloc(&c->dmsnap[0], (size_t)3 * cfg->n_domain * EMB);
        dev.alloc(&c->dmsnap[1], (size_t)3 * cfg->n_domain * EMB);
    }
    dev.alloc(&c->slabs, (size_t)WGRAD_MAX_GROUPS * c->slab_ld);
    dev.alloc(&c->tiles, tiles.size());
    dev.alloc(&c->thresholds, (size_t)500);
    dev.alloc(&c->frozen_sumsq, (size_t)4);
    dev.alloc(&c->sumsq_partials, (size_t)1024);
    if (const int rc = dev.check(g_err)) return rc;

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
    if (e != hipSuccess) return fail(MAMDR_EHIP, "workspace initialisation: %s", hipGetErrorString(e));
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

const char* mamdr_last_error(void) { return g_err.text; }
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
    if (const int rc = validate_config(cfg)) return rc;

    mamdr_ctx* c = new (std::nothrow) mamdr_ctx();
    if (!c) return fail(MAMDR_EINVAL, "out of host memory");
    c->cfg = *cfg;
    c->stream = (hipStream_t)stream;
    c->nfm = cfg->tower == MAMDR_TOWER_NFM;
    c->deepfm = cfg->tower == MAMDR_TOWER_DEEPFM || cfg->tower == MAMDR_TOWER_WDL || c->nfm;   // linear tables (+ FM term)
    c->pnn = cfg->tower == MAMDR_TOWER_PNN;
    c->star = cfg->tower == MAMDR_TOWER_STAR;
    read_switches(c);
    const std::vector<TileDesc> tiles = lay_out(c);
    if (const int rc = alloc_workspace(c, tiles)) {
        mamdr_destroy(c);
        return rc;
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
    c->dev.free_all();
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
    if (const int rc = check_state_ptrs(g_err, d_params, d_adam_m, d_adam_v)) return rc;
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
    tf_beta_powers(c->cfg.adam_beta1, c->cfg.adam_beta2, optimizer_steps, &c->b1p, &c->b2p);
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
    if (const int rc = check_bind_table(g_err, c->cfg.emb_trainable != 0, seg, d_rows, n_rows, c->cfg.n_user, c->cfg.n_item)) return rc;
    drop_pregathered(c);        // rows gathered ahead of their calls came from the old table
    const int item = seg == MAMDR_SEG_ITEM_EMB;
    (item ? c->item_tab : c->user_tab) = d_rows;
    launch_sumsq(d_rows, n_rows * EMB, c->sumsq_partials, c->frozen_sumsq + item, c->stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_bind_domain_data(mamdr_ctx* c, int domain, int split, const int32_t* d_uid, const int32_t* d_pid,
                           const int32_t* d_domain, const float* d_label, int64_t n_rows) {
    if (check_ctx(c)) return MAMDR_EINVAL;
    if (const int rc = bind_columns(g_err, split_of(c, domain, split), domain, split, d_uid, d_pid, d_domain, d_label, n_rows))
        return rc;
    drop_pregathered(c);        // (a pass gathered ahead of its call may have come from the old columns)
    const int64_t tiles = (n_rows + TILE_ROWS - 1) / TILE_ROWS;
    if ((size_t)tiles > c->eval_part.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (const int rc = c->eval_part.grow(c->dev, g_err, (size_t)tiles)) return rc;
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
