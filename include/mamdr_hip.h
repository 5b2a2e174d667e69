/*
 * mamdr_hip.h -- C ABI of libmamdr_hip.so: the MI355X (gfx950) hot path of MAMDR.
 *
 * The reference (RManLuo/MAMDR) has no FFI; its de-facto boundary is the handful
 * of Keras/TF calls through which the meta-learning wrappers touch numerics
 * (SURVEY.md section 8b).  Each entry point below names the reference interface
 * it replaces (file:line under /root/reference).  The reference-side binding a
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no torch/HIP types in signatures; `stream` is a hipStream_t passed
 *    as void* (NULL = the null stream).
 *  - every pointer named d_* is a DEVICE pointer owned by the caller and must
 *    stay valid while bound; the library allocates only its private workspace.
 *  - return 0 on success, negative MAMDR_E* on failure; mamdr_last_error() gives
 *    the text (thread-local).  No internal threads; a context is not re-entrant.
 *  - all launches are asynchronous on the context's stream; nothing here
 *    synchronises the device except mamdr_profile_read().
 */
#ifndef MAMDR_HIP_H
#define MAMDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAMDR_ABI_VERSION 19

enum {
    MAMDR_OK = 0,
    MAMDR_EINVAL = -1,      /* bad argument / unsupported configuration */
    MAMDR_ESTATE = -2,      /* call out of order (state/tables/data not bound) */
    MAMDR_EHIP = -3,        /* a HIP runtime call failed */
    MAMDR_ENOTBUILT = -4    /* feature named by the reference but not built in this round */
};

/* tower kinds: run.py:37-47 + model_zoo/DeepCTR/deepctr.py:24-50 name registry */
enum { MAMDR_TOWER_MLP = 0, MAMDR_TOWER_DEEPFM = 1, MAMDR_TOWER_STAR = 2,
       /* deepctr WDL (deepctr.py:29-32): linear tables + DNN = DeepFM without the FM term; same segments */
       MAMDR_TOWER_WDL = 3,
       /* deepctr PNN (deepctr.py:44-46; use_inner, no outer product): the mlp tower on [user | item | domain | <u,i> <u,d>
          <i,d>] -- the three inner products feed three more rows of the first kernel (segment MAMDR_SEG_W0X).  Steps of
          up to 2,048 rows (every reference config has batch_size 1,024); larger batches: the generic-layer engine */
       MAMDR_TOWER_PNN = 4,
       /* deepctr NFM (deepctr.py:33-35): linear tables (as WDL) + DNN over the 128 bi-interaction columns u i + (u + i) d.
          Same segments as WDL, but segment W0 is deepctr's [128, 256] kernel: it occupies rows 256..383 of the mlp
          tower's W0 (the bi-interaction takes the domain field's place in the input tile; rows 0..255 stay zero and
          belong to no segment).  Steps of up to 2,048 rows, as PNN */
       MAMDR_TOWER_NFM = 5 };
/* data splits: utils/dataset.py:79-92 */
enum { MAMDR_SPLIT_TRAIN = 0, MAMDR_SPLIT_VAL = 1, MAMDR_SPLIT_TEST = 2 };
/* optimisers: deepctr.py:55 (Adam) / specific_base_model.py:120, base_model.py:69 (SGD finetune) */
enum { MAMDR_OPT_ADAM = 0, MAMDR_OPT_SGD = 1,
       /* no update: add d total_loss / d theta of the batch (dropout off) to the bound accumulator --
          the meta pass of first-order MAML, model_zoo/maml.py:107-109,196-229 */
       MAMDR_OPT_ACCUMULATE = 2 };
/* merged_method: model_zoo/specific_base_model.py:164-172 */
enum { MAMDR_MERGE_PLUS = 0, MAMDR_MERGE_TIMES = 1 };
/* segments of the flat trainable vector, in Keras trainable_weights order */
enum {
    MAMDR_SEG_USER_EMB = 0, MAMDR_SEG_ITEM_EMB = 1, MAMDR_SEG_DOMAIN_EMB = 2,
    MAMDR_SEG_W0 = 3, MAMDR_SEG_W1 = 4, MAMDR_SEG_W2 = 5,
    MAMDR_SEG_B0 = 6, MAMDR_SEG_B1 = 7, MAMDR_SEG_B2 = 8,
    MAMDR_SEG_WO = 9, MAMDR_SEG_GB = 10,
    /* DeepFM 1-d linear tables (deepctr get_linear_logit): the user / item ones are in the
       vector only when emb_trainable (they inherit the feature column's `trainable`), behind the
       embedding tables; the domain one follows the global bias */
    MAMDR_SEG_LIN_USER = 11, MAMDR_SEG_LIN_ITEM = 12, MAMDR_SEG_LIN_DOMAIN = 13,
    /* Star tower (model_zoo/Star/star_fcn.py:61-103, partitioned_norm.py:56-100): shared kernels / biases
       (meta parameters), then PartitionedNorm gamma / beta (shared [384], specific [D][384]), specific
       kernels [D][in][out] and biases [D][out].  W0..B2 report count 0 for this tower. */
    MAMDR_SEG_STAR_WS0 = 14, MAMDR_SEG_STAR_WS1 = 15, MAMDR_SEG_STAR_WS2 = 16,
    MAMDR_SEG_STAR_BS0 = 17, MAMDR_SEG_STAR_BS1 = 18, MAMDR_SEG_STAR_BS2 = 19,
    MAMDR_SEG_PN_GAMMA_SHARED = 20, MAMDR_SEG_PN_BETA_SHARED = 21,
    MAMDR_SEG_PN_GAMMA_SPEC = 22, MAMDR_SEG_PN_BETA_SPEC = 23,
    MAMDR_SEG_STAR_WD0 = 24, MAMDR_SEG_STAR_WD1 = 25, MAMDR_SEG_STAR_WD2 = 26,
    MAMDR_SEG_STAR_BD0 = 27, MAMDR_SEG_STAR_BD1 = 28, MAMDR_SEG_STAR_BD2 = 29,
    /* uncertainty weighting: `log_var` [D] (model_zoo/uncertainty_weight/weighted_loss.py:23-28), last segment */
    MAMDR_SEG_LOG_VAR = 30,
    /* PNN: rows 384..386 of deepctr's first DNN kernel [387, 256] (the inner products' rows), behind everything else */
    MAMDR_SEG_W0X = 31,
    MAMDR_SEG_COUNT = 32
};
/* kernels whose device time can be profiled (mamdr_profile_*) */
enum { MAMDR_KERNEL_FWD_BWD = 0, MAMDR_KERNEL_WGRAD = 1, MAMDR_KERNEL_UPDATE = 2,
       MAMDR_KERNEL_EVAL = 3, MAMDR_KERNEL_GATHER = 4, MAMDR_KERNEL_EMB_SWEEP = 5,
       /* every other launch of a training call, so that the slots add up to the whole step: k_pass_prep, k_emb_rows,
          k_emb_catchup, k_lin_sweep, k_star_catchup, and as ONE timed group each [k_star_stats + k_star_prep] and
          PartitionedNorm's backward [k_star_pnb_partial + _final + _apply (+ k_star_dm_final)] */
       MAMDR_KERNEL_AUX = 6,
       /* k_emb_flush: the lazy table Adam's replay of every lagging row (forced every 32 Adam steps) */
       MAMDR_KERNEL_FLUSH = 7, MAMDR_KERNEL_COUNT = 8 };

typedef struct mamdr_ctx mamdr_ctx;

/* Model / step configuration.  Replaces the `model` + `train` sections consumed by
 * DeepCTR.__init__/build_model (model_zoo/base_model.py:14-33,
 * model_zoo/DeepCTR/deepctr.py:20-61,95-136). */
typedef struct mamdr_config {
    int32_t abi_version;     /* MAMDR_ABI_VERSION */
    int32_t tower;           /* MAMDR_TOWER_* */
    int32_t n_user;          /* dataset.n_uid, utils/dataset.py:50-52 */
    int32_t n_item;          /* dataset.n_pid, utils/dataset.py:53-55 */
    int32_t n_domain;        /* utils/dataset.py:63-65 */
    int32_t emb_dim;         /* model.user_dim == item_dim == domain_dim (128) */
    int32_t hidden[3];       /* model.hidden_dim (256,128,64) */
    int32_t max_batch;       /* dataset.batch_size */
    int32_t emb_trainable;   /* train.emb_trainable: user/item tables join the trainable vector */
    float dropout;           /* model.dropout (rate) */
    float l2_emb;            /* deepctr.py:118 l2_reg_embedding = 1e-5 */
    float l2_linear;         /* DeepFM l2_reg_linear (deepctr default 1e-5); ignored by the mlp tower */
    float adam_beta1, adam_beta2, adam_eps; /* tf.train.AdamOptimizer defaults 0.9/0.999/1e-8 */
    int32_t uncertainty_weight; /* 1: training loss = mean(BCE) / var_d^2 + log var_d + regularisers with one trainable
                                   var per domain (model_zoo/uncertainty_weight/weighted_loss.py:30-43); evaluation is
                                   unweighted, as the reference evaluates the base model.  Every tower of mamdr_create but Star */
} mamdr_config;

const char* mamdr_last_error(void);
int mamdr_abi_version(void);
/* Every environment switch this build reads (library, Python host, bench.py, tools, tests), one per line:
 * "NAME\twho reads it\teffect\n"; a trailing '*' marks a name prefix.  Diagnostics only -- the reference is configured by
 * its JSON files alone (run.py:20-33) and the defaults are what the parity tests and bench.py run.  mamdr_create /
 * mamdr_graph_create report (stderr, once per process) any MAMDR_* name of the environment that is NOT in this table;
 * mamdr_env_unknown returns how many there were.  (ABI 18) */
const char* mamdr_env_switches(void);
int mamdr_env_unknown(void);

/* --- lifetime: replaces DeepCTR(dataset, config) / build_model + compile
 *     (model_zoo/DeepCTR/deepctr.py:20-61). */
int mamdr_create(const mamdr_config* cfg, void* stream, mamdr_ctx** out);
int mamdr_destroy(mamdr_ctx* ctx);

/* --- flat trainable vector ("meta parameters"): replaces
 *     MAML._get_model_meta_parms with meta_parms ["all"] (model_zoo/maml.py:153-179).
 *     mamdr_param_count = number of floats of the flat vector INCLUDING alignment
 *     padding (padding elements stay 0).  Layout per segment via mamdr_param_segment;
 *     a segment absent from the vector (frozen tables) reports count 0. */
int64_t mamdr_param_count(const mamdr_ctx* ctx);
/* Length of the META prefix of the flat vector: the tensors `MAML._get_model_meta_parms` selects
 * (model_zoo/maml.py:153-179).  Equals mamdr_param_count for the mlp / deepfm towers (meta_parms ["all"]);
 * for the Star tower it covers the tables, shared kernels and shared biases
 * (config/Taobao-10/star_taobao.json:37-41) -- theta / phi / merged vectors have this length and the
 * outer updates and weight assignment act on this prefix only. */
int64_t mamdr_meta_count(const mamdr_ctx* ctx);
/* Non-trainable model state (Star: PartitionedNorm moving mean / variance per domain and the
 * zero-debias slots of their moving averages, partitioned_norm.py:71-87,177-193): number of floats
 * (0 for the other towers) and binding of a caller-owned device buffer, initialised by the caller
 * (layout: mov_mean [D][384] = 0 | mov_var [D][384] = 1 | biased_mean = 0 | biased_var = 0 | steps [D] = 0). */
int64_t mamdr_aux_count(const mamdr_ctx* ctx);
int mamdr_bind_aux(mamdr_ctx* ctx, float* d_aux);
int mamdr_param_segment(const mamdr_ctx* ctx, int seg, int64_t* offset, int64_t* count);

/* Bind the live model state (caller-owned device memory, mamdr_param_count floats
 * each): weights, Adam m, Adam v.  Replaces the TF variables + optimizer slots
 * created at deepctr.py:55-60.  Adam slots are NOT reset by weight assignment
 * (SURVEY A.5); mamdr_optimizer_reset zeroes m, v and the step count. */
int mamdr_bind_state(mamdr_ctx* ctx, float* d_params, float* d_adam_m, float* d_adam_v);
int mamdr_optimizer_reset(mamdr_ctx* ctx);
/* Bind the meta-gradient accumulator (mamdr_param_count floats, caller-owned, caller zeroes it):
 * target of MAMDR_OPT_ACCUMULATE steps.  Replaces `self.accum_grads` (model_zoo/maml.py:202). */
int mamdr_bind_accumulator(mamdr_ctx* ctx, float* d_acc);
int64_t mamdr_optimizer_steps(const mamdr_ctx* ctx);
/* Restore the run's two host-side counters -- the Adam step count with its running beta powers (TF's `beta1_power` /
 * `beta2_power` slot variables, restored by tf.train.Saver with the optimizer: deepctr.py:55-60 creates them) and the
 * position of the dropout stream (mamdr_dropout_steps) -- e.g. when a run resumes from saved weights and slots written into
 * the bound vectors.  The live state is synchronised first (as mamdr_sync_tables); afterwards every table row counts as
 * current AT `optimizer_steps`.  The parity tests use it to start a pass from the oracle's state at that point
 * (tests/test_gpu_teacher.py).  (ABI 18) */
int mamdr_set_counters(mamdr_ctx* ctx, int64_t optimizer_steps, int64_t dropout_steps);
/* Trainable tables only (no-op otherwise).  tf.train.AdamOptimizer moves every table row every step
 * (deepctr.py:54-60 with l2_reg_embedding: regulariser gradient + decaying moments).  The library replays
 * those per-row steps lazily -- bit-identical to the per-step dense update -- so between two calls of
 * mamdr_train_steps rows that no batch touched may lag.  Call this before READING the bound weights /
 * Adam slots from outside the library or REPLACING them (K.batch_get_value / SetVarOp, maml.py:181-194;
 * mamdr_copy / mamdr_interp / ... on the bound vectors).  mamdr_eval_domain, mamdr_gather_rows,
 * mamdr_optimizer_reset, mamdr_bind_state and SGD / accumulate steps synchronise by themselves.
 * A non-null d_loss_out makes every step synchronise first (its regulariser term sums over all rows).
 * MAMDR_DENSE_ADAM=1 in the environment keeps the per-step dense sweep instead. */
int mamdr_sync_tables(mamdr_ctx* ctx);
/* Launches of the lazy table Adam's replay kernel (k_emb_flush) so far: all of them, or (forced_only != 0) only those
 * the flush period forced inside a training call.  Lets a parity test state how many flushes a run spanned
 * (tests/test_gpu_fullsize.py); no reference counterpart -- TF1's dense Adam has no such event. */
int64_t mamdr_table_flushes(const mamdr_ctx* ctx, int32_t forced_only);

/* Bind the frozen user / item tables (row-major [rows, emb_dim] fp32).  Replaces
 * DeepCTR.build_emb with a Constant initializer, trainable=False
 * (deepctr.py:104-116).  seg = MAMDR_SEG_USER_EMB or MAMDR_SEG_ITEM_EMB.  With
 * emb_trainable the tables live inside the flat vector and this is an error. */
int mamdr_bind_table(mamdr_ctx* ctx, int seg, const float* d_rows, int64_t n_rows);

/* Bind one domain's split: int32 uid/pid/domain columns and fp32 label column of
 * n rows, in file order.  Replaces get_dataset / make_csv_dataset + expand_dim
 * (utils/dataset.py:12-38,79-92): columns uid,pid,domain,label. */
int mamdr_bind_domain_data(mamdr_ctx* ctx, int domain, int split, const int32_t* d_uid,
                           const int32_t* d_pid, const int32_t* d_domain, const float* d_label,
                           int64_t n_rows);

/* Run n_steps consecutive inner optimisation steps ("domain-steps") on one
 * domain's TRAIN split, entirely device-side.  Replaces the loops
 *   for step in range(train_step): model.train_on_batch(train_iter)
 * (model_zoo/mamdr.py:85-86,96-97, domain_negotiation.py:71-72, reptile.py:69-70)
 * and model.fit(iter, steps_per_epoch=n) (mamdr.py:54, deepctr.py:76).
 *   d_perm     row order of this pass (the shuffled iterator, utils/dataset.py:27-37),
 *              n_rows int32, or NULL for file order
 *   first_step first batch index within the pass; batch s covers
 *              perm[s*batch .. min(n_rows,(s+1)*batch))  (final partial batch kept,
 *              utils/dataset.py:25)
 *   dropout_seed seed of the counter-based dropout stream (step index = the
 *              context's global inner-step counter)
 *   d_loss_out optional device array of n_steps floats: total loss per step
 *              (BCE mean + regularisers), what train_on_batch returns as `loss`. */
int mamdr_train_steps(mamdr_ctx* ctx, int domain, const int32_t* d_perm, int64_t first_step,
                      int64_t n_steps, int32_t batch, uint32_t dropout_seed, int32_t optimizer,
                      float lr, float* d_loss_out);
/* Same, over a pass of `pass_rows` positions only (d_perm then holds pass_rows row indices of the split;
 * -1 = the whole split).  Replaces the take/skip sub-datasets of the meta-train / meta-val split
 * (model_zoo/maml.py:300-330, mldg.py:309-325: `dataset.take(n_train)` / `dataset.skip(n_train)`), whose
 * final partial batch ends at the sub-dataset's end. */
int mamdr_train_steps_n(mamdr_ctx* ctx, int domain, const int32_t* d_perm, int64_t pass_rows, int64_t first_step,
                        int64_t n_steps, int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr,
                        float* d_loss_out);

/* Evaluate one domain's split with the live weights, dropout off.  Replaces
 * model.evaluate(data, steps=n_step) (model_zoo/base_model.py:131,
 * specific_base_model.py:84).
 *   d_loss_out  1 float: mean over batches of the batch-mean loss (+ regularisers)
 *   d_hist      2*501 uint32 (zeroed by this call): d_hist[c*501 + k] = number of
 *               rows with (label != 0) == c whose prediction exceeds exactly k of
 *               the 500 AUC thresholds (utils/auc.py:118-126).  The confusion
 *               counts of utils/metrics_utils.py:297-354 are suffix sums of it.
 *   d_pred_out  optional n_rows floats: predictions in file order. */
int mamdr_eval_domain(mamdr_ctx* ctx, int domain, int split, int32_t batch, float* d_loss_out,
                      uint32_t* d_hist, float* d_pred_out);

/* Standalone embedding gather (K1 of SURVEY 2.2): out[r] = [U[uid]|I[pid]|Dm[dom]]
 * for n rows of a bound split in d_perm order.  Same code path the step kernel
 * uses for its tiles; exported for parity tests and bandwidth measurement. */
int mamdr_gather_rows(mamdr_ctx* ctx, int domain, int split, const int32_t* d_perm,
                      int64_t first_row, int64_t n_rows, float* d_out);

/* Top-K item recommendation from the live weights of an mlp / wdl / deepfm tower.  NO REFERENCE COUNTERPART: the
 * reference's pipeline ends at per-domain loss and AUC (base_model.py:111-144); this scores (query, candidate) pairs
 * with the same tower in inference mode (dropout off, no regularisers) and ranks them on the device.
 *   n_query, d_uid, d_domain   the queries: user and domain of each
 *   d_cand, n_cand             candidate item ids, DISTINCT (not checked) and inside [0, n_item) (ids outside are clamped:
 *                              range-check on the host); NULL: every item 0 .. n_item - 1, n_cand ignored
 *   d_excl_off, d_excl_ids     optional CSR, both or neither: query q never gets the ids d_excl_ids[d_excl_off[q] ..
 *                              d_excl_off[q + 1]), which are ascending
 *   k                          1 .. 128
 *   d_ids_out, d_scores_out    [n_query][k]: the k best candidates by logit, descending; equal logits by ascending item
 *                              id (the id, not the position in d_cand); a NaN logit ranks behind every number; the score
 *                              is sigmoid(logit) as mamdr_eval_domain's d_pred_out computes it.  A query with fewer than
 *                              k candidates left ends in id -1 / score 0
 *   d_scores_all               optional [n_query][n_cand]: sigmoid(logit) of every pair in d_cand order, 0 for an
 *                              excluded pair
 * The first layer separates by field -- z0 = (u.W0[0:128] + d.W0[256:384] + b0) + i.W0[128:256] -- so the query term is
 * formed once per query, the item term once per candidate and call, and layers 1 and 2 + the head per pair: 82,048 flop
 * per pair against the full tower's 360,576.  A pair's logit is the same bits wherever it sits in the call: full or
 * remainder tile, any chunking (MAMDR_REC_CHUNK), any neighbouring queries.
 * Reads the state only: weights, Adam slots, step and dropout counters and gathered pass windows are unchanged; lagging
 * table rows and a pending domain-table step are brought up to date first (as mamdr_sync_tables).  The workspace is the
 * context's, allocated on first use.
 * MAMDR_EINVAL: null / unaligned required pointer, k outside 1..128, n_query <= 0, n_cand <= 0 with a list given;
 * MAMDR_ESTATE: state or frozen tables not bound; MAMDR_ENOTBUILT: the pnn / nfm towers (their first layer does not
 * separate this way) and the star tower, whose first layer separates for one domain at a time only: its item term depends
 * on the domain, so a call that mixes domains stays refused and the single-domain call declared next serves it.  (Added
 * within ABI 19: a new entry point only, no structure or existing call changed.) */
int mamdr_recommend(mamdr_ctx* ctx, int32_t n_query, const int32_t* d_uid, const int32_t* d_domain,
                    const int32_t* d_cand, int64_t n_cand,
                    const int64_t* d_excl_off, const int32_t* d_excl_ids,
                    int32_t k, int32_t* d_ids_out, float* d_scores_out,
                    float* d_scores_all);

/* Top-K item recommendation with every query of the call in ONE domain, from the live weights of an mlp / wdl / deepfm /
 * star tower.  NO REFERENCE COUNTERPART, as mamdr_recommend.  `domain` is a host integer; every other argument, the
 * ranking keys, the tie and NaN rules, the -1 / 0 padding, d_scores_all, the chunking (MAMDR_REC_CHUNK) and the "same bits
 * wherever the pair sits" guarantee are mamdr_recommend's; on mlp / wdl / deepfm the outputs are the bytes of
 * mamdr_recommend with d_domain[q] = domain for every q.
 * Star: in inference PartitionedNorm with domain d's moving statistics is a per-column affine xn = x * scale_d + shift_d
 * and layer 0 a plain matmul with K0_d = Ws0 * Wd0[d], b0_d = bs0 + bd0[d] (partitioned_norm.py:143-165,
 * star_fcn.py:105-110), so z0 = (xn_u.K0_d[0:128] + xn_dm.K0_d[256:384] + b0_d) + xn_i.K0_d[128:256]: the same query term /
 * item term / per-pair split, on the effective dense block and PartitionedNorm workspace that mamdr_eval_domain builds for
 * the domain.  The scores are mamdr_eval_domain's d_pred_out of the same (user, item, domain) triples up to fp32
 * summation order.
 * Reads the state only, as mamdr_recommend (lazily replayed per-domain slices are brought up to date first); the effective
 * block and the PartitionedNorm workspace it overwrites are rebuilt by every training and evaluation call before use.
 * MAMDR_EINVAL: domain outside [0, n_domain), and mamdr_recommend's cases; MAMDR_ESTATE: as mamdr_recommend;
 * MAMDR_ENOTBUILT: the pnn / nfm towers.  (Added within ABI 19: a new entry point only, no structure or existing call
 * changed.) */
int mamdr_recommend_domain(mamdr_ctx* ctx, int32_t domain, int32_t n_query, const int32_t* d_uid,
                           const int32_t* d_cand, int64_t n_cand,
                           const int64_t* d_excl_off, const int32_t* d_excl_ids,
                           int32_t k, int32_t* d_ids_out, float* d_scores_out, float* d_scores_all);

/* Exact ranks of target items among a candidate list, every query of the call in ONE domain, from the live weights of an
 * mlp / wdl / deepfm / star tower.  NO REFERENCE COUNTERPART, as mamdr_recommend.  Where mamdr_recommend_domain returns the
 * first k <= 128 positions of a query's ordering, this call returns, for chosen (query, target) pairs, the position
 * itself -- one integer per pair, from which MRR, mean percentile rank and HitRate / Recall / NDCG at any K follow.
 *   domain, n_query, d_uid, d_cand, n_cand, d_excl_off, d_excl_ids
 *                              mamdr_recommend_domain's, with the same checks and errors
 *   d_tgt_off [n_query + 1], d_tgt_ids
 *                              CSR of target items per query: offsets ascending from 0 (checked: the call reads them back,
 *                              its one synchronisation of the context's stream); the ids of a query ascending and
 *                              distinct, inside [0, n_item) (ids outside are clamped: range-check on the host).  A query
 *                              may have no targets; so may the whole call, which then produces d_live_out only
 *   d_rank_out [n targets]     int32, see Rank
 *   d_score_out                optional [n targets], see Score
 *   d_live_out [n_query]       int32, see Live
 * key(q, x) is the 64-bit ranking key of the top-K calls: (order-preserving bits of the logit << 32) | ~id, so a larger
 * key is a higher logit or an equal logit and a smaller item id; -0 counts as +0; a NaN logit is behind every number.
 * A candidate c is live for q when it is not in q's exclusion list.
 * Rank.  d_rank_out[j], for target j = (q, t), is #{ c in candidates, live for q : key(q, c) > key(q, t) }: the number
 *   of live candidates that order strictly before the pair.  It is defined for any target id, whether or not t is among
 *   the candidates or excluded for q: the caller decides what an unlisted target means.  The target never counts itself:
 *   equal ids give equal keys, the target's key being the bits the candidate pass computes for the same pair.
 * Score.  d_score_out[j] = sigmoid(logit(q, t)), the bits d_scores_all of mamdr_recommend_domain holds for that pair.
 * Live.  d_live_out[q] is the number of live candidates of q.  A NaN-scored candidate is live.
 * Link to top-K.  For t among the candidates and live, and k <= 128: t is at position r of mamdr_recommend_domain's list
 *   exactly when its rank is r < k.
 * Two phases per block of 256 queries: the target keys (the targets' item term, then 64 consecutive targets per
 * workgroup through the layers and the head of the scoring tile), then the scoring tiles of the top-K calls with a
 * counting ending instead of the sort -- popcount(ballot(key > target key)) per (tile, target), added with an integer
 * atomic.  No merge pass.
 * Determinism: all counts are integers and there is no floating-point atomic: the outputs are the same bits from run to
 * run and under any MAMDR_REC_CHUNK.
 * Reads the state only, as mamdr_recommend_domain: tables and lazily replayed slices are brought up to date first, the star
 * tower's effective block and PartitionedNorm workspace are built for `domain` in inference mode; weights, Adam slots,
 * counters and gathered windows are untouched.  The call zeroes d_rank_out and d_live_out itself, on the context's stream;
 * the target keys live in a workspace of the context, grown on demand.
 * MAMDR_EINVAL: mamdr_recommend_domain's cases; a null d_tgt_off, d_rank_out or d_live_out; d_tgt_ids null while targets
 * exist; offsets that do not start at 0 or descend; a misaligned pointer.  MAMDR_ESTATE: as mamdr_recommend;
 * MAMDR_ENOTBUILT: the pnn / nfm towers.  (Added within ABI 19: a new entry point only, no structure or existing call
 * changed.) */
int mamdr_rank_domain(mamdr_ctx* ctx, int32_t domain, int32_t n_query, const int32_t* d_uid,
                      const int32_t* d_cand, int64_t n_cand,
                      const int64_t* d_excl_off, const int32_t* d_excl_ids,
                      const int64_t* d_tgt_off, const int32_t* d_tgt_ids,
                      int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out);

/* Per-query candidate slates scored and ordered, every query of the call in ONE domain, from the live weights of an mlp /
 * wdl / deepfm / star tower.  NO REFERENCE COUNTERPART, as mamdr_recommend.  The three calls above share one candidate list
 * among all queries of a call; here every query brings its own list -- the ranking stage behind a retrieval stage, and the
 * sampled-negatives evaluation protocol (each held-out positive among N sampled items) -- and the work is one pair per
 * entry, sum of the slates' lengths, not n_query x |union of the slates|.
 *   domain, n_query, d_uid     mamdr_rank_domain's
 *   d_slate_off [n_query + 1]  int64 offsets ascending from 0 (checked: the call reads them back, its one synchronisation of
 *                              the context's stream)
 *   d_slate_ids [n entries]    the item ids of slate q at [d_slate_off[q], d_slate_off[q + 1]), in any order, DISTINCT within
 *                              a slate (not checked) and inside [0, n_item) (ids outside are clamped: range-check on the
 *                              host).  A slate may be empty; so may the whole call, which then returns MAMDR_OK and writes
 *                              nothing
 *   d_pos_out [n entries]      int32, see Position
 *   d_score_out                optional [n entries], see Score
 *   d_order_out                optional [n entries] int32, see Order
 * key(q, x) is the 64-bit ranking key of the family: (order-preserving bits of the logit << 32) | ~id, so a larger key is
 * a higher logit or an equal logit and a smaller item id; -0 counts as +0; a NaN logit is behind every number.
 * Position.  d_pos_out[j], for entry j of slate q, is the number of entries of the same slate whose key is strictly
 *   greater.  With distinct ids the positions of a slate of L entries are a permutation of 0 .. L - 1.
 * Score.  d_score_out[j] = sigmoid(logit) of the pair: the bits mamdr_rank_domain's d_score_out and
 *   mamdr_recommend_domain's d_scores_all hold for that (user, item, domain).
 * Order.  d_order_out[d_slate_off[q] + d_pos_out[j]] = j - d_slate_off[q]: the slate-local index of the entry at each
 *   position.  The call fills the array with -1 first; with distinct ids no -1 remains.  Duplicate ids share a position:
 *   which of them claims the slot is unspecified, and the slots nobody claims keep -1.
 * Per block of 256 queries: the query terms, then -- a workspace's worth of entries at a time -- mamdr_rank_domain's target
 * pre-pass over the block's entries (the entries' item term, then 64 consecutive entries per workgroup through the layers
 * and the head of the scoring tile: the keys are the bits the grid computes for the same pair), then k_slate_order: one
 * wave per slate of up to 64 entries, one workgroup per 256 entries of a longer slate with the slate's keys staged through
 * LDS 1,024 at a time; every entry counts the keys of its slate above its own.  That is O(L^2) integer compares per
 * slate, ON PURPOSE: slates are short (tens to a few thousand entries); ordering a whole catalogue stays
 * mamdr_rank_domain's job.  An item that sits in several slates has its item term formed once per slate.  The grid of the
 * longer slates' launch is ceil(longest slate of the block / 256) x the block's queries, and workgroups without entries leave
 * at once: a block whose slates are of very unequal lengths launches many that do no work.
 * Determinism: the ordering uses integers only and no atomics, every output word is written by one thread; the bits do not
 * depend on MAMDR_REC_CHUNK, on neighbouring queries, or on the order of the entries inside a slate.
 * Reads the state only, as mamdr_rank_domain: tables and lazily replayed slices are brought up to date first, the star
 * tower's effective block and PartitionedNorm workspace are built for `domain` in inference mode; weights, Adam slots,
 * counters and gathered windows are untouched.  The keys live in a workspace of the context, grown on demand.
 * Under mamdr_profile_enable the call's phases land in three slots: the entries' item term in MAMDR_KERNEL_GATHER, the pair
 * tiles in MAMDR_KERNEL_EVAL and k_slate_order in MAMDR_KERNEL_AUX (the query terms are not timed).
 * MAMDR_EINVAL: a null d_uid, d_slate_off or d_pos_out; d_slate_ids null while entries exist; a misaligned pointer; domain
 * outside [0, n_domain); n_query <= 0; offsets that do not start at 0 or descend, or a slate of more than 2^31 - 1 entries.
 * MAMDR_ESTATE: as mamdr_recommend; MAMDR_ENOTBUILT: the pnn / nfm towers.  (Added within ABI 19: a new entry point only,
 * no structure or existing call changed.) */
int mamdr_rank_slates(mamdr_ctx* ctx, int32_t domain, int32_t n_query, const int32_t* d_uid,
                      const int64_t* d_slate_off, const int32_t* d_slate_ids,
                      float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out);

/* Per-user grouped AUC (GAUC, Zhou et al., DIN, KDD 2018) of one split's predictions.  NO REFERENCE COUNTERPART: the
 * reference reports one 500-threshold AUC per domain (base_model.py:111-144) and nothing per user.  Stateless, any stream.
 * Definition.  For one split of one domain, group the rows by uid.  For a group u with r_u rows, P_u of them positive
 * (label != 0, as the eval histogram classifies) and N_u negative:
 *   T_u = 2 * #{(p, n): s_p > s_n} + #{(p, n): s_p == s_n} over positive rows p and negative rows n of the group.  It is
 *   an integer.  AUC_u = T_u / (2 * P_u * N_u), the Mann-Whitney statistic with ties counted half.
 *   Predictions compare as IEEE floats, with three rules.  -0 equals +0.  A NaN is below every number, -inf included.
 *   Two NaNs are equal.
 *   A group is valid when P_u > 0 and N_u > 0.
 *   GAUC = sum_valid r_u * AUC_u / sum_valid r_u.
 *   Report beside it n_groups, n_valid and rows_valid = sum_valid r_u.
 *   When no group is valid, GAUC is reported as 0.0 with n_valid = 0.  This is the convention of
 *   recommend.ranking_metrics.
 * Arguments (device pointers; mamdr_amd/gauc.py: group_plan builds the grouping on the host):
 *   d_pred, d_label [n]        predictions and labels in file order
 *   d_order [n]                row indices grouped by uid (an index outside [0, n) is clamped: check on the host)
 *   d_group_off [n_groups + 1] positions into d_order, ascending from 0 to n; n_groups <= n
 *   d_tile_group, d_tile_first [n_tiles], both or neither: EVERY group of more than 64 rows is covered exactly once by
 *                              tiles (group, first position into d_order) of up to 256 consecutive positions (not
 *                              checked: a larger group without tiles reports T_u = P_u = 0); groups of up to 64 rows
 *                              need none
 *   d_T, d_P                   optional [n_groups]: T_u (uint64) and P_u (uint32) of every group, valid or not
 *   d_result [4]               doubles: num = sum_valid r_u * AUC_u (GAUC = num / rows_valid), rows_valid, n_valid,
 *                              n_groups -- the three counts are exact integers
 * T_u and P_u are exact integers; the fp64 sum runs over one fixed tree per n_groups, so d_result is the same bits from
 * run to run, under any permutation of the rows (with the plan of the permuted rows) and for any order of a group's
 * members inside d_order.  No floating-point atomics.  Nothing synchronises the device; the only memory written is the
 * outputs (a missing d_T / d_P and the tree's partial sums live in a stream-ordered allocation of the call,
 * hipMallocAsync / hipFreeAsync on `stream`).
 * MAMDR_EINVAL, before any device call: a null d_result, d_group_off, or (n > 0) d_pred / d_label / d_order; n < 0 or
 * beyond int32; n_groups < 0 or > n; n_tiles < 0; a tile list given with n_tiles = 0, or n_tiles > 0 without both lists.
 * (Added within ABI 19: a new entry point only, no structure or existing call changed.) */
int mamdr_group_auc(const float* d_pred, const float* d_label, const int32_t* d_order, int64_t n,
                    const int64_t* d_group_off, int64_t n_groups,
                    const int32_t* d_tile_group, const int64_t* d_tile_first, int64_t n_tiles,
                    uint64_t* d_T, uint32_t* d_P, double* d_result, void* stream);

/* Exact AUC, average precision and equal-mass calibration bins of one split's predictions.  NO REFERENCE COUNTERPART: every
 * AUC the reference prints is AUC(num_thresholds=500), a trapezoid over 500 evenly spaced thresholds
 * (base_model.py:111-144), which stays the metric of parity and early stopping.  Stateless, any stream.
 * Definition.  Per row:
 *   key is GAUC's order-preserving 32-bit key: NaN is lowest and equals NaN, -0 equals +0.
 *   positive is label != 0.
 *   The composite is (uint64) key << 1 | positive.
 * Sort the composites ascending.  Equal composites are indistinguishable, so the sorted array is unique.  Inside a run of
 * equal keys the negatives come first.  For sorted position i:
 *   rs(i) is the first position of i's run of equal keys.
 *   cp(i) is the number of positives at positions < i.
 *   cn(i) = i - cp(i).
 * Arguments (device pointers; nothing is read back by the call):
 *   d_pred, d_label [n]   fp32 predictions and labels in file order, 0 <= n < 2^31; read only
 *   n_bins                1 .. MAMDR_EXACT_MAX_BINS
 *   d_counts [5]          int64 words T, P, N, n_runs, n_nan:
 *                         T = sum_{i positive} (cn(rs(i)) + cn(i)).  This is 2 * #{s_p > s_n} + #{s_p == s_n}, the integer
 *                         mamdr_group_auc's definition gives for the whole split as one group.  n_runs is the number of
 *                         distinct keys, n_nan the number of NaN predictions.
 *                         AUC = T / (2 * P * N); when P * N == 0 it is 0.0 with valid = 0 (recommend.ranking_metrics'
 *                         convention)
 *   d_ap [1]              one double, sum_{i positive} (double)(P - cp(rs(i))) / (double)(n - rs(i)).  Average precision
 *                         is that sum divided by P, 0.0 when P = 0: scikit-learn's step-wise definition, each positive
 *                         contributes the precision at its own threshold
 *   d_bins [3][n_bins]    int64, with every row of a run in bin floor(rs(i) * n_bins / n) (64-bit arithmetic): rows,
 *                         positives, and the sum of predictions in Q32 fixed point, floor(clamp(p, 0, 1) * 2^32 + 0.5)
 *                         evaluated in fp64, where it is exact.  A NaN prediction adds 0 and is counted in n_nan.  A tie
 *                         run is never split across bins: bins may come out EMPTY or UNEQUAL (predictions quantised to
 *                         fewer values than bins leave most bins empty)
 *   d_sorted_out [n]      optional int64: the sorted composites (the last sort pass writes them here)
 * Determinism.  All outputs are the same bits from run to run and under any permutation of the rows.  Every integer is
 * exact (integer atomics commute; the bin sums are fixed-point for that reason); each AP term is one division, and their
 * sum runs over one fixed tree per n that depends on the sorted array alone.  No floating-point atomics.
 * The sort is a least-significant-digit radix sort, the scans are three launches each; the kernel boundary is the only
 * hand-off between workgroups (csrc/exact_kernels.hip).  Nothing synchronises the device; the only memory written is the
 * outputs and a stream-ordered allocation of the call (hipMallocAsync / hipFreeAsync on `stream`) of about 17 bytes per row.
 * n = 0 writes zeros and returns MAMDR_OK.
 * MAMDR_EINVAL, before any device call: a null d_counts, d_ap, d_bins, or (n > 0) d_pred / d_label; a pointer that is not
 * aligned to its element size; n < 0 or n >= 2^31; n_bins outside 1 .. MAMDR_EXACT_MAX_BINS.
 * (Added within ABI 19: a new entry point only, no structure or existing call changed.) */
#define MAMDR_EXACT_MAX_BINS 4096
int mamdr_exact_metrics(const float* d_pred, const float* d_label, int64_t n, int32_t n_bins,
                        int64_t* d_counts, double* d_ap, int64_t* d_bins, int64_t* d_sorted_out, void* stream);

/* Bootstrap replicates of the exact AUC's integers: the statistic of mamdr_exact_metrics under integer resampling weights,
 * n_rep times over, for standard errors, confidence intervals and paired comparisons of the exact AUC
 * (mamdr_amd/bootstrap.py: finish, paired).  NO REFERENCE COUNTERPART: every figure the reference reports is a point estimate.
 * Stateless, any stream.
 * Row order.  key is GAUC's order-preserving 32-bit key: NaN is lowest and equals NaN, -0 equals +0.  positive is
 * label != 0.  The sorted order is ascending in (key, positive, row index): inside a run of equal keys the negatives come
 * first, as in mamdr_exact_metrics, and equal (key, positive) pairs order by row index, which makes the sorted array unique.
 * Unit.  unit(i) = d_unit ? (uint32) d_unit[i] : (uint32) i, with i the row's index in file order.  Passing the split's uid
 * column resamples users (the cluster bootstrap: a user's rows are correlated); NULL resamples rows.
 * Weight.  For replicate b = 1 .. n_rep: w(b, i) = poisson1(u32(b, unit(i))).
 *   u32(b, x) = the high 32 bits of mix64(mix64(seed + 0x9E3779B97F4A7C15 * (uint64) b) ^ (uint64) x).
 *   mix64 is the splitmix64 finaliser: z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
 *   z ^= z >> 31.  All arithmetic is mod 2^64.
 *   poisson1(u) = the number of k >= 0 with u >= MAMDR_BOOT_THR[k], where THR[k] = floor(2^32 * sum_{j <= k} e^-1 / j!),
 *   listed up to and including the first k where it reaches 2^32 - 1: a Poisson(1) draw to 32 bits, at most
 *   MAMDR_BOOT_WMAX.
 *   Replicate 0 is the unweighted statistic: w(0, .) = 1.
 * Outputs (device pointers; nothing is read back by the call), arrays [n_rep + 1], slot b for replicate b:
 *   d_P[b] = sum_{positive i} w(b, i).
 *   d_N[b] = sum_{negative i} w(b, i).
 *   d_T[b] = sum_{positive i} w(b, i) * (Cn_b(rs(i)) + Cn_b(i)), with Cn_b(j) the weight of negatives at sorted positions < j
 *   and rs(i) the first position of i's run of equal keys.  That is 2 * #{s_p > s_n} + #{s_p == s_n} with every pair counted
 *   w_p * w_n times: mamdr_exact_metrics' T under weights.  Slot 0 is therefore exactly mamdr_exact_metrics' (T, P, N).
 *   AUC_b = T_b / (2 * P_b * N_b) is formed on the host in fp64.  A replicate with P_b * N_b = 0 is invalid; it is
 *   reported, not hidden.
 * Bounds.  0 <= n < 2^27: a replicate's weights add up to S <= n * MAMDR_BOOT_WMAX < 2^27 * 13 < 2^31, P_b + N_b = S gives
 * 2 * P_b * N_b <= S^2 / 2 < 2^61, and T_b <= 2 * P_b * N_b: every word fits 64 bits, every partial sum 32.
 * 0 <= n_rep <= 65,535.  n = 0 writes zeros and returns MAMDR_OK.
 * Determinism.  Every output word is an exact integer: integer atomics commute, and there is no floating-point arithmetic
 * on the device at all.  The bits depend on (values, file order or unit ids, seed) alone, not on grid, tiling or chunking.
 * With d_unit = NULL the replicates do depend on file order, which is inherent to resampling rows; slot 0 does not.
 * Two calls with the same seed, labels and units give every row the same weights: their d_P and d_N are identical and
 * their replicates are paired.
 * The sort is mamdr_exact_metrics' radix sort on a wider word; the weights are recomputed where they are used, never
 * stored (csrc/bootstrap_kernels.hip).  Nothing synchronises the device; the only memory written is the outputs and a
 * stream-ordered allocation of the call (hipMallocAsync / hipFreeAsync on `stream`): about 17 bytes per row and 12 bytes
 * per (tile of 1,024 rows, replicate), the latter bounded by 64 MiB -- more replicates than fit run in chunks.
 * mamdr_auc_bootstrap_bounded is the same call with that bound given in 32-bit words (> 0; the tests force the chunking
 * with it): the outputs do not depend on it.
 * MAMDR_EINVAL, before any device call: a null d_T, d_P, d_N, or (n > 0) d_pred / d_label; a pointer that is not aligned
 * to its element size; n < 0 or n >= 2^27; n_rep < 0 or n_rep > 65,535; part_words <= 0.
 * (Added within ABI 19: a new entry point only, no structure or existing call changed.) */
#define MAMDR_BOOT_WMAX 13
#define MAMDR_BOOT_THR {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, \
                        4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u}
int mamdr_auc_bootstrap(const float* d_pred, const float* d_label, const int32_t* d_unit, int64_t n, int32_t n_rep,
                        uint64_t seed, uint64_t* d_T, int64_t* d_P, int64_t* d_N, void* stream);
int mamdr_auc_bootstrap_bounded(const float* d_pred, const float* d_label, const int32_t* d_unit, int64_t n, int32_t n_rep,
                                uint64_t seed, uint64_t* d_T, int64_t* d_P, int64_t* d_N, int64_t part_words, void* stream);

/* Isotonic regression of one split's (prediction, label) pairs -- the pool-adjacent-violators fit behind recalibration and
 * the CORP score decomposition (mamdr_amd/isotonic.py: corp, finish) --, its application to other predictions, and the Brier
 * and log-loss sums of a split.  NO REFERENCE COUNTERPART: the reference never looks at calibration.  Stateless, any stream.
 * Rows and runs.  Per row: key is GAUC's order-preserving 32-bit key (NaN is lowest and equals NaN, -0 equals +0); positive
 * is label != 0.  Sort by key ascending.  A run is a maximal set of rows with one key; run j has r_j rows and s_j positives.
 * Points Q_0 = (0, 0), Q_{j+1} = Q_j + (r_j, s_j), R runs in all.  NaN predictions form the lowest run and take part like
 * any other; n_nan is reported.
 * Fit.  The blocks are the maximal groups of consecutive runs between consecutive STRICT vertices of the lower convex hull
 * of Q_0 .. Q_R: with A, B, C consecutive candidates, B is dropped exactly when
 * (B.x - A.x) * (C.y - B.y) - (B.y - A.y) * (C.x - B.x) <= 0 in int64 (coordinates are below 2^31, the products below 2^62).
 * Equivalently: PAV over the runs, pooling the last two blocks while mean_left >= mean_right.  Block means are strictly
 * increasing.  Value v_b = (float)((double)positives[b] / (double)rows[b]): one fp64 division, rounded once to fp32.
 * mamdr_isotonic_fit (device pointers; nothing is read back by the call):
 *   d_pred, d_label [n]   fp32 predictions and labels in file order, 0 <= n < 2^31; read only
 *   d_counts [4]          int64 words n_blocks, n_runs, n_nan, P (the positives)
 *   d_first_key, d_rows, d_positives   capacity n each (uint32, int64, int64); the first n_blocks entries are written:
 *                         the key of the block's first run, its rows, its positives
 * mamdr_isotonic_fit_bounded is the same call with tile_points given, the points per tile of the hull's levels
 * (>= MAMDR_ISOTONIC_MIN_TILE; mamdr_isotonic_fit uses 64; the tests force several tiles and levels on small inputs with
 * it): the outputs do not depend on it.
 * Determinism.  The fit is integer arithmetic throughout -- no floating point, no atomics -- and the hull is unique: the
 * outputs are the same bits from run to run, under any permutation of the rows and under any tile_points.
 * The sort is mamdr_exact_metrics' radix sort; run heads and positives are counted by three-launch scans; the hull is built
 * by levels of per-tile monotone chains (a strict vertex of the whole hull is a strict vertex of the hull of every
 * contiguous subset that holds it) whose number the host fixes from n and tile_points alone, and finished by one chain
 * over what is left; the kernel boundary is the only hand-off between workgroups (csrc/isotonic_kernels.hip).  A diagram
 * that never shrinks (strictly convex: every run its own block) leaves all its points to that last chain, on one lane.
 * Nothing synchronises the device; the only memory written is the outputs and a stream-ordered allocation of the call
 * (hipMallocAsync / hipFreeAsync on `stream`) of about 33 bytes per row.
 * mamdr_isotonic_apply: for a row with key k, b = max(0, #{blocks with first_key <= k} - 1), d_out[i] = v_b -- a step
 * function, clipped at both ends (a NaN prediction, the lowest key, gets block 0).  n_blocks >= 1 when n > 0.  No allocation.
 * mamdr_score_sums: d_out [2] doubles, with y = positive and p widened to fp64: the Brier sum, sum (p - y)^2, and the
 * log-loss sum, sum -[y ln q + (1 - y) ln(1 - q)] with q = clamp(p, 1e-7, 1 - 1e-7) (the Keras epsilon).  A NaN prediction
 * makes both NaN.  Each sum runs over one fixed tree per n, without floating-point atomics: the same bits from run to run.
 * Workspace: a stream-ordered allocation of 16 bytes per 1,024 rows.
 * n = 0 writes zeros (nothing, for mamdr_isotonic_apply) and returns MAMDR_OK.
 * MAMDR_EINVAL, before any device call: a null d_counts / d_out, or (n > 0) any other null pointer; a pointer that is not
 * aligned to its element size; n < 0 or n >= 2^31; tile_points < MAMDR_ISOTONIC_MIN_TILE; n_blocks < 0 or >= 2^31, or
 * n_blocks = 0 while n > 0.
 * (Added within ABI 19: new entry points only, no structure or existing call changed.) */
#define MAMDR_ISOTONIC_MIN_TILE 4
int mamdr_isotonic_fit(const float* d_pred, const float* d_label, int64_t n, int64_t* d_counts, uint32_t* d_first_key,
                       int64_t* d_rows, int64_t* d_positives, void* stream);
int mamdr_isotonic_fit_bounded(const float* d_pred, const float* d_label, int64_t n, int64_t* d_counts, uint32_t* d_first_key,
                               int64_t* d_rows, int64_t* d_positives, int32_t tile_points, void* stream);
int mamdr_isotonic_apply(const uint32_t* d_first_key, const int64_t* d_rows, const int64_t* d_positives, int64_t n_blocks,
                         const float* d_pred, int64_t n, float* d_out, void* stream);
int mamdr_score_sums(const float* d_pred, const float* d_label, int64_t n, double* d_out, void* stream);

/* Gram matrices of up to MAMDR_GRAM_MAX_VEC flat fp32 vectors over column ranges, in fp64 -- the reduction behind the
 * domain-conflict report (the cosines between the domains' gradients).  NO REFERENCE COUNTERPART: the reference argues
 * that domains conflict and never measures it.  Stateless, any stream, no synchronisation, no allocation: the workspace
 * is the caller's.
 *   d_vecs, stride, n_vec, n_cols   vector i is d_vecs + i * stride, n_cols floats long; stride >= n_cols; n_vec in
 *                                   [1, MAMDR_GRAM_MAX_VEC]; d_vecs 4-byte aligned (nothing wider is assumed)
 *   h_off, h_count [n_range]        HOST arrays: range r is columns [h_off[r], h_off[r] + h_count[r]) inside [0, n_cols).
 *                                   Ranges may overlap, may be empty and may start at any element
 *   d_work, work_doubles            workspace of at least mamdr_gram_work(n_vec, h_off, h_count, n_range) doubles
 *   d_out [n_range][n_vec][n_vec]   out[r][i][j] = sum over k in range r of (double) v_i[k] * (double) v_j[k]; the full
 *                                   matrix is written, out[r][i][j] and out[r][j][i] are the same bits; an empty range
 *                                   gives zeros
 * Arithmetic.  Every product is formed in fp64 from the two fp32 values (48 significant bits: exact) and accumulated in
 * fp64, on the f64 matrix cores.  No floating-point atomics.
 * Reduction order.  Range r is cut, from ITS first column, into slabs of MAMDR_GRAM_SLAB columns; every slab's partial
 * matrix goes to d_work; a second launch adds a range's partials in ascending slab order.  Inside a slab the order of k
 * per output element is fixed.  The bits of d_out therefore depend on the values and the range table alone -- not on
 * stride, on where the buffers sit, on their alignment or on the grid --, and a range of an overlapping request gets the
 * bits it gets when asked for alone.  NaN and Inf propagate as IEEE: they reach their own vector's row and column only.
 * MAMDR_EINVAL, with the argument named and nothing launched: n_vec outside [1, MAMDR_GRAM_MAX_VEC]; stride < n_cols; a
 * range that is negative or leaves [0, n_cols); a null pointer; d_vecs not 4-byte, d_work or d_out not 8-byte aligned;
 * work_doubles below mamdr_gram_work's answer.  mamdr_gram_work returns MAMDR_EINVAL for a bad n_vec or range table.
 * (Added within ABI 19: new entry points only, no structure or existing call changed.) */
#define MAMDR_GRAM_SLAB 16384
#define MAMDR_GRAM_MAX_VEC 32
int64_t mamdr_gram_work(int32_t n_vec, const int64_t* h_off, const int64_t* h_count, int32_t n_range);
int mamdr_gram(const float* d_vecs, int64_t stride, int32_t n_vec, int64_t n_cols,
               const int64_t* h_off, const int64_t* h_count, int32_t n_range,
               double* d_work, int64_t work_doubles, double* d_out, void* stream);

/* What top-K lists are made of -- the two device reductions behind the beyond-accuracy report (mamdr_amd/list_metrics.py:
 * coverage, Gini, entropy, novelty, personalisation, intra-list diversity).  NO REFERENCE COUNTERPART: the reference never
 * builds a list.  Stateless, any stream, no synchronisation, no allocation; both calls take lists from anywhere.
 *
 * mamdr_id_counts: a histogram of int32 ids.
 *   d_ids [n], d_label [n] or null  d_counts[i] = the number of positions j with d_ids[j] == i -- with a label column, of
 *                                   those with d_label[j] != 0 (fp32 compare: -0.0 is 0, NaN is not).  An id outside
 *                                   [0, n_bins) counts nowhere: the -1 padding of a short list, a foreign id
 *   d_counts [n_bins]               zeroed by the call on `stream`, then counted into
 *   The two inputs it serves: item EXPOSURE -- the flattened [Q][K] lists, no labels -- and item POPULARITY -- a train
 *   split's pid and label columns, which already live on the device.  Integer atomics only: the same bits whatever order
 *   the workgroups run in.  n == 0 zeroes the counts and returns MAMDR_OK (the two input pointers may then be null).
 *   MAMDR_EINVAL, nothing launched: a null d_counts, a null d_ids with n > 0, a pointer not 4-byte aligned, n < 0,
 *   n >= 2^32 (a count is 32 bits), n_bins <= 0.
 *
 * mamdr_list_similarity: the sum of pairwise cosines inside every list, over rows of an embedding table.
 *   d_ids [n_list][k]               k in 1 .. MAMDR_LIST_MAX_K.  An entry of list q is VALID when its id lies inside
 *                                   [0, n_rows); every other id is padding, wherever it sits in the list.  Duplicate ids
 *                                   are simply two entries
 *   d_rows [n_rows][emb_dim]        fp32, 16-byte aligned, emb_dim 32, 64, 128 or 256 (the widths the project trains at)
 *   d_pairs [n_list]                L (L - 1) / 2 with L the list's valid entries
 *   d_sim_sum [n_list]              sum over the valid entries a < b, in list order, of cos(x_a, x_b)
 * Arithmetic.  cos = (x_a . x_b) / (|x_a| |x_b|), exactly 0 when either norm is 0.  Dots and squared norms are fp32, on
 * the fp32 matrix cores: one fma chain per dot product over the columns in a fixed order; the squared norms are the Gram
 * matrix's own diagonal.  Square root and the two divisions (g / |x_a|) / |x_b| are IEEE (correctly rounded).  The fp32
 * cosines are added in fp64.  Against the fp64 definition on the same fp32 rows (list_metrics.list_similarity_host):
 * |d_sim_sum - host| <= d_pairs * (2 emb_dim + 8) * 2^-24.  NaN and Inf rows propagate as IEEE into their own pairs.
 * Order.  Every order -- of the columns inside a dot product, of the cosines inside the sum -- depends on the list's own
 * valid entries alone.  No floating-point atomics.  A list's two outputs are the same bits from run to run, wherever the
 * list sits in the call, whatever its neighbours are, wherever its padding sits and whatever k the call has.
 * MAMDR_EINVAL, nothing launched: a null pointer; d_ids / d_pairs not 4-byte, d_sim_sum not 8-byte, d_rows not 16-byte
 * aligned; n_list <= 0; k outside 1 .. MAMDR_LIST_MAX_K; emb_dim not one of the four widths; n_rows <= 0.
 * (Added within ABI 19: new entry points only, no structure or existing call changed.) */
#define MAMDR_LIST_MAX_K 128
int mamdr_id_counts(const int32_t* d_ids, const float* d_label, int64_t n, int64_t n_bins, uint32_t* d_counts,
                    void* stream);
int mamdr_list_similarity(const int32_t* d_ids, int32_t n_list, int32_t k, const float* d_rows, int64_t n_rows,
                          int32_t emb_dim, double* d_sim_sum, int32_t* d_pairs, void* stream);

/* mamdr_list_diversify: greedy Maximal Marginal Relevance (Carbonell & Goldstein 1998) -- out of every list's n candidates,
 * k picks that trade relevance against similarity to what is already picked.  NO REFERENCE COUNTERPART.  Stateless, any
 * stream, no synchronisation, no allocation; the only memory written is the two outputs.
 *   d_ids [n_list][n]               n in 1 .. MAMDR_LIST_MAX_K; valid / padding as mamdr_list_similarity: an id inside
 *                                   [0, n_rows) is valid, anything else is padding wherever it sits.  Valid ids are
 *                                   DISTINCT within a list (not checked; which of two duplicates wins a tie is unspecified)
 *   d_rel [n_list][n]               each entry's relevance, fp32, used as given (not normalised)
 *   d_rows [n_rows][emb_dim]        as mamdr_list_similarity: fp32, 16-byte aligned, emb_dim 32, 64, 128 or 256
 *   k in 1 .. n, lambda in [0, 1]
 *   d_pos_out [n_list][k]           the position in the input list (0 .. n - 1) of pick t; -1 behind a short list
 *   d_value_out [n_list][k] or null the value pick t won with (its relevance at step 0); 0 behind a short list
 * Definition, per list: its valid entries in list order are e_0 .. e_{L-1}.
 *   cos(a, b), a < b                exactly the fp32 number mamdr_list_similarity forms for that pair standing in that
 *                                   order: the same fma chain for the dot product and the squared norms, the quotient
 *                                   (g / sqrtf(n_a)) / sqrtf(n_b) with a the earlier entry, 0 when either squared norm is 0
 *   oml = 1.0f - lambda             in fp32
 *   step 0                          the entry with the largest key (rel, id): the highest relevance, equal relevance by
 *                                   ascending id, NaN behind every number (the retrieval family's ranking key: fp32
 *                                   values order by their bits, so -0.0 stands behind +0.0)
 *   step t >= 1                     for every entry c not yet picked, m_c = the running maximum of cos(c, s) over the
 *                                   picks s so far (the first pick's cosine, then `cos > m ? cos : m`) and
 *                                   v_c = (lambda * rel_c) - (oml * m_c): three fp32 roundings, no fused multiply-add.  The
 *                                   entry with the largest key (v_c, id_c) is picked
 *   stop                            after min(k, L) picks
 * A list's outputs are the same bits from run to run, wherever the list sits in the call, whatever its neighbours hold,
 * wherever its padding sits and for any n >= its last valid position + 1.  At lambda = 1 and finite rows the picks are
 * the stable order by (rel descending, id ascending).  No floating-point atomics.  Against the float64 definition on the
 * same fp32 inputs (list_metrics.diversify_host), with rel in [0, 1]: a pick's float64 value is within
 * 2 tol of the step's best, tol = ((1 - lambda) (2 emb_dim + 8) + 8) * 2^-24.
 * MAMDR_EINVAL, nothing launched: a null required pointer; d_ids / d_rel / d_pos_out / d_value_out not 4-byte, d_rows not
 * 16-byte aligned; n_list <= 0; n outside 1 .. MAMDR_LIST_MAX_K; k outside 1 .. n; emb_dim not one of the four widths;
 * n_rows <= 0; lambda outside [0, 1] or NaN.
 * (Added within ABI 19: a new entry point only, no structure or existing call changed.) */
int mamdr_list_diversify(const int32_t* d_ids, const float* d_rel, int32_t n_list, int32_t n, int32_t k, float lambda,
                         const float* d_rows, int64_t n_rows, int32_t emb_dim, int32_t* d_pos_out, float* d_value_out,
                         void* stream);

/* mamdr_row_neighbours: for every query row of a table, its k nearest candidate rows by cosine -- exact, the whole
 * query set x candidate set cosine matrix with the per-query selection fused behind it ("items like this one", and across
 * catalogues "the items of B closest to this item of A").  NO REFERENCE COUNTERPART.  Stateless, any stream, no
 * synchronisation; the only memory written is the two outputs and a stream-ordered allocation of the call's own (squared
 * norms of the queries and of a pass's candidates, and each query's running lists).
 *   d_rows [n_rows][emb_dim]        fp32, 16-byte aligned; emb_dim 32, 64, 128 or 256, as mamdr_list_similarity takes them
 *   d_query [n_query]               row ids.  An id outside [0, n_rows) is no error: that query's list is all padding
 *   d_cand [n_cand] or null         candidate row ids; null = "candidate p is row p", with n_cand = n_rows.  Ids are
 *                                   DISTINCT (not checked; with duplicates, which copies appear is unspecified).  An id
 *                                   outside [0, n_rows) is never returned
 *   exclude_self                    != 0: the candidate whose id equals the query's id is skipped
 *   k in 1 .. MAMDR_KNN_MAX_K
 *   d_ids_out, d_sim_out [n_query][k]  the query's eligible candidates by cosine descending, equal cosines by ascending
 *                                   id -- the retrieval family's ranking key on (cos, id): fp32 values order by their bits
 *                                   (-0.0 behind +0.0), a NaN cosine stands behind every number (and is returned as the
 *                                   quiet NaN 0x7fc00000).  A list with fewer than k eligible candidates ends in
 *                                   id -1 / sim 0.0f
 * Definition: cos(q, c) is exactly the fp32 number mamdr_list_similarity forms for the two-entry list [q, c]: the same
 * fma chain over the columns for the dot product, the squared norms with the bits of that chain applied to the row with
 * itself, the quotient (g / sqrtf(n_q)) / sqrtf(n_c) with IEEE square root and division and the query in the earlier
 * entry's place, exactly 0 when either squared norm is 0 (IEEE propagation otherwise).
 * Determinism: distinct ids give distinct keys, so a query's list is ONE list; its bytes do not depend on where the query
 * stands in the call or what its neighbours are, on the order of d_cand, on the grid, the tile shapes or `chunk`.  No
 * floating-point atomics.
 * mamdr_row_neighbours_bounded is the same call with the number of candidates per pass given: chunk > 0, rounded up to the
 * tile width (64); passes carry every query's running best.  The plain call picks a default.
 * MAMDR_EINVAL, nothing launched: a null d_rows / d_query / d_ids_out / d_sim_out; d_rows not 16-byte, the others not
 * 4-byte aligned; n_rows <= 0 or >= 2^31; emb_dim not one of the four widths; n_query <= 0; n_cand <= 0, or
 * n_cand != n_rows with a null d_cand; k outside 1 .. MAMDR_KNN_MAX_K; chunk <= 0.
 * (Added within ABI 19: new entry points only, no structure or existing call changed.) */
#define MAMDR_KNN_MAX_K 128
int mamdr_row_neighbours(const float* d_rows, int64_t n_rows, int32_t emb_dim, const int32_t* d_query, int32_t n_query,
                         const int32_t* d_cand, int64_t n_cand, int32_t exclude_self, int32_t k, int32_t* d_ids_out,
                         float* d_sim_out, void* stream);
int mamdr_row_neighbours_bounded(const float* d_rows, int64_t n_rows, int32_t emb_dim, const int32_t* d_query,
                                 int32_t n_query, const int32_t* d_cand, int64_t n_cand, int32_t exclude_self, int32_t k,
                                 int32_t* d_ids_out, float* d_sim_out, int32_t chunk, void* stream);

/* The baselines a ranking table is read against -- MostPopular and ItemKNN under the protocol of mamdr_rank_domain -- and
 * the two calls that rank from a score matrix no tower produced: mamdr_item_cooc, mamdr_history_scores, mamdr_rank_scores,
 * mamdr_topk_scores (mamdr_amd/baselines.py holds the host definitions and the report).  NO REFERENCE COUNTERPART: the
 * reference never ranks.  Stateless: no context, any stream, no synchronisation, nothing read back; the only memory written
 * is the outputs and, in mamdr_history_scores, a stream-ordered allocation of the call's own (m floats).  Wave64; integer
 * atomics only; nothing depends on the order in which workgroups arrive.
 *
 * Histories.  A CSR over users: d_hist_off [n_user + 1] int64 ascending from 0 to nnz, d_hist_pos [nnz] int32 positions in a
 * catalogue of m items, inside [0, m), ascending and distinct within a user (build and check it on the host:
 * baselines.histories).  nnz is a host argument.  The kernels clamp both ends of every user's range into [0, nnz] and skip a
 * position outside [0, m): a broken CSR gives wrong numbers, never an access outside the arrays.
 *
 * mamdr_item_cooc: d_cooc [m][m] uint32, zeroed by the call on `stream`, then C[a][b] = the number of users whose history
 *   holds both a and b; the diagonal C[a][a] is the number of users that hold a.  The full symmetric matrix is stored: the
 *   scorer reads row j as contiguous memory.  One integer atomic per ordered pair of a history (sum over users of L_u^2
 *   adds; a history longer than a workgroup is strided over, all L^2 pairs are made; one wave-instruction's adds go along
 *   one row of C).  Integers only: the same bits whatever order the workgroups run in.
 *   MAMDR_EINVAL, nothing launched: a null d_hist_off or d_cooc; a null d_hist_pos with nnz > 0; d_hist_off not 8-byte,
 *   d_hist_pos / d_cooc not 4-byte aligned; nnz < 0; m <= 0 or m > 65,535; n_user <= 0.
 *
 * mamdr_history_scores: the ItemKNN score of every catalogue item for the users d_query [n_query] (indices into the CSR; an
 *   index outside [0, n_user) is no error: that row is all +0.0f), d_scores [n_query][m] fp32.  Fixed to the bit: with
 *   n_a = float(C[a][a]) (exact: counts stay below 2^24 -- the call checks n_user < 2^24; a caller's own matrix with a
 *   larger diagonal is outside the contract),
 *     sim(c, j) = float(C[c][j]) / (sqrtf(n_c) * sqrtf(n_j) + shrink)     for c != j and C[c][j] > 0,
 *     sim(c, j) = +0.0f                                                   otherwise,
 *   every operation separately rounded, IEEE square root and division, no contraction; score[q][c] is the fp32 sum of
 *   sim(c, j) over j in H(q) in ascending history order, started from +0.0f, one add per history entry.
 *   Consequences: a row's bytes do not depend on where the query stands in the call, on its neighbours or on the grid
 *   (every output element is owned by one lane for the whole sum); an empty history gives an all-zero row; an item's own
 *   entry contributes nothing (a user's own items still collect the similarities to the user's OTHER items: exclude them
 *   in the ranking calls); an item nobody holds scores +0.0f everywhere, at shrink = 0 too (its counts are all 0).
 *   d_cooc is read with 16-byte loads where m is a multiple of 4 and d_cooc / d_scores are 16-byte aligned, with 4-byte
 *   loads otherwise: the same bits either way.
 *   MAMDR_EINVAL, nothing launched: a null d_cooc, d_hist_off, d_query or d_scores; a null d_hist_pos with nnz > 0; a
 *   misaligned pointer (d_hist_off 8, the others 4 bytes); nnz < 0; m <= 0 or m > 65,535; n_user <= 0 or >= 2^24;
 *   n_query <= 0; shrink outside [0, 2^20] or NaN.
 *
 * mamdr_rank_scores: mamdr_rank_domain's Rank and Live with "logit" replaced by d_scores[q * row_stride + p] for
 *   candidate position p.
 *   d_scores, row_stride            fp32; row_stride int64 counts elements: 0 = one row serves every query (MostPopular),
 *                                   otherwise >= n_cand
 *   d_cand [n_cand] or null         the id of position p, ASCENDING and distinct (the caller's contract: a catalogue is
 *                                   np.unique's output); null = "the id of position p is p"
 *   d_excl_off [n_query + 1], d_excl_ids   as in the tower calls: CSR by query, ids ascending; both or neither
 *   d_tgt_off [n_query + 1], d_tgt_ids [n_tgt]   the targets' CSR, ids ascending and distinct per query; n_tgt is a host
 *                                   argument (nothing is read back); offsets are clamped into [0, n_tgt]
 *   d_rank_out [n_tgt] int32, d_score_out [n_tgt] fp32 or null, d_live_out [n_query] int32
 *   key(q, p) = rec_key(score, id of p): (order-preserving bits of the score << 32) | ~id -- a larger key is a higher score
 *   or an equal score and a smaller id; -0 counts as +0; a NaN is behind every number.  A position is live for q when its
 *   id is not in q's exclusion list.
 *   Rank.  A target's key is the key of the candidate position that holds its id (binary search).  d_rank_out[j] =
 *     #{ p live for q : key(q, p) > key(q, target) }.  A target that is not among the candidates gets rank -1 and score 0.
 *     A target that is among the candidates but excluded is ranked as mamdr_rank_domain ranks it: against the live ones.
 *   Score.  d_score_out[j] = the raw bits d_scores holds for the pair.   Live.  d_live_out[q] = live positions of q.
 *   Link to top-K.  A live candidate t sits at position r of mamdr_topk_scores' list exactly when its rank is r < k.
 *   All outputs are integers or copied bits -- no floating-point arithmetic at all: a pure function of the input bits.
 *   MAMDR_EINVAL, nothing launched: a null d_scores, d_tgt_off or d_live_out; a null d_rank_out or d_tgt_ids with
 *   n_tgt > 0; exclusion offsets without ids or ids without offsets; a misaligned pointer (the offsets 8, the others 4
 *   bytes); n_query <= 0; n_cand <= 0 or >= 2^31; row_stride < 0 or 0 < row_stride < n_cand; n_tgt < 0.
 *
 * mamdr_topk_scores: the first k <= MAMDR_SCORES_MAX_K live positions of the same ordering, as (id, score) in
 *   d_ids_out / d_scores_out [n_query][k]; a short list ends in id -1 / score 0.0f; the score is decoded from the key (a
 *   NaN leaves as 0x7fc00000, as mamdr_row_neighbours returns it; a -0.0 as +0.0).  Distinct ids give distinct keys: a
 *   query's list is ONE list, whatever the tiles.
 *   MAMDR_EINVAL, nothing launched: a null d_scores, d_ids_out or d_scores_out; the exclusion lists, alignment, n_query,
 *   n_cand and row_stride as above; k outside 1 .. MAMDR_SCORES_MAX_K.
 * Slates from scores (the sampled-negatives protocol) are out of scope: with the dense matrix on the device a caller
 * gathers them.  (Added within ABI 19: new entry points only, no structure or existing call changed.) */
#define MAMDR_SCORES_MAX_K 128
int mamdr_item_cooc(const int64_t* d_hist_off, const int32_t* d_hist_pos, int64_t nnz, int32_t n_user, int32_t m,
                    uint32_t* d_cooc, void* stream);
int mamdr_history_scores(const uint32_t* d_cooc, int32_t m, const int64_t* d_hist_off, const int32_t* d_hist_pos,
                         int64_t nnz, int32_t n_user, const int32_t* d_query, int32_t n_query, float shrink,
                         float* d_scores, void* stream);
int mamdr_rank_scores(const float* d_scores, int64_t row_stride, int32_t n_query, const int32_t* d_cand, int64_t n_cand,
                      const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                      const int32_t* d_tgt_ids, int64_t n_tgt, int32_t* d_rank_out, float* d_score_out,
                      int32_t* d_live_out, void* stream);
int mamdr_topk_scores(const float* d_scores, int64_t row_stride, int32_t n_query, const int32_t* d_cand, int64_t n_cand,
                      const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out,
                      float* d_scores_out, void* stream);

/* --- outer (meta) updates on flat vectors; stateless, any stream.  Each op is
 *     evaluated with one fp32 rounding per arithmetic step in the reference's
 *     order (no FMA contraction) and matches its numpy result bit-for-bit.
 *
 * dst[i] += (a[i] - b[i]) * scale
 *   DN / Reptile: model_zoo/domain_negotiation.py:118-123, reptile.py:127-132
 *   MAMDR:        model_zoo/mamdr.py:173-180 (b = merged or dst itself) */
int mamdr_interp(float* d_dst, const float* d_a, const float* d_b, float scale, int64_t n,
                 void* stream);
/* average_meta_grad == "moving_mean": `K.moving_average_update(ag, g, 0.999)` (model_zoo/maml.py:219-220,
 * mldg.py:222-223, pcgrad.py:229-230) = TF 1.12's zero-debiased moving average of the accumulator variable:
 *   biased[i] -= (biased[i] - value[i]) * decay;   unbiased[i] -= unbiased[i] - biased[i] / denom
 * decay = float(1 - momentum); denom = 1 - (1 - decay)^local_step, formed by the caller (float32, local_step =
 * number of updates since the accumulator was created, this one included).  One rounding per operation. */
int mamdr_moving_average(float* d_unbiased, float* d_biased, const float* d_value, float decay, float denom,
                         int64_t n, void* stream);
/* dst[i] = theta[i] + phi[i]  or  theta[i] * phi[i]  (specific_base_model.py:164-172) */
int mamdr_merge(float* d_dst, const float* d_theta, const float* d_phi, int32_t mode, int64_t n,
                void* stream);
/* One Domain-Regularisation support step on flat vectors in a single pass (mamdr.py:103-105, then the next
 * support's assignment of the merged weights to the model, mamdr.py:74):
 *   phi[i] += (w[i] - merged[i]) * gamma;  merged[i] = theta[i] (+|*) phi[i];  if (assign_model) w[i] = merged[i]
 * bit-identical to mamdr_interp(phi, w, merged, gamma) + mamdr_merge(merged, theta, phi, mode) + mamdr_copy(w, merged). */
int mamdr_dr_advance(float* d_phi, float* d_w, float* d_merged, const float* d_theta, float gamma, int32_t mode,
                     int32_t assign_model, int64_t n, void* stream);
/* The same on the context's LIVE weights, range [meta_off, meta_off + n) of the bound vector (d_w = live + meta_off):
 * what a caller gets from mamdr_sync_tables(ctx) followed by mamdr_dr_advance(.., live + meta_off, ..) -- the library
 * brings the live state up to date itself, and a domain-table step the fused step path left pending is materialised
 * inside the same launch.  Same bits. */
int mamdr_dr_advance_live(mamdr_ctx* ctx, float* d_phi, float* d_merged, const float* d_theta, float gamma, int32_t mode,
                          int32_t assign_model, int64_t meta_off, int64_t n);
/* dst[i] = a[i] - b[i]   (mamdr.py:168-171) */
int mamdr_sub(float* d_dst, const float* d_a, const float* d_b, int64_t n, void* stream);
/* acc[i] += (a[i] - b[i]) [* shared[i]] / divisor   (reptile.py:134-137 with shared NULL,
 * divisor 1; mamdr.py:182-191) */
int mamdr_accumulate(float* d_acc, const float* d_a, const float* d_b, const float* d_shared,
                     float divisor, int64_t n, void* stream);
/* dst[i] += acc[i] / divisor * scale; acc[i] = 0   (mamdr.py:193-196; reptile.py:139-142
 * with divisor <= 0 meaning "no division") */
int mamdr_apply_accumulated(float* d_dst, float* d_acc, float divisor, float scale, int64_t n,
                            void* stream);
/* TF1 Adam on flat vectors with caller-owned slots: the OUTER optimiser of MAML
 * (`self.meta_optimizer.apply_gradients`, model_zoo/maml.py:201,215,236-243).
 *   alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power), powers AFTER this step's update
 *   m += (g - m)(1 - beta1); v += (g*g - v)(1 - beta2); p -= m * alpha / (sqrt(v) + eps);
 *   grad_scale multiplies g first (average_meta_grad = "mean", maml.py:208-210; 1 otherwise). */
int mamdr_adam_apply(float* d_p, float* d_m, float* d_v, const float* d_g, float grad_scale, float lr,
                     float beta1, float beta2, float eps, float beta1_power, float beta2_power, int64_t n,
                     void* stream);
/* dst[i] = src[i]: SetVarOp.__call__ / K.batch_get_value without the host round
 * trip (utils/tool.py:36-45, maml.py:189-194) */
int mamdr_copy(float* d_dst, const float* d_src, int64_t n, void* stream);
/* PCGrad projection of one auxiliary gradient onto the running gradient, both flat device vectors, in place.
 * Replaces `PCGrad.PCGrad(final_grads, current_grads, aux_grads)` with final_grads IS current_grads
 * (model_zoo/pcgrad.py:107-124,152-160).  The n_seg tensors are given as HOST arrays: element offset, number of
 * slices along the last axis (rows), slice length (cols <= 4096); at most 24 tensors.  Bit-identical to numpy. */
int mamdr_pcgrad_project(float* d_final, float* d_aux, const int64_t* h_offsets, const int64_t* h_rows,
                         const int32_t* h_cols, int32_t n_seg, void* stream);

/* --- host-side helper: tf.data shuffle(buffer_size) order of range(n)
 *     (utils/dataset.py:27-37), splitmix64-driven; writes n int32 to HOST memory. */
int mamdr_shuffle_perm(int64_t n, int64_t buffer_size, uint64_t seed, int32_t* h_out);
/* the same for every pass of an epoch in one call: pass k is a shuffle of range(h_n[k]) with seed h_seeds[k],
 * written at h_out + sum(h_n[0..k)) (one pinned staging buffer, one upload per epoch instead of one per
 * re-initialised iterator: mamdr.py:52-53,81-82,92-93). */
int mamdr_shuffle_perms(int32_t n_passes, const int64_t* h_n, int64_t buffer_size, const uint64_t* h_seeds,
                        int32_t* h_out);

/* --- profiling: per-kernel device time from HIP events on the context's stream.
 *     enable != 0 brackets every launch of the listed kernels with events.
 *     mamdr_profile_read synchronises the stream, returns the summed milliseconds
 *     and launch count since the last reset. */
int mamdr_profile_enable(mamdr_ctx* ctx, int32_t enable);
/* A HINT about the next calls of mamdr_train_steps(_n): they will run these passes -- (domain, permutation, rows of the
 * pass; h_pass_rows null or an entry < 0: the whole split) at batch size `batch` -- in this order.  Where a call would
 * resolve and gather its pass's rows itself (frozen tables on the k_wgrad_adam path: k_pass_prep, once per call) the
 * library gathers all of them in ONE launch now, and each of those calls finds its rows ready; it matches a call by
 * (domain, d_perm pointer, pass rows, batch), skipping entries in between, and forgets the hint when a call matches
 * none (that call then gathers as before).  The permutations and the bound columns must not change in between.  At
 * most 16 passes per hint (more: the first 16); everywhere else this is a no-op.  Same rows, same bits.  No reference
 * counterpart: the reference's tf.data iterator re-reads the csv files on every pass (utils/dataset.py:20-38).
 * mamdr_pregather_hits: how many calls found their pass gathered; mamdr_pregather_launches: how many hints had their
 * window gathered ahead of its calls (by one k_pass_prep_multi launch, or by riders, see below) -- both for tests and
 * reports.
 *
 * mamdr_pregather_ahead announces the window AFTER the current one: the list mamdr_pregather_passes will be called with
 * once the caller has run `spread_steps` more steps of the k_wgrad_adam path.  On a device with more CUs than a
 * k_wgrad_adam launch has workgroups, every such step then carries a few rider workgroups that gather the next slice of
 * that window into a second set of the pass buffer; the later mamdr_pregather_passes with the same list (same domains,
 * permutation pointers, rows and batch, in the same order) adopts that set and launches k_pass_prep_multi only over the
 * positions the riders did not reach (no launch if there are none).  Any other list, a call that matches no announced
 * pass, mamdr_bind_table, mamdr_bind_domain_data and mamdr_set_tower_tile drop the announcement, and the next hint
 * gathers as without it.  A hint only: nothing happens where mamdr_pregather_passes does nothing, in a profiled context
 * (every kernel is timed on its own there), with spread_steps <= 0 or MAMDR_NO_PREGATHER_RIDE=1, or on a device without
 * idle CUs.  The permutations must be on the device when the hint is given.  Same rows, same bits.
 * mamdr_pregather_rider_rows / _remainder_rows: positions (rows and padding rows) gathered by riders / by the launches
 * over what they did not reach.  (Added within ABI 19: new entry points only, no structure or existing call changed.) */
int mamdr_pregather_passes(mamdr_ctx* ctx, int32_t n_passes, const int32_t* h_domains, const int32_t* const* h_d_perms,
                           const int64_t* h_pass_rows, int32_t batch);
int mamdr_pregather_ahead(mamdr_ctx* ctx, int32_t n_passes, const int32_t* h_domains, const int32_t* const* h_d_perms,
                          const int64_t* h_pass_rows, int32_t batch, int64_t spread_steps);
int64_t mamdr_pregather_hits(const mamdr_ctx* ctx);
int64_t mamdr_pregather_launches(const mamdr_ctx* ctx);
int64_t mamdr_pregather_rider_rows(const mamdr_ctx* ctx);
int64_t mamdr_pregather_remainder_rows(const mamdr_ctx* ctx);
/* which kernels a training step of `batch` rows launches (for reports; no reference counterpart):
 *   0  tower -> k_wgrad (split-K slabs) -> k_update
 *   1  [k_pass_prep once per call] tower -> k_wgrad_adam (weight gradients + optimiser step in one launch;
 *      MAMDR_KERNEL_WGRAD times it), the domain table's step applied by the next tower, k_dm_finish once per call
 *      (MAMDR_KERNEL_UPDATE times it) */
int mamdr_step_path(const mamdr_ctx* ctx, int32_t batch);
/* how the context's latest k_wgrad_adam launch ran (for reports and tests; -1: none yet): bit 0 = it left W1^T alone (no
 * tower of the context reads it), bit 1 = it left W2^T alone (every tower of its call read W2 in place: no transposed copy
 * was built either), bit 2 = its S workgroups took their column blocks in grid order (MAMDR_FZ_S_INORDER=1), bit 3 = its
 * workgroups were dealt their blocks by residue, every XCD the same mix, instead of by matrix (MAMDR_FZ_DEAL_RESIDUE=1, and
 * implied by bit 2) */
int mamdr_fused_flags(const mamdr_ctx* ctx);
/* rows per tower workgroup from the next call on: 0 = the library's choice (4-row tiles while the grid fits the CUs in one
 * round: ONE chain of steps then has every CU busy), 4 or 16 forced.  16 is the choice of a context that SHARES the
 * device with other contexts on other streams (the lanes of mamdr_amd/parallel.py: 64 workgroups per 1,024-row step
 * leave the other CUs to the other lanes' launches; 4 lanes: 72 K instead of 59 K domain-steps/s,
 * profiles/r05_lanes_probe.txt).  Same arithmetic per element either way; the two tiles add the split-K partials of a
 * layer in different orders (rounding-level differences, each inside the parity bars).  No reference counterpart.
 * (ABI 17; the environment's MAMDR_TOWER_TILE sets the initial value.) */
int mamdr_set_tower_tile(mamdr_ctx* ctx, int32_t rows);
/* rows per tower workgroup of a training step of `batch` rows under the present choice: 4 or 16 (for reports and tests) */
int mamdr_tower_tile(const mamdr_ctx* ctx, int32_t batch);
/* training steps taken so far (any optimiser): the position of the counter-based dropout stream, which the mask of
 * step s is keyed on (dropout_seed, s).  A caller that replays the run elsewhere continues the stream from here. */
int64_t mamdr_dropout_steps(const mamdr_ctx* ctx);
int mamdr_profile_reset(mamdr_ctx* ctx);
int mamdr_profile_read(mamdr_ctx* ctx, int32_t kernel, double* total_ms, int64_t* launches);

/* ====================================================================================================
 * Towers built from generic dense layers: the reference's multi-task baselines
 * (model_zoo/DeepMTLCTR/deep_mtl_ctr.py).  `DeepMTLCTR.build_model` (:21-67) builds deepctr's
 * SharedBottom / MMOE / PLE with one binary task per domain and compiles, per domain, `Model(inputs, outputs[d])` on ONE
 * shared tf.train.AdamOptimizer; `train()` (:69-96) fits domain d's model on domain d's batches.  A handle of its own
 * (the hot path's context is specialised to the 384-256-128-64 tower); same conventions as above.
 * The flat vector lists, in order: the domain table, the experts every task mixes, then per task its own experts (PLE),
 * its gate DNN + gate kernel, its tower DNN, its output unit and global bias (tensor names: mamdr_graph_tensor_info).
 * Frozen user / item tables are bound through mamdr_graph_bind_table; with emb_trainable = 1 (the Amazon configs) they sit
 * at the head of the flat vector and take TF1's dense Adam step (every row, every step) like any other tensor. */
enum { MAMDR_GRAPH_SHARED_BOTTOM = 0,   /* deep_mtl_ctr.py:25-30  models.SharedBottom */
       MAMDR_GRAPH_MMOE = 1,            /* deep_mtl_ctr.py:31-38  models.MMOE */
       MAMDR_GRAPH_PLE = 2,             /* deep_mtl_ctr.py:39-49  models.PLE (num_levels = 1, as in every reference config) */
       /* single-output towers of the deepctr family on the same generic layers (model_zoo/DeepCTR/deepctr.py): ONE model
          serves every domain; flat vector = [user_emb item_emb (lin_user lin_item) if trainable] domain_emb W0 W1 W2 b0 b1 b2
          wo gb (lin_domain); hidden_dim in expert_hidden, tower / gate fields unused */
       MAMDR_GRAPH_NFM = 3,             /* deepctr.py:33-35  models.NFM: linear tables + DNN(BiInteractionPooling) */
       MAMDR_GRAPH_PNN = 4,             /* deepctr.py:44-46  models.PNN: DNN([fields | pairwise inner products]) */
       /* deepctr.py:41-43  models.CCPM: convolutions (6, 1) x 4 and (5, 1) x 4 over the field axis with tanh and k-max pooling
          (k = 1 with three fields) -> DNN + linear tables; conv tensors conv1_w [6][4] conv1_b conv2_w [4][4] conv2_b precede W0 */
       MAMDR_GRAPH_CCPM = 5,
       /* deepctr.py:37-40  models.AutoInt(att_head_num=4): three InteractingLayers (4 heads x 8, residual, relu) over the three
          fields beside the DNN, Dense(1) on [attention output 96 | DNN output] + linear tables; att<l>_w = [W_query | W_key |
          W_value | W_res] ([128][128], then [32][128] twice) precede W0, wo has 96 + hidden[-1] rows */
       MAMDR_GRAPH_AUTOINT = 6,
       /* round 5: the towers of the step kernels with ANY hidden_dim of 1..4 layers (widths multiples of 64) -- the step
        * kernels are built for [256, 128, 64]; deepctr.py:26-32,36-38 pass hidden_dim through as dnn_hidden_units.
        * Flat layout = oracle/tower.param_names: [tables | 1-d linear tables] domain_emb | W0.. | b0.. | wo | gb | lin_domain */
       MAMDR_GRAPH_MLP = 7,             /* deepctr.py:118-136 build_mlp: DNN(x) -> Dense(1) -> sigmoid */
       MAMDR_GRAPH_WDL = 8,             /* deepctr.py:29-32  models.WDL: linear tables + DNN(x) */
       MAMDR_GRAPH_DEEPFM = 9,          /* deepctr.py:36-38  models.DeepFM: linear tables + FM second-order term + DNN(x) */
       /* model_zoo/Star/star.py:70-96 as a family (ABI 19): norm none / PartitionedNorm / BatchNormalization (star_norm), plain
        * Dense or StarFCN hidden layers (star_dense), the auxiliary network (auxiliary_dim), hidden_dim of 1..4 layers in
        * expert_hidden; 128-wide embeddings only.  No dropout and no regularisers (dropout, l2_emb, l2_linear are ignored).  The
        * per-domain tensors are read at d = the domain id of the batch's FIRST row; the other domains' slices take a zero
        * gradient and still the Adam step.  Flat layout: [user_emb item_emb if trainable] domain_emb | Ws0.. bs0.. (dense: W0..
        * b0..) | pn_gamma_shared pn_beta_shared pn_gamma_spec pn_beta_spec (bn: bn_gamma bn_beta) | Wd0.. bd0.. | wo gb | aux_W
        * aux_b.  The norm layer's moving statistics live outside the flat vector: mamdr_graph_aux_count / mamdr_graph_bind_aux */
       MAMDR_GRAPH_STAR = 10 };
typedef struct mamdr_graph mamdr_graph;
typedef struct mamdr_graph_config {
    int32_t abi_version;        /* MAMDR_ABI_VERSION */
    int32_t kind;               /* MAMDR_GRAPH_* */
    /* emb_dim = model.user_dim == item_dim == domain_dim.  MAMDR_GRAPH_MLP / _WDL / _DEEPFM: 32, 64, 128 or 256; every other
     * kind: 128 only (MAMDR_EINVAL otherwise, before any device call; mamdr_graph_last_error() names the accepted set) */
    int32_t n_user, n_item, n_domain, emb_dim, max_batch, emb_trainable;
    int32_t n_expert_hidden; int32_t expert_hidden[4];   /* model.hidden_dim: bottom / expert DNN (deep_mtl_ctr.py:26,33,44) */
    int32_t n_tower_hidden;  int32_t tower_hidden[4];    /* model.tower_hidden_dim (:27,34,43) */
    int32_t n_gate_hidden;   int32_t gate_hidden[4];     /* model.gate_dnn_hidden_units (:36,45); unused by shared_bottom */
    int32_t num_experts;                                 /* mmoe (:32) */
    int32_t shared_expert_num, specific_expert_num;      /* ple (:40-41) */
    float dropout, l2_emb, adam_beta1, adam_beta2, adam_eps;
    float l2_linear;                                     /* NFM: deepctr l2_reg_linear (1e-5) on the 1-d linear tables */
    int32_t uncertainty_weight;                          /* single-output towers: the weighted loss of uncertainty_weight/
                                                          * weighted_loss.py:30-43 (one trainable `log_var` per domain, last
                                                          * tensor of the flat vector); evaluation stays unweighted */
    /* MAMDR_GRAPH_STAR only (ABI 19; ignored by every other kind) */
    int32_t star_norm;          /* 0 none, 1 pn (PartitionedNorm), 2 bn (Keras BatchNormalization, momentum 0.99, eps 1e-3) */
    int32_t star_dense;         /* 0 dense (plain kernels), 1 star (StarFCN: shared (.) specific[d]) */
    int32_t auxiliary_dim;      /* 0: no auxiliary network; otherwise = the last hidden width (MAMDR_EINVAL if not) */
} mamdr_graph_config;
const char* mamdr_graph_last_error(void);
int mamdr_graph_create(const mamdr_graph_config* cfg, void* stream, mamdr_graph** out);   /* build_model, deep_mtl_ctr.py:21-67 */
int mamdr_graph_destroy(mamdr_graph* g);
int64_t mamdr_graph_param_count(const mamdr_graph* g);
int32_t mamdr_graph_tensor_count(const mamdr_graph* g);
/* tensor i of the flat vector: Keras-style name ("expert_0/W1", "gate_3/Wg", "tower_3/b0", "head_3/w", ...), element offset
 * and shape (biases and scalars: rows = 1) -- model.trainable_weights of deep_mtl_ctr.py:51 */
int mamdr_graph_tensor_info(const mamdr_graph* g, int32_t i, char* name, int32_t name_cap, int64_t* offset, int64_t* rows,
                            int64_t* cols);
/* the two ranges of the flat vector a step on `domain` trains = trainable_weights of Model(inputs, outputs[domain])
 * (deep_mtl_ctr.py:62-66): the shared block and that task's block; everything else neither moves nor decays */
int mamdr_graph_task_ranges(const mamdr_graph* g, int domain, int64_t* shared_off, int64_t* shared_count, int64_t* task_off,
                            int64_t* task_count);
int mamdr_graph_bind_state(mamdr_graph* g, float* d_params, float* d_adam_m, float* d_adam_v);
int mamdr_graph_optimizer_reset(mamdr_graph* g);
/* epsilon of the following Adam steps: `compile(optimizer='adam')` of deep_mtl_ctr.py:147-148 builds a Keras Adam
 * (epsilon = K.epsilon() = 1e-7) where the shared optimiser of :53-56 is tf.train.AdamOptimizer (1e-8) */
int mamdr_graph_set_adam_eps(mamdr_graph* g, float eps);
int64_t mamdr_graph_optimizer_steps(const mamdr_graph* g);
/* MAMDR_GRAPH_STAR: floats of non-trainable state and the device buffer that holds them (as mamdr_aux_count / mamdr_bind_aux).
 * pn: [mov_mean | mov_var | biased_mean | biased_var] each [D][384], then steps [D], padded to 4 floats -- the step engine's
 * layout; bn: [mov_mean | mov_var] each [384] (initial zeros / ones; updated without zero-debias); none: count 0.  A step or
 * an evaluation before the buffer is bound: MAMDR_ESTATE, nothing launched. */
int64_t mamdr_graph_aux_count(const mamdr_graph* g);
int mamdr_graph_bind_aux(mamdr_graph* g, float* d_aux);
/* kernel launches this process has issued through mamdr_graph_* calls so far (measurement: launches per step) */
int64_t mamdr_graph_launch_count(void);
int64_t mamdr_graph_dropout_steps(const mamdr_graph* g);
/* as mamdr_set_counters: the optimizer's step count (with TF's running beta powers) and the dropout stream's position (ABI 18) */
int mamdr_graph_set_counters(mamdr_graph* g, int64_t optimizer_steps, int64_t dropout_steps);
int mamdr_graph_bind_table(mamdr_graph* g, int seg, const float* d_rows, int64_t n_rows);     /* deep_mtl_ctr.py:98-121 */
int mamdr_graph_bind_domain_data(mamdr_graph* g, int domain, int split, const int32_t* d_uid, const int32_t* d_pid,
                                 const int32_t* d_domain, const float* d_label, int64_t n_rows);
/* n_steps x `domain_model_dict[domain]` train_on_batch: deep_mtl_ctr.py:79-80 (Adam) / :158-172 (per-domain fit).
 * Same batch / permutation / dropout-stream conventions as mamdr_train_steps; MAMDR_OPT_ADAM, MAMDR_OPT_SGD or
 * MAMDR_OPT_ACCUMULATE (after mamdr_graph_bind_accumulator). */
int mamdr_graph_train_steps(mamdr_graph* g, int domain, const int32_t* d_perm, int64_t first_step, int64_t n_steps,
                            int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr, float* d_loss_out);
/* as mamdr_train_steps_n: the pass covers `pass_rows` positions, d_perm lists that many rows of the split (the take / skip
 * sub-datasets of the meta-train / meta-val split, maml.py:300-330, mldg.py:309-325); pass_rows < 0 = the whole split */
int mamdr_graph_train_steps_n(mamdr_graph* g, int domain, const int32_t* d_perm, int64_t pass_rows, int64_t first_step,
                              int64_t n_steps, int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr,
                              float* d_loss_out);
/* MAMDR_OPT_ACCUMULATE steps of the meta wrappers on these towers (maml.py:107-109,196-229; mldg.py; pcgrad.py): dropout off,
 * no update, the step's gradient (every tensor the task's model trains, tables included) added to this flat vector of
 * mamdr_graph_param_count floats; NULL unbinds */
int mamdr_graph_bind_accumulator(mamdr_graph* g, float* d_acc);
/* `domain_model_dict[domain].evaluate(data, steps=n_step)`: deep_mtl_ctr.py:207; outputs as mamdr_eval_domain */
int mamdr_graph_eval_domain(mamdr_graph* g, int domain, int split, int32_t batch, float* d_loss_out, uint32_t* d_hist,
                            float* d_pred_out);

/* Top-K lists, exact ranks and per-query slates from the live weights of the generic-layer engine's SINGLE-OUTPUT towers:
 * MAMDR_GRAPH_NFM, _PNN, _CCPM, _AUTOINT, _MLP, _WDL and _DEEPFM, at every hidden shape and field width that
 * mamdr_graph_create accepts, with frozen or trainable tables, with or without the weighted loss (retrieval, like
 * evaluation, is unweighted).  NO REFERENCE COUNTERPART, as mamdr_recommend.  The argument lists are those of
 * mamdr_recommend, mamdr_recommend_domain, mamdr_rank_domain and mamdr_rank_slates with the graph handle in place of the
 * context, and the header text of those four calls applies as written -- the 64-bit key (order-preserving logit bits << 32)
 * | ~id, ties by ascending id, a NaN logit behind every number, -0 as +0, key 0 = no entry, k in 1 .. 128 with -1 / 0
 * padding, d_scores_all in d_cand order with 0 for an excluded pair, Rank, Score, Live, Position, Order, the link
 * "rank r < k <=> position r of the top-K list", integer-only counting, one stream synchronisation to read offsets back,
 * the MAMDR_EINVAL and MAMDR_ESTATE cases (reported through mamdr_graph_last_error) -- except where listed here:
 * 1. The whole tower runs per pair.  These towers' inputs do not separate into a query term and an item term (inner
 *    products, bi-interaction, convolutions and attention act across the fields), so every (user, item, domain) pair goes
 *    through the engine's inference forward: the pair rows (k_graph_pair_rows), the gather, the tower, and a head that
 *    ends in the key (k_graph_head_keys) instead of the loss.  The logit is formed by the very device function
 *    mamdr_graph_eval_domain's head uses: the retrieval score IS the evaluation score.
 * 2. Bit rule: every forward batch is padded to max_batch rows (rounded up to 64).  On this engine a layer's rounding
 *    depends on the padded row count of the batch (it picks the 32 x 32 tile form, which splits the reduction over four
 *    waves, or the 64 x 64 form), so a remainder batch would score a pair to other bits than a full one.  All forward
 *    batches of these calls therefore run at the full padded height whatever their row count, and a pair's logit is the
 *    same bits in any chunk, at any position, beside any neighbours, across all four calls -- and the bits
 *    mamdr_graph_eval_domain(batch = max_batch) writes to d_pred_out for the same triple in a FULL batch.  Evaluation's
 *    own remainder batch (rows < max_batch, padded to the next 64 only) may round differently; that is unchanged.
 * 3. Chunking: candidates are passed MAMDR_REC_CHUNK at a time (default 16384, rounded up to 64; read at
 *    mamdr_graph_create) in blocks of up to 256 queries; within a pass the pairs are query-major with each query's chunk
 *    padded to a multiple of 64, so a 64-key tile never straddles two queries.  Any chunking gives the same bytes.  The
 *    workspaces (pair rows, keys, per-tile lists, running best, target keys) belong to the handle, grow on demand and are
 *    freed by mamdr_graph_destroy.
 * 4. Reads the state only: parameters, Adam slots, the accumulator, the optimizer and dropout counters and the bound splits
 *    are unchanged.  The activation workspaces the forward overwrites (the activations, AutoInt's token buffers and
 *    attention buffers, the linear-logit column, the label and domain-row columns) are rebuilt by every training and
 *    evaluation call before use.  No loss, histogram or regulariser work is done.
 * MAMDR_ENOTBUILT: shared_bottom / mmoe / ple (one task per domain) and every MAMDR_GRAPH_STAR form (per-domain tensors,
 * BatchNorm state); the message names the kind.  (Added within ABI 19: new entry points only, no structure or existing
 * call changed.) */
int mamdr_graph_recommend(mamdr_graph* g, int32_t n_query, const int32_t* d_uid, const int32_t* d_domain,
                          const int32_t* d_cand, int64_t n_cand,
                          const int64_t* d_excl_off, const int32_t* d_excl_ids,
                          int32_t k, int32_t* d_ids_out, float* d_scores_out, float* d_scores_all);
int mamdr_graph_recommend_domain(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid,
                                 const int32_t* d_cand, int64_t n_cand,
                                 const int64_t* d_excl_off, const int32_t* d_excl_ids,
                                 int32_t k, int32_t* d_ids_out, float* d_scores_out, float* d_scores_all);
int mamdr_graph_rank_domain(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid,
                            const int32_t* d_cand, int64_t n_cand,
                            const int64_t* d_excl_off, const int32_t* d_excl_ids,
                            const int64_t* d_tgt_off, const int32_t* d_tgt_ids,
                            int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out);
int mamdr_graph_rank_slates(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid,
                            const int64_t* d_slate_off, const int32_t* d_slate_ids,
                            float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out);

#ifdef __cplusplus
}
#endif
#endif /* MAMDR_HIP_H */
