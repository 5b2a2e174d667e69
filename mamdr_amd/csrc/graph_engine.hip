// Towers built from GENERIC dense layers: deepctr's SharedBottom / MMOE / PLE under the reference's per-domain
// compiled models (model_zoo/DeepMTLCTR/deep_mtl_ctr.py:21-96).  SURVEY.md section 8 f4: comparison baselines next
// to the hot path -- layer widths, expert counts and gate shapes vary per config (config/*/{shared_bottom,mmoe,ple}.json:
// hidden_dim [512,256,128] ... [256], 2-5 experts, PLE 3-15 specific + 2 shared experts per task), so nothing here is
// specialised to one shape the way step_kernels.hip is to 384-256-128-64.
//
// One training step of task d on a batch (what `domain_model_dict[d].fit` executes per batch, deep_mtl_ctr.py:79-80):
//   gather x = [U[uid] | I[pid] | Dm[dom]]                                   k_graph_gather   (hbm)
//   every expert task d mixes: DNN = per layer  relu(h W + b) * dropout       k_graph_gemm<0>  (mfma, 64x64 tiles)
//   gate_d: DNN, then softmax(q Wg) and the mixture sum_e gate_e expert_e     k_graph_gate_fwd (one workgroup per row)
//   tower_d: DNN;  head: sigmoid(t w + gb), Keras BCE, d loss / d logit       k_graph_head     (one wave per row)
//   backward, layer by layer (dnn_backward): dW = in^T dz (launch_wgrad: queued for the step's flat grid, or k_graph_gemm<2>
//   with the batch rows split over up to 16 workgroups per tile + k_graph_wfinish = the partial products summed in a fixed
//   order and db = column sums), d in = dz W^T times the producer's relu / dropout gate (k_graph_gemm<1>); the mixture's
//   backward (k_graph_gate_bwd) between tower and experts; the first layers add into d x[:, domain columns]
//   domain table: segment sum of d x over the batch's domain ids + 2 l2 Dm    k_graph_domain_grad
//   TF1 Adam (or SGD) on the two ranges of the flat vector task d's model trains: the shared block (domain table +
//   shared experts) and task d's block (its experts, gate, tower, head)       k_graph_adam     (hbm)
// Launch plan (the per-layer launches above remain under MAMDR_GRAPH_NO_DEFER=1):
//   * forward / d-input contractions of fewer than 512 tiles of 64 x 64 run on 32 x 32 tiles with the reduction index
//     split over the workgroup's four waves (gemm_tile32, k_graph_gemm32*: 4 x the workgroups, 128-deep stages);
//   * the weight gradients are QUEUED by the backward pass and contracted in one flat grid at its end
//     (launch_wgrad -> queue_wgrad, flush_wgrads: k_graph_wgrad_multi; the queue's launch aims at WQ_BLOCKS workgroups);
//   * one tail launch (k_graph_tail) finishes them (split sums, bias column sums), runs the narrow contractions
//     (head / gate kernels, PNN's rows, attention projections), the domain table's and the linear table's gradients --
//     and steps every parameter where its gradient is finished (GradSink, open_sink; k_graph_adam -- adam_step -- for the
//     weighted loss, the Star forms, MAMDR_GRAPH_NO_TAIL_OPT=1 and a step whose queue ran full).
// All fp32 (`v_mfma_f32_32x32x2_f32`: exact fp32 products), every reduction in a fixed order (no float atomics).
// Trainable user / item tables (the Amazon configs: no pretraining) sit at the head of the flat vector; their step is
// TF1's dense Adam over every row -- regulariser gradient 2 l2 p + the scatter-add of the batch's row gradients --
// through the table kernels of emb_kernels.hip in their per-step form (k_emb_flag / k_emb_reduce: duplicates summed
// in batch order by the row's first position; k_emb_sweep: one HBM pass over both tables).
//
// Field width: 128 for every tower; MLP / WDL / DeepFM also run at 32, 64 and 256 (cfg.emb_dim = model.user_dim; deepctr.py:95-102
// hands it to SparseFeat): k_graph_gather<E>, k_graph_fm_fwd / _bwd<E>, k_emb_reduce<E> / k_emb_sweep<OPT, E> index by it, the
// first layer's 3 E input columns need no multiple of 64 (gemm_tile32's zero tail, GemmArgs::m_rows), the flat vector is unpadded.
//
// The single-output deepctr towers on the same layers (deepctr.py:33-46; ONE task serves every domain):
//   NFM      f = bi-interaction of the three fields (k_graph_feat_fwd/bwd), DNN over f, + deepctr's linear logit
//   PNN      DNN over [x | the 3 pairwise inner products] (the 3 extra kernel rows ride as a rank-3 epilogue of the GEMM)
//   CCPM     Conv2D (6,1) -> max over the fields -> Conv2D (5,1) centre tap, tanh (k_graph_ccpm_fwd/bwd), DNN over 512 features
//   AutoInt  3 x multi-head self-attention over the 3 field tokens on compact token-major buffers (projections as GEMMs
//            over 3 B token rows, the 3 x 3 attention core in k_graph_att_fwd/bwd), beside the DNN; head over [96 | DNN]
//   Star     star.py:70-96 as a family: norm none / PartitionedNorm / BatchNormalization over x (k_star_colstats, k_star_norm_fwd /
//            _bwd), Dense or StarFCN layers on the kernels of the batch's first-row domain (k_star_eff, k_star_chain), the auxiliary
//            network joined at the head (k_star_join_fwd / _bwd); moving statistics outside the flat vector (mamdr_graph_bind_aux)
//
// Device side: six headers that this file alone includes, in this order (ONE translation unit; the code object lists the
// plain kernels in the order their definitions are read, so the headers are cut along the order the code has always had)
//   graph_gemm.h     GemmArgs / GroupTab, gemm_tile (64 x 64) and gemm_tile32 (32 x 32), k_graph_gemm / _gemm32 and their _group
//                    forms (apply_member)
//   graph_reduce.h   colsum_body and split_sum4 (every column sum / split sum of the engine), k_graph_colsum, k_graph_wfinish /
//                    _group, the queue (WMulti: k_graph_wgrad_multi; WFinish: wfinish_multi_body), GradSink / opt_elem / opt_step4 /
//                    sink1 / sink4 / no_sink, k_graph_dx_reduce, k_graph_small_tn
//   graph_towers.h   k_graph_gather, wave_sum, feat / fm (NFM, PNN, DeepFM) and NFM's linear domain table, CCPM, attention,
//                    k_graph_small_nt / _add_x, gate, head, loss, scale
//   graph_tail.h     the step's end: the domain table's gradient, TailJobs / k_graph_tail, AdamArgs / k_graph_adam
//   graph_star.h     StarNormArgs .. k_star_join_bwd
//   graph_retrieval.h  retrieval from the single-output towers: k_graph_pair_rows, k_graph_head_keys (head_logit of
//                    graph_towers.h with a key ending), k_graph_tile_topk, k_graph_rank_count; last, so the kernels before it
//                    keep their places in the code object
//
// Host side, here (GLAUNCH, the error buffer, the launch_* helpers, then "host side: structure of the tower"):
//   contractions   gemm_args / fwd_args / din_args describe a GemmArgs by role, launch_wgrad takes a weight gradient's operands;
//                  dnn_forward / dnn_backward walk ONE DNN over its layers' operands of this step (LayerOps: layers_of, and
//                  star_layers / star_aux_net for the scratch blocks of k_star_eff / k_star_chain), dnn_forward_group /
//                  dnn_backward_group a group of experts of one shape (same_shape) in single launches per layer
//   towers         one <family>_forward / _backward pair each -- star, single_dnn (MLP / WDL), feat (NFM / PNN / DeepFM), ccpm,
//                  autoint, shared_bottom, gated (MMOE / PLE) -- behind ONE switch per direction: task_forward / task_backward
//   a step         mamdr_graph_train_steps_n: step_ctx, advance_optimizer, open_sink, launch_gather, task_forward, launch_head,
//                  launch_loss, task_backward, finish_grads, star_chain, table_step, adam_step; mamdr_graph_eval_domain shares
//                  step_ctx / launch_gather / task_forward / launch_head / launch_loss.  Nothing in a step allocates.
//   retrieval      mamdr_graph_recommend / _recommend_domain / _rank_domain / _rank_slates: retrieval_host.h's retrieval_call
//                  (shared with the step engine) over GraphRetrieval, this engine's backend: retrieval_kind, grow_retrieval, pair_args,
//                  retrieval_forward (launch_gather + task_forward at the full padded height), cand_pass / list_pass, and the
//                  step engine's k_rec_merge / k_slate_order through their launchers (mamdr_kernels.h)
//   a context      mamdr_graph_create: validate_config, read_switches, layout_one_task (layout_star / layout_single) or
//                  layout_multi_task, alloc_workspace; every device pointer is freed from the record it came from (mamdr_graph::dev)
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mamdr_hip.h"
#include "mamdr_kernels.h"
#include "host_common.h"
#include "retrieval_host.h"
#include "graph_gemm.h"
#include "graph_reduce.h"
#include "graph_towers.h"
#include "graph_tail.h"
#include "graph_star.h"
#include "graph_retrieval.h"

// every kernel launch of this engine goes through here: the count is what tools/graph_bench.py reports as launches per step
static std::atomic<long long> g_graph_launches{0};      // (contexts may be driven from several host threads: lanes)
#define GLAUNCH(...)                      \
    do {                                  \
        ++g_graph_launches;               \
        hipLaunchKernelGGL(__VA_ARGS__);  \
    } while (0)

using namespace mamdr;

namespace {

thread_local ErrBuf g_gerr;     // mamdr_graph_last_error
template <typename... A>
int gfail(int code, const char* fmt, A... a) { return g_gerr.fail(code, fmt, a...); }
#define GHIP(expr) MAMDR_HIP_TRY(g_gerr, expr, #expr)

// rows_pad is a multiple of 64, a workgroup serves 4 waves x 128 / E rows (at most 16)
static void launch_graph_gather(const GatherArgs& a, int emb, hipStream_t s) {
    switch (emb) {
        case 32: GLAUNCH(k_graph_gather<32>, dim3(a.rows_pad / 16), dim3(256), 0, s, a); break;
        case 64: GLAUNCH(k_graph_gather<64>, dim3(a.rows_pad / 8), dim3(256), 0, s, a); break;
        case 256: GLAUNCH(k_graph_gather<256>, dim3(a.rows_pad / 4), dim3(256), 0, s, a); break;
        default: GLAUNCH(k_graph_gather<EMB>, dim3(a.rows_pad / 4), dim3(256), 0, s, a); break;
    }
}
static void launch_colsum(hipStream_t s, const float* dz, int ld, int rows, float* out, int n_valid) {
    GLAUNCH(k_graph_colsum, dim3((n_valid + CS_COLS - 1) / CS_COLS), dim3(256), 0, s, dz, ld, rows, out, n_valid);
}
static void launch_small_tn(hipStream_t s, const float* in, int in_ld, const float* d, int d_ld, int rows, int n_j, int n_e,
                            float* out, float* sum_out = nullptr) {
    GLAUNCH(k_graph_small_tn, dim3((n_j * n_e + CS_COLS - 1) / CS_COLS + (sum_out ? 1 : 0)), dim3(256), 0, s, in, in_ld,
                       d, d_ld, rows, n_j, n_e, out, sum_out);
}
static void launch_lin_domain_grad(hipStream_t s, const float* dlogit, const int32_t* domrow, int rows, const float* w, float two_l2,
                                   int n_domain, float* g) {
    GLAUNCH(k_graph_lin_domain_grad, dim3(n_domain), dim3(256), 0, s, dlogit, domrow, rows, w, two_l2, n_domain, g);
}

// ------------------------------------------------------------------ host side: structure of the tower
constexpr int MAX_LAYERS = 4;   // hidden layers of one DNN (validate_config)
struct Layer {
    int64_t w_off, b_off;
    int in, out;
    uint32_t id;            // dropout stream id = position among all DNN kernels in flat-vector order
};
struct Dnn {
    std::string name;
    std::vector<Layer> layers;
    int in_dim;
};
struct TensorInfo {
    std::string name;
    int64_t off, rows, cols;
};
struct Task {
    std::vector<int> mix;   // indices into dnns: the experts this task mixes (specific ones first, then the shared ones)
    int gate = -1;          // gate DNN
    int64_t wg_off = 0;
    int tower = -1;
    int64_t head_w = 0, head_gb = 0;
    int64_t blk_off = 0, blk_end = 0;
    // column plan of the activation / gradient workspaces for this task's path
    std::vector<std::vector<int>> col;  // col[dnn index in `path`][layer] -> first column of that layer's output
    std::vector<int> path;              // dnns on the path: mix..., gate, tower
    int g_col = 0, m_col = 0, n_cols = 0;
};
}  // namespace

struct mamdr_graph {
    mamdr_graph_config cfg;
    hipStream_t stream = nullptr;
    std::vector<Dnn> dnns;
    std::vector<Task> tasks;
    std::vector<TensorInfo> tensors;
    int64_t n_params = 0, dm_off = 0, shared_end = 0;
    bool gated = false;
    int n_h = 0;                // expert width
    // single-output towers of the deepctr family on the same layers (NFM, PNN): ONE task serves every domain
    bool single = false;
    bool has_lin = false;       // NFM / CCPM / AutoInt: the three 1-d linear tables (deepctr get_linear_logit)
    int f_col = 0;              // interaction features: NFM 128 columns, PNN 3 (+ 1 pad), CCPM 512
    int in_col = 0;             // what the single tower's DNN reads: the features (NFM, CCPM) or x (0)
    int xe_col = -1;            // PNN: the inner products that ride in the first layer's epilogue (-1: none)
    int cg_col = 0;             // CCPM: 64 columns of the gradient workspace for the rows' shares of the 48 conv gradients
    int64_t conv_off = 0;       // CCPM: [w1 6x4 | b1 | w2 4x4 | b2]
    // AutoInt: three attention layers on compact token-major buffers (row 3 b + t = field t of batch row b)
    int64_t att_w[3] = {0, 0, 0};
    int top_col = 0;            // [attention output 96 | last DNN layer] contiguous in the activation workspace (head input)
    float *xt = nullptr, *dxt = nullptr;
    float *attP[3] = {nullptr, nullptr, nullptr}, *attdP[3] = {nullptr, nullptr, nullptr};
    float *attA[3] = {nullptr, nullptr, nullptr}, *attY[3] = {nullptr, nullptr, nullptr}, *attdY[3] = {nullptr, nullptr, nullptr};
    int64_t lin_d_off = 0;      // NFM: 1-d linear table of the domain feature (behind the global bias)
    int64_t lv_off = -1;        // weighted loss: `log_var` [n_domain], the last tensor (-1: plain loss)
    int64_t lin_u_off = 0, lin_i_off = 0;       // ... of the user / item features (trainable tables only)
    float *extra = nullptr, *glin_u = nullptr, *glin_i = nullptr;
    // Star forms (MAMDR_GRAPH_STAR): cfg.star_norm / star_dense / auxiliary_dim
    bool star = false;
    int xn_col = 0, a_col = 0, jtop_col = 0;       // normalised input (0 = x itself without a norm), auxiliary output, h_n + a
    int64_t norm_off[4] = {0, 0, 0, 0};             // pn: gamma_shared beta_shared gamma_spec beta_spec; bn: gamma beta
    StarTab stab;                                   // the step's effective tensors (k_star_eff / k_star_chain)
    int seg_k[4] = {-1, -1, -1, -1}, seg_b[4] = {-1, -1, -1, -1}, seg_aw = -1, seg_ab = -1;     // their segments
    float *eff = nullptr, *deff = nullptr, *pnv = nullptr;
    double* spart = nullptr;
    float* aux = nullptr;                           // moving statistics (mamdr_graph_bind_aux)
    int64_t aux_count = 0;
    float* E(int seg) const { return eff + 4 * (size_t)stab.first4[seg]; }
    float* DE(int seg) const { return deff + 4 * (size_t)stab.first4[seg]; }
    // bound state
    float *params = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    float* accum = nullptr;     // meta-gradient accumulator of MAMDR_OPT_ACCUMULATE steps (mamdr_graph_bind_accumulator)
    const float *user_tab = nullptr, *item_tab = nullptr;
    std::vector<SplitData> data;
    int64_t adam_t = 0;
    float b1p = 1.f, b2p = 1.f;
    uint32_t global_step = 0;
    // workspace
    DevAllocs dev;              // every device allocation of this context: what mamdr_graph_destroy frees
    int rows_pad_max = 0, ld = 0;
    float *act = nullptr, *dact = nullptr, *grad = nullptr, *dlogit = nullptr, *rowloss = nullptr, *y = nullptr;
    float* wpart = nullptr;     // split-K partial products of one weight gradient (launch_wgrad)
    size_t wpart_floats = 0;
    float* dxpart = nullptr;    // the members' products of a group's first-layer d x (dnn_backward_group)
    size_t dxpart_floats = 0;
    // the step's weight gradients, queued by the backward pass and run in ONE pair of launches at its end (flush_wgrads);
    // MAMDR_GRAPH_NO_DEFER=1: a pair of launches per layer, where the backward pass meets it (A/B)
    struct WProb { const float* A; int lda; const float* B; int ldb; float* out; int M, N, rows; const float* dz; float* db; };
    std::vector<WProb> wq;
    struct TnProb { const float* in; int in_ld; const float* d; int d_ld; int rows, n_j, n_e; float* out; float* sum_out; };
    std::vector<TnProb> tq;     // narrow contractions (k_graph_small_tn's problems) that ride in the queue's second launch
    bool defer_w = true;
    // the optimiser step inside the tail launch (every gradient of a step's two ranges is finished there): no k_graph_adam.
    // Off for the weighted loss (k_graph_loss writes d / d log_var) and under MAMDR_GRAPH_NO_TAIL_OPT=1 (A/B; same bits)
    bool tail_opt = true;
    GradSink sink;              // this step's sink (p null: gradients are stored, k_graph_adam follows)
    int32_t* domrow = nullptr;
    float *thresholds = nullptr, *frozen_sumsq = nullptr, *sumsq_partials = nullptr, *eval_acc = nullptr;
    // trainable tables
    int emb = EMB;              // width of the three tables' rows (cfg.emb_dim; other than 128 for mlp / wdl / deepfm only)
    bool tables = false;
    int64_t table_floats = 0;
    int32_t *urow = nullptr, *irow = nullptr, *map_u = nullptr, *map_i = nullptr, *hasdup_u = nullptr, *hasdup_i = nullptr;
    float *gbuf_u = nullptr, *gbuf_i = nullptr;
    float* G(int64_t off) const { return grad + (off - table_floats); }      // gradient of the flat vector's element `off`
    // retrieval (graph_retrieval.h): the pair rows and keys of one forward batch [rows_pad_max], the per-tile lists and the
    // running best of a block of queries, the target / slate keys of a call.  Allocated on first use, grown on demand
    int rec_chunk = 16384;      // candidates per pass (MAMDR_REC_CHUNK)
    int32_t *ret_uid = nullptr, *ret_pid = nullptr, *ret_dom = nullptr, *ret_rowq = nullptr;
    float* ret_label = nullptr;
    unsigned long long *ret_keys = nullptr, *ret_best = nullptr;
    GrowBuf<unsigned long long> ret_part, ret_tkey;
    // the x columns of the gradient workspace that a first layer on x fills: the domain columns alone while the tables are
    // frozen (n 0: all of them)
    int dx_first() const { return tables ? 0 : 2 * emb; }
    int dx_n() const { return tables ? 0 : emb; }
};

namespace {

// the queue's launch splits the batch rows until it has about this many workgroups (256 and 1024 are within 1 - 4 % either
// way: profiles/r04f_graph_tail_launch.txt)
constexpr int WQ_BLOCKS = 512;

struct StepCtx {
    int rows, rp;               // rows of the batch, padded to 64
    bool train;
    uint32_t seed, step, drop_thresh;
    float keep_scale;
    bool use_dropout;
};
// what one step of the optimiser applies: the same rule in the tail launch's sink, the table step and k_graph_adam
struct OptStep {
    int optimizer;
    float alpha, omb1, omb2, eps;
    float* slot_m;              // Adam's m, or the accumulator of MAMDR_OPT_ACCUMULATE
};

// ---- a layer as ONE step uses it: kernel, bias and where their gradients go.  The flat vector and its gradient for every
// tower (layers_of); a StarFCN layer reads the scratch block of k_star_eff and leaves its gradients in that of k_star_chain
struct LayerOps {
    const float *w, *b;
    float *gw, *gb;
    int in, out;
    uint32_t id;
};
struct DnnOps {
    LayerOps l[MAX_LAYERS];
    int n;
};
DnnOps layers_of(const mamdr_graph* g, const Dnn& d) {
    DnnOps o;
    o.n = (int)d.layers.size();
    for (int l = 0; l < o.n; ++l) {
        const Layer& L = d.layers[l];
        o.l[l] = LayerOps{g->params + L.w_off, g->params + L.b_off, g->G(L.w_off), g->G(L.b_off), L.in, L.out, L.id};
    }
    return o;
}

// ---- one description per kind of contraction (GemmArgs: what k_graph_gemm* read)
GemmArgs gemm_args(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int K) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A;
    a.lda = lda;
    a.B = B;
    a.ldb = ldb;
    a.C = C;
    a.ldc = ldc;
    a.K = K;
    return a;
}
// layer forward on the activation workspace: columns dst = relu(columns src . W + b) * dropout
GemmArgs fwd_args(const mamdr_graph* g, const LayerOps& L, int src_col, int dst_col, const StepCtx& sc) {
    GemmArgs a = gemm_args(g->act + src_col, g->ld, L.w, L.out, g->act + dst_col, g->ld, L.in);
    a.bias = L.b;
    a.relu = 1;
    a.use_dropout = sc.use_dropout ? 1 : 0;
    a.drop_key = dropout_layer_key(sc.seed, sc.step, L.id);
    a.drop_thresh = sc.drop_thresh;
    a.keep_scale = sc.keep_scale;
    a.n_cols = L.out;
    return a;
}
// d input on the gradient workspace: columns dst (+)= columns dz (n_dz wide) . W^T, times the relu / dropout gate of the
// activation columns `gate_col` when >= 0
GemmArgs din_args(const mamdr_graph* g, int dz_col, int n_dz, const float* W, int dst_col, int gate_col, bool acc, const StepCtx& sc) {
    GemmArgs a = gemm_args(g->dact + dz_col, g->ld, W, n_dz, g->dact + dst_col, g->ld, n_dz);
    a.gate_scale = sc.keep_scale;
    if (gate_col >= 0) {
        a.gate_y = g->act + gate_col;
        a.gate_ld = g->ld;
    }
    a.accumulate = acc ? 1 : 0;
    return a;
}

int64_t add_tensor(mamdr_graph* g, const std::string& name, int64_t rows, int64_t cols) {
    const int64_t off = g->n_params;
    g->tensors.push_back(TensorInfo{name, off, rows, cols});
    g->n_params = (off + rows * cols + 3) & ~(int64_t)3;
    return off;
}
int add_dnn(mamdr_graph* g, const std::string& name, int in_dim, const int32_t* hidden, int n_hidden, uint32_t& next_id) {
    Dnn d;
    d.name = name;
    d.in_dim = in_dim;
    int in = in_dim;
    for (int l = 0; l < n_hidden; ++l) {
        Layer L;
        L.in = in;
        L.out = hidden[l];
        L.w_off = add_tensor(g, name + "/W" + std::to_string(l), in, hidden[l]);
        L.b_off = add_tensor(g, name + "/b" + std::to_string(l), 1, hidden[l]);
        L.id = next_id++;
        d.layers.push_back(L);
        in = hidden[l];
    }
    g->dnns.push_back(d);
    return (int)g->dnns.size() - 1;
}

// dW[M x N] = A[rows x M]^T . B[rows x N], the rows split over up to 16 workgroups per tile when the tiles alone leave
// most of the 256 CUs idle (a 384 x 512 kernel is 48 tiles); the partial products meet in k_graph_wfinish, which also
// carries the layer's bias gradient (column sums of `dz` into `db`, skipped when db is null)
// `end`: the flush that ends a step's backward pass -- its tail launch also carries the domain table's gradient and the 1-d
// linear domain table's (null: a queue ran full in mid-step)
void flush_wgrads(mamdr_graph* g, const StepCtx* end = nullptr) {
    const int n = (int)g->wq.size();
    if (!n && g->tq.empty() && !end) return;
    int tiles = 0;
    for (const auto& q : g->wq) tiles += ((q.M + GT - 1) / GT) * (q.N / GT);
    int S = 1;
    while (S < 16 && tiles * S < WQ_BLOCKS) S *= 2;
    int split[MAX_WQ];
    for (;; S /= 2) {       // per problem: the largest power of two <= S that leaves every split >= 4 k-tiles; all must fit
        size_t need = 0;
        for (int p = 0; p < n; ++p) {
            const auto& q = g->wq[p];
            const int nkt = q.rows / GK;
            int sp = 1;
            while (sp < S && nkt % (2 * sp) == 0 && nkt / (2 * sp) >= 4) sp *= 2;
            split[p] = sp;
            if (sp > 1) need += (size_t)sp * q.M * q.N;
        }
        if (need <= g->wpart_floats || S == 1) break;
    }
    WMulti m;
    WFinish f;
    memset(&m, 0, sizeof(m));
    memset(&f, 0, sizeof(f));
    m.n = f.n = n;
    size_t used = 0;
    int nb = 0, nf = 0;
    for (int p = 0; p < n; ++p) {
        const auto& q = g->wq[p];
        const int sp = split[p];
        float* part = g->wpart + used;
        if (sp > 1) used += (size_t)sp * q.M * q.N;
        m.first[p] = nb;
        m.A[p] = q.A;
        m.lda[p] = q.lda;
        m.B[p] = q.B;
        m.ldb[p] = q.ldb;
        m.C[p] = sp > 1 ? part : q.out;
        m.N[p] = q.N;
        m.tx[p] = q.N / GT;
        m.ty[p] = (q.M + GT - 1) / GT;
        m.K[p] = q.rows / sp;
        m.mn[p] = q.M * q.N;
        m.M[p] = q.M;
        nb += m.tx[p] * m.ty[p] * sp;
        f.first[p] = nf;
        f.part[p] = sp > 1 ? part : q.out;
        f.out[p] = q.out;
        f.dz[p] = q.dz;
        f.db[p] = q.db;
        f.split[p] = sp;
        // (a gradient that the contraction wrote in place still has to pass through the optimiser when the sink steps)
        f.nb_red[p] = (sp > 1 || g->sink.p) ? (q.M * q.N / 4 + 255) / 256 : 0;
        f.N[p] = q.db ? q.N : 0;
        f.rows[p] = q.rows;
        f.ld[p] = g->ld;
        f.mn[p] = q.M * q.N;
        nf += f.nb_red[p] + (q.db ? (q.N + CS_COLS - 1) / CS_COLS : 0);
    }
    m.first[n] = nb;
    f.first[n] = nf;
    if (nb) GLAUNCH(k_graph_wgrad_multi, dim3(nb), dim3(256), 0, g->stream, m);
    TailJobs j;
    memset(&j, 0, sizeof(j));
    int nt = 0;
    j.n_tn = (int)g->tq.size();
    for (int q = 0; q < j.n_tn; ++q) {
        const auto& t = g->tq[q];
        j.tn_first[q] = nt;
        j.in[q] = t.in;
        j.in_ld[q] = t.in_ld;
        j.d[q] = t.d;
        j.d_ld[q] = t.d_ld;
        j.rows[q] = t.rows;
        j.n_j[q] = t.n_j;
        j.n_e[q] = t.n_e;
        j.out[q] = t.out;
        j.sum_out[q] = t.sum_out;
        nt += (t.n_j * t.n_e + CS_COLS - 1) / CS_COLS + (t.sum_out ? 1 : 0);
    }
    j.tn_first[j.n_tn] = nt;
    j.dg_first = nt;
    if (end) {
        j.dg_blocks = (g->emb / CS_COLS) * g->cfg.n_domain;
        j.dg_emb = g->emb;
        j.dx = g->dact;
        j.ld = g->ld;
        j.x_col = 2 * g->emb;
        j.domrow = g->domrow;
        j.dg_rows = end->rows;
        j.dm = g->params + g->dm_off;
        j.two_l2 = 2.0f * g->cfg.l2_emb;
        j.g_dm = g->G(g->dm_off);
        if (g->has_lin) {
            j.lin_blocks = g->cfg.n_domain;
            j.lin_dlogit = g->dlogit;
            j.lin_w = g->params + g->lin_d_off;
            j.lin_two_l2 = 2.0f * g->cfg.l2_linear;
            j.lin_g = g->G(g->lin_d_off);
        }
    }
    j.sink = g->sink;
    const int nblk = nf + nt + j.dg_blocks + j.lin_blocks;
    if (nblk) GLAUNCH(k_graph_tail, dim3(nblk), dim3(256), 0, g->stream, f, j);
    g->wq.clear();
    g->tq.clear();
}
// a narrow contraction of the backward pass: queued beside the weight gradients (their outputs are gradients too)
void small_tn(mamdr_graph* g, const float* in, int in_ld, const float* d, int d_ld, int rows, int n_j, int n_e, float* out,
              float* sum_out = nullptr) {
    if (!g->defer_w) {
        launch_small_tn(g->stream, in, in_ld, d, d_ld, rows, n_j, n_e, out, sum_out);
        return;
    }
    if ((int)g->tq.size() == MAX_TQ) {
        g->sink.p = nullptr;
        flush_wgrads(g);
    }
    g->tq.push_back(mamdr_graph::TnProb{in, in_ld, d, d_ld, rows, n_j, n_e, out, sum_out});
}
void queue_wgrad(mamdr_graph* g, const float* A, int lda, const float* B, int ldb, float* out, int M, int N, int rows,
                 const float* dz, float* db) {
    if ((int)g->wq.size() == MAX_WQ) {      // a flush in mid-step must not step parameters the backward pass still reads:
        g->sink.p = nullptr;                // this step's gradients are stored and k_graph_adam runs at its end
        flush_wgrads(g);
    }
    g->wq.push_back(mamdr_graph::WProb{A, lda, B, ldb, out, M, N, rows, dz, db});
}
// a weight gradient launched on its own: the ways its batch rows are split -- doubled while the grid stays under 256 workgroups,
// a split keeps a whole number (at least 4) of staged tiles and the partial products (`floats` per split) fit the workspace
int pick_split(const mamdr_graph* g, int tiles, int rows, size_t floats) {
    const int nkt = rows / GK;
    int split = 1;
    while (split < 16 && tiles * split < 256 && nkt % (2 * split) == 0 && nkt / (2 * split) >= 4 &&
           (size_t)(2 * split) * floats <= g->wpart_floats)
        split *= 2;
    return split;
}
// weight gradient out[M x N] = A^T B over `rows` rows (+ db = column sums of dz): queued, or a pair of launches right here
void launch_wgrad(mamdr_graph* g, const float* A, int lda, const float* B, int ldb, float* out, int M, int N, int rows,
                  const float* dz, float* db) {
    if (g->defer_w) {
        queue_wgrad(g, A, lda, B, ldb, out, M, N, rows, dz, db);
        return;
    }
    const int ty = (M + GT - 1) / GT, split = pick_split(g, ty * (N / GT), rows, (size_t)M * N);
    GemmArgs a = gemm_args(A, lda, B, ldb, split > 1 ? g->wpart : out, N, rows / split);
    a.zstride = (size_t)M * N;
    a.m_rows = M;
    GLAUNCH(k_graph_gemm<2>, dim3(N / GT, ty, split), dim3(256), 0, g->stream, a);
    const int64_t n4 = (int64_t)M * N / 4;
    const int nb_red = split > 1 ? (int)((n4 + 255) / 256) : 0, nb_cs = db ? (N + CS_COLS - 1) / CS_COLS : 0;
    if (nb_red + nb_cs)
        GLAUNCH(k_graph_wfinish, dim3(nb_red + nb_cs), dim3(256), 0, g->stream, g->wpart, split, a.zstride, n4, out,
                           nb_red, dz, g->ld, rows, db, N);
}

// 32 x 32 tiles (gemm_tile32) while the 64 x 64 ones would leave CUs idle or nearly so; MAMDR_GRAPH_TILE32_BELOW=<tiles> (0: never)
// (process-wide like the environment it comes from; re-read at EVERY mamdr_graph_create -- round 6: a value set by one context's
// environment used to stay in force for every later context of the process, and a test that set MAMDR_GRAPH_TILE32_BELOW=0
// changed the rounding of every generic-layer run after it in the same session)
constexpr int TILE32_BELOW_DEFAULT = 512;
std::atomic<int> g_tile32_below{TILE32_BELOW_DEFAULT};
// (a width that is no multiple of 64 -- d x of a first layer on 32- or 96-wide fields -- has no 64 x 64 tiling at all)
inline bool use_tile32(int M, int N, int n_group = 1) {
    return N % T32 == 0 && (N % GT != 0 || (M / GT) * (N / GT) * n_group < g_tile32_below.load(std::memory_order_relaxed));
}
void launch_gemm(int mode, const GemmArgs& a, int M, int N, hipStream_t s) {
    const dim3 grid(N / GT, M / GT), block(256);
    if (mode != 2 && use_tile32(M, N)) {
        const dim3 g32(N / T32, M / T32);
        if (mode == 0) GLAUNCH(k_graph_gemm32<0>, g32, block, 0, s, a);
        else GLAUNCH(k_graph_gemm32<1>, g32, block, 0, s, a);
        return;
    }
    if (mode == 0) GLAUNCH(k_graph_gemm<0>, grid, block, 0, s, a);
    else if (mode == 1) GLAUNCH(k_graph_gemm<1>, grid, block, 0, s, a);
    else GLAUNCH(k_graph_gemm<2>, grid, block, 0, s, a);
}
// the grouped forms of modes 0 / 1: `n` problems of one [sc.rp x N] shape in one grid
template <int MODE>
void launch_gemm_group(mamdr_graph* g, const GemmArgs& a, const GroupTab& t, int N, const StepCtx& sc) {
    if (use_tile32(sc.rp, N, t.n))
        GLAUNCH(k_graph_gemm32_group<MODE>, dim3(N / T32, sc.rp / T32, t.n), dim3(256), 0, g->stream, a, t);
    else
        GLAUNCH(k_graph_gemm_group<MODE>, dim3(N / GT, sc.rp / GT, t.n), dim3(256), 0, g->stream, a, t);
}

// forward of one DNN: input columns `in_col` of the activation workspace, layer l's output at cols[l]; xe_col >= 0 (PNN):
// the three inner products there times rows in..in + 2 of the first kernel
void dnn_forward(mamdr_graph* g, const DnnOps& d, const int* cols, int in_col, const StepCtx& sc, int xe_col = -1) {
    for (int l = 0; l < d.n; ++l) {
        const LayerOps& L = d.l[l];
        GemmArgs a = fwd_args(g, L, l == 0 ? in_col : cols[l - 1], cols[l], sc);
        if (l == 0 && xe_col >= 0) {
            a.xe = g->act + xe_col;
            a.xe_ld = g->ld;
            a.we = L.w + (size_t)L.in * L.out;
            a.n_xe = 3;
        }
        launch_gemm(0, a, sc.rp, L.out, g->stream);
    }
}
// backward of one DNN whose last layer's d z already sits in the gradient workspace.  The input's gradient goes to
// `din_col` of the gradient workspace: times the gate of `in_gate_col` (the producer's relu / dropout) when >= 0;
// accumulated when `din_acc`; only columns [din_first, din_first + din_n) of the input when din_n > 0 (first layers
// on x: the domain columns alone matter while the tables are frozen); skipped when din_col < 0.
void dnn_backward(mamdr_graph* g, const DnnOps& d, const int* cols, int in_col, int din_col, int in_gate_col, bool din_acc,
                  int din_first, int din_n, const StepCtx& sc) {
    for (int l = d.n - 1; l >= 0; --l) {
        const LayerOps& L = d.l[l];
        launch_wgrad(g, g->act + (l == 0 ? in_col : cols[l - 1]), g->ld, g->dact + cols[l], g->ld, L.gw, L.in, L.out, sc.rp,
                     g->dact + cols[l], L.gb);
        if (l > 0) {
            launch_gemm(1, din_args(g, cols[l], L.out, L.w, cols[l - 1], cols[l - 1], false, sc), sc.rp, L.in, g->stream);
        } else if (din_col >= 0) {
            const int first = din_n > 0 ? din_first : 0, n = din_n > 0 ? din_n : L.in;
            launch_gemm(1, din_args(g, cols[0], L.out, L.w + (size_t)first * L.out, din_col + first,
                                    in_gate_col >= 0 ? in_gate_col + first : -1, din_acc, sc), sc.rp, n, g->stream);
        }
    }
}

// ---- a group of DNNs of ONE shape on ONE input (the experts a task mixes), layer by layer in single launches.  The
// members' operands are offsets (GroupTab) from the workspaces' and the flat vector's bases; cols[e] = member e's columns
GroupTab group_tab(int n) {      // n members, every offset zero
    GroupTab t;
    memset(&t, 0, sizeof(t));
    t.n = n;
    return t;
}
bool same_shape(const mamdr_graph* g, const std::vector<int>& ids) {
    if (ids.size() < 2 || ids.size() > (size_t)MAX_GROUP) return false;
    const Dnn& d0 = g->dnns[ids[0]];
    for (int id : ids) {
        const Dnn& d = g->dnns[id];
        if (d.in_dim != d0.in_dim || d.layers.size() != d0.layers.size()) return false;
        for (size_t l = 0; l < d.layers.size(); ++l)
            if (d.layers[l].in != d0.layers[l].in || d.layers[l].out != d0.layers[l].out) return false;
    }
    return true;
}
void dnn_forward_group(mamdr_graph* g, const std::vector<int>& ids, const std::vector<int>* cols, int in_col, const StepCtx& sc) {
    const Dnn& d0 = g->dnns[ids[0]];
    const int n = (int)ids.size();
    for (size_t l = 0; l < d0.layers.size(); ++l) {
        const Layer& L0 = d0.layers[l];
        const GemmArgs a = fwd_args(g, LayerOps{g->params, g->params, nullptr, nullptr, L0.in, L0.out, 0}, 0, 0, sc);
        GroupTab t = group_tab(n);
        for (int e = 0; e < n; ++e) {
            const Layer& L = g->dnns[ids[e]].layers[l];
            t.a_off[e] = l == 0 ? in_col : cols[e][l - 1];
            t.b_off[e] = L.w_off;
            t.c_off[e] = cols[e][l];
            t.bias_off[e] = L.b_off;
            t.drop_key[e] = dropout_layer_key(sc.seed, sc.step, L.id);
        }
        launch_gemm_group<0>(g, a, t, L0.out, sc);
    }
}
// backward of the group (every member's last-layer d z sits in the gradient workspace): weight / bias gradients and the
// inner layers' d inputs in grouped launches; the FIRST layers' d x adds up over the members and stays one launch each
void dnn_backward_group(mamdr_graph* g, const std::vector<int>& ids, const std::vector<int>* cols, int in_col, bool din_acc,
                        int din_first, int din_n, const StepCtx& sc) {
    const Dnn& d0 = g->dnns[ids[0]];
    const int n = (int)ids.size();
    for (int l = (int)d0.layers.size() - 1; l >= 0; --l) {
        const Layer& L0 = d0.layers[l];
        const int M = L0.in, N = L0.out;
        if (g->defer_w) {
            for (int e = 0; e < n; ++e) {
                const Layer& L = g->dnns[ids[e]].layers[l];
                queue_wgrad(g, g->act + (l == 0 ? in_col : cols[e][l - 1]), g->ld, g->dact + cols[e][l], g->ld, g->G(L.w_off), M, N,
                            sc.rp, g->dact + cols[e][l], g->G(L.b_off));
            }
        } else {    // dW_e = in_e^T dz_e, db_e = column sums of dz_e
            const int split = pick_split(g, (M / GT) * (N / GT) * n, sc.rp, (size_t)n * M * N);
            GemmArgs a = gemm_args(g->act, g->ld, g->dact, g->ld, split > 1 ? g->wpart : g->grad, N, sc.rp / split);
            a.zstride = (size_t)M * N;
            GroupTab t = group_tab(n), f = group_tab(n);
            t.tiles_y = M / GT;
            for (int e = 0; e < n; ++e) {
                const Layer& L = g->dnns[ids[e]].layers[l];
                t.a_off[e] = l == 0 ? in_col : cols[e][l - 1];
                t.b_off[e] = cols[e][l];
                t.c_off[e] = split > 1 ? (int64_t)e * split * M * N : L.w_off - g->table_floats;
                f.a_off[e] = cols[e][l];
                f.c_off[e] = L.w_off - g->table_floats;
                f.bias_off[e] = L.b_off - g->table_floats;
            }
            GLAUNCH(k_graph_gemm_group<2>, dim3(N / GT, (M / GT) * n, split), dim3(256), 0, g->stream, a, t);
            const int64_t n4 = (int64_t)M * N / 4;
            const int nb_red = split > 1 ? (int)((n4 + 255) / 256) : 0, nb_cs = (N + CS_COLS - 1) / CS_COLS;
            GLAUNCH(k_graph_wfinish_group, dim3(nb_red + nb_cs, n), dim3(256), 0, g->stream, g->wpart, split,
                               a.zstride, n4, g->grad, nb_red, g->dact, g->ld, sc.rp, g->grad, N, f);
        }
        GroupTab t = group_tab(n);
        if (l > 0) {    // d in_e = dz_e W_e^T through the producer's relu / dropout gate
            const GemmArgs a = din_args(g, 0, N, g->params, 0, 0, false, sc);
            for (int e = 0; e < n; ++e) {
                t.a_off[e] = cols[e][l];
                t.b_off[e] = g->dnns[ids[e]].layers[l].w_off;
                t.c_off[e] = cols[e][l - 1];
                t.gate_off[e] = cols[e][l - 1];
            }
            launch_gemm_group<1>(g, a, t, M, sc);
            continue;
        }
        // d x = sum_e dz_e W_e[first : first + nn]^T
        const int first = din_n > 0 ? din_first : 0, nn = din_n > 0 ? din_n : M;
        GemmArgs a = din_args(g, 0, N, g->params + (size_t)first * N, in_col + first, -1, false, sc);
        for (int e = 0; e < n; ++e) {
            t.a_off[e] = cols[e][0];
            t.b_off[e] = g->dnns[ids[e]].layers[0].w_off;
        }
        // every member's product as a launch-mate of the others (n x the tiles), summed in member order.  The products fit
        // dxpart: the one caller (gated_backward) hands over dx_first() / dx_n(), so nn = XDIM with trainable tables (the experts
        // read x: in = XDIM) and EMB without, n <= the largest mix and sc.rp <= rows_pad_max -- alloc_workspace's very product
        const size_t stride = (size_t)sc.rp * nn;
        a.C = g->dxpart;
        a.ldc = nn;
        for (int e = 0; e < n; ++e) t.c_off[e] = (int64_t)e * stride;
        launch_gemm_group<1>(g, a, t, nn, sc);
        const int64_t tot = (int64_t)sc.rp * (nn / 4);
        GLAUNCH(k_graph_dx_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, g->stream, g->dxpart, n, stride, sc.rp,
                nn / 4, g->dact + in_col + first, g->ld, din_acc ? 1 : 0);
    }
}

// ================================================================== the towers, one pair of functions per family.
// forward: from the gathered x to the head's input, -> its first column; backward: from the head's d input (k_graph_head)
// down to d x, every weight gradient through launch_wgrad / small_tn / queue_wgrad.  (Star stands first and launch_feat
// names its forward kernels before its backward ones: the device code object lists a kernel template's instances in the
// order the host code first names them, and this order keeps it comparable byte for byte across host-only changes)

// ---- Star forms: the norm over x, Dense or StarFCN layers on the kernels of the batch's first-row domain, the auxiliary
// network joined at the head.  The layers and the auxiliary net run on dnn_forward / dnn_backward: a StarFCN layer and the
// auxiliary net read the scratch block of k_star_eff and leave their gradients in the scratch block k_star_chain splits
DnnOps star_layers(const mamdr_graph* g, const Dnn& d) {
    DnnOps o = layers_of(g, d);
    for (int l = 0; l < o.n; ++l)
        if (g->seg_k[l] >= 0) {
            o.l[l].w = g->E(g->seg_k[l]);
            o.l[l].b = g->E(g->seg_b[l]);
            o.l[l].gw = g->DE(g->seg_k[l]);
            o.l[l].gb = g->DE(g->seg_b[l]);
        }
    return o;
}
DnnOps star_aux_net(const mamdr_graph* g) {     // a = relu(xn . aux_W[d] + aux_b[d]): one layer on the NORMALISED input (star.py:76-82)
    DnnOps o;
    o.n = 1;
    o.l[0] = LayerOps{g->E(g->seg_aw), g->E(g->seg_ab), g->DE(g->seg_aw), g->DE(g->seg_ab), XDIM, g->cfg.auxiliary_dim, 0};
    return o;
}
void fill_star_norm(const mamdr_graph* g, const StepCtx& sc, StarNormArgs& na) {
    memset(&na, 0, sizeof(na));
    na.x = g->act;
    na.xn = g->act + g->xn_col;
    na.ld = g->ld;
    na.dxn = g->dact + g->xn_col;
    na.dx = g->dact;
    na.rows = sc.rows;
    na.rows_pad = sc.rp;
    na.n_chunks = (sc.rows + SN_ROWS - 1) / SN_ROWS;
    na.n_domain = g->cfg.n_domain;
    na.norm = g->cfg.star_norm;
    na.train = sc.train ? 1 : 0;
    na.domrow = g->domrow;
    na.part = g->spart;
    na.pnv = g->pnv;
    na.gs = g->params + g->norm_off[0];
    na.bs = g->params + g->norm_off[1];
    na.g_gs = g->G(g->norm_off[0]);
    na.g_bs = g->G(g->norm_off[1]);
    if (g->cfg.star_norm == 1) {
        na.gd = g->params + g->norm_off[2];
        na.bd = g->params + g->norm_off[3];
        na.g_gd = g->G(g->norm_off[2]);
        na.g_bd = g->G(g->norm_off[3]);
    }
    na.aux = g->aux;
}
int star_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    const int A = g->cfg.auxiliary_dim;
    if (g->stab.n)
        GLAUNCH(k_star_eff, dim3((g->stab.first4[g->stab.n] + 255) / 256), dim3(256), 0, g->stream, g->stab, g->params, g->domrow,
                g->eff);
    if (g->cfg.star_norm) {
        StarNormArgs na;
        fill_star_norm(g, sc, na);
        if (sc.train) GLAUNCH(k_star_colstats<false>, dim3(na.n_chunks), dim3(XDIM), 0, g->stream, na);
        GLAUNCH(k_star_norm_fwd, dim3((sc.rp + SN_ROWS - 1) / SN_ROWS), dim3(XDIM), 0, g->stream, na);
    }
    dnn_forward(g, star_layers(g, g->dnns[t.tower]), t.col[0].data(), g->xn_col, sc);
    if (!A) return t.col[0].back();
    dnn_forward(g, star_aux_net(g), &g->a_col, g->xn_col, sc);
    GLAUNCH(k_star_join_fwd, dim3((sc.rp * (A / 4) + 255) / 256), dim3(256), 0, g->stream, g->act, g->ld, t.col[0].back(), g->a_col,
            g->jtop_col, A, sc.rp);
    return g->jtop_col;
}
void star_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    const int A = g->cfg.auxiliary_dim;
    if (A)
        GLAUNCH(k_star_join_bwd, dim3((sc.rp * (A / 4) + 255) / 256), dim3(256), 0, g->stream, g->act, g->dact, g->ld,
                t.col[0].back(), g->a_col, g->jtop_col, A, sc.rp);
    // without a norm d xn IS d x: the domain columns alone matter while the tables are frozen
    const bool part = !g->cfg.star_norm && !g->tables;
    const int first = part ? 2 * EMB : 0, nx = part ? EMB : XDIM;
    dnn_backward(g, star_layers(g, g->dnns[t.tower]), t.col[0].data(), g->xn_col, g->xn_col, -1, false, first, nx, sc);
    if (A) dnn_backward(g, star_aux_net(g), &g->a_col, g->xn_col, g->xn_col, -1, true, first, nx, sc);     // d xn += dz_a . aux_W[d]^T
    if (g->cfg.star_norm) {
        StarNormArgs na;
        fill_star_norm(g, sc, na);
        GLAUNCH(k_star_colstats<true>, dim3(na.n_chunks), dim3(XDIM), 0, g->stream, na);
        GLAUNCH(k_star_norm_bwd, dim3((sc.rp + SN_ROWS - 1) / SN_ROWS), dim3(XDIM), 0, g->stream, na);
    }
}

void fill_gate(const mamdr_graph* g, const Task& t, const StepCtx& sc, GateArgs& ga) {
    memset(&ga, 0, sizeof(ga));
    ga.act = g->act;
    ga.dact = g->dact;
    ga.ld = g->ld;
    const size_t gi = t.mix.size();                 // position of the gate DNN in `path`
    const Dnn& gd = g->dnns[t.gate];
    ga.q_col = t.col[gi].back();
    ga.n_q = gd.layers.back().out;
    ga.wg = g->params + t.wg_off;
    ga.n_e = (int)t.mix.size();
    for (size_t e = 0; e < t.mix.size(); ++e) ga.e_col[e] = t.col[e].back();
    ga.n_h = g->n_h;
    ga.g_col = t.g_col;
    ga.m_col = t.m_col;
    ga.rows_pad = sc.rp;
    ga.gate_scale = sc.keep_scale;
}
// the interaction features: NFM's bi-interaction, PNN's inner products, DeepFM's FM term (at its field width)
void launch_feat(mamdr_graph* g, const Task& t, const StepCtx& sc, bool bwd) {
    FeatArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.act = g->act;
    fa.dact = g->dact;
    fa.ld = g->ld;
    fa.f_col = g->f_col;
    fa.rows_pad = sc.rp;
    fa.kind = g->cfg.kind == MAMDR_GRAPH_NFM ? 0 : (g->cfg.kind == MAMDR_GRAPH_DEEPFM ? 2 : 1);
    fa.extra = g->extra;
    fa.dlogit = g->dlogit;
    fa.dx_all = g->tables ? 1 : 0;
    const Layer& L0 = g->dnns[t.tower].layers[0];
    fa.w_ip = g->params + L0.w_off + (size_t)L0.in * L0.out;
    fa.z_col = t.col[0][0];
    fa.n_out = L0.out;
    if (!bwd) {
        switch (g->emb) {       // (other than 128: DeepFM alone)
            case 32: GLAUNCH(k_graph_fm_fwd<32>, dim3(sc.rp / 32), dim3(256), 0, g->stream, fa); break;
            case 64: GLAUNCH(k_graph_fm_fwd<64>, dim3(sc.rp / 16), dim3(256), 0, g->stream, fa); break;
            case 256: GLAUNCH(k_graph_fm_fwd<256>, dim3(sc.rp / 4), dim3(256), 0, g->stream, fa); break;
            default: GLAUNCH(k_graph_feat_fwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, fa); break;
        }
        return;
    }
    switch (g->emb) {
        case 32: GLAUNCH(k_graph_fm_bwd<32>, dim3(sc.rp / 32), dim3(256), 0, g->stream, fa); break;
        case 64: GLAUNCH(k_graph_fm_bwd<64>, dim3(sc.rp / 16), dim3(256), 0, g->stream, fa); break;
        case 256: GLAUNCH(k_graph_fm_bwd<256>, dim3(sc.rp / 4), dim3(256), 0, g->stream, fa); break;
        default: GLAUNCH(k_graph_feat_bwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, fa); break;
    }
}
void fill_ccpm(const mamdr_graph* g, const StepCtx& sc, CcpmArgs& ca) {
    memset(&ca, 0, sizeof(ca));
    ca.act = g->act;
    ca.dact = g->dact;
    ca.ld = g->ld;
    ca.f_col = g->f_col;
    ca.cg_col = g->cg_col;
    ca.rows_pad = sc.rp;
    ca.dx_all = g->tables ? 1 : 0;
    ca.conv = g->params + g->conv_off;
}
void fill_att(const mamdr_graph* g, int l, const StepCtx& sc, bool bwd, AttArgs& aa) {
    memset(&aa, 0, sizeof(aa));
    aa.P = g->attP[l];
    aa.A = g->attA[l];
    aa.Y = g->attY[l];
    aa.rows_pad = sc.rp;
    if (bwd) {
        aa.dY = g->attdY[l];
        aa.dP = g->attdP[l];
    }
    if (l == 2 && bwd) {
        aa.dtop = g->dact + g->top_col;
        aa.dtop_ld = g->ld;
    } else if (l == 2) {
        aa.top = g->act + g->top_col;
        aa.top_ld = g->ld;
    }
}

// ---- the single towers' DNN on g->in_col (x, or the interaction features), PNN's epilogue included: MLP / WDL as they are
int single_dnn_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    dnn_forward(g, layers_of(g, g->dnns[t.tower]), t.col[0].data(), g->in_col, sc, g->xe_col);
    return t.col[0].back();
}
void single_dnn_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    const bool on_x = g->in_col == 0;       // as any first layer on x; otherwise d features, whole
    dnn_backward(g, layers_of(g, g->dnns[t.tower]), t.col[0].data(), g->in_col, g->in_col, -1, false, on_x ? g->dx_first() : 0,
                 on_x ? g->dx_n() : 0, sc);
}
// ---- NFM / PNN / DeepFM: the feature kernel beside that DNN
int feat_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    launch_feat(g, t, sc, false);
    return single_dnn_forward(g, t, sc);
}
void feat_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    single_dnn_backward(g, t, sc);
    if (g->xe_col >= 0) {       // PNN: rows in..in + 2 of the first kernel against the inner products
        const Layer& L0 = g->dnns[t.tower].layers[0];
        small_tn(g, g->act + g->xe_col, g->ld, g->dact + t.col[0][0], g->ld, sc.rp, 3, L0.out, g->G(L0.w_off + (int64_t)L0.in * L0.out));
    }
    launch_feat(g, t, sc, true);            // d x from d features (NFM) / the inner products / the FM term
}
// ---- CCPM: the convolutions' kernel, the DNN over its 512 features
int ccpm_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    CcpmArgs ca;
    fill_ccpm(g, sc, ca);
    GLAUNCH(k_graph_ccpm_fwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, ca);
    return single_dnn_forward(g, t, sc);
}
void ccpm_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    // d features from the first layer; the convolutions' backward per row; their 48 gradients summed over the batch
    single_dnn_backward(g, t, sc);
    CcpmArgs ca;
    fill_ccpm(g, sc, ca);
    GLAUNCH(k_graph_ccpm_bwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, ca);
    if (g->defer_w)     // the 48 column sums as a queue entry without a contraction (its end = the bias-gradient workgroups)
        queue_wgrad(g, nullptr, 0, nullptr, 0, nullptr, 0, 48, sc.rp, g->dact + g->cg_col, g->G(g->conv_off));
    else
        launch_colsum(g->stream, g->dact + g->cg_col, g->ld, sc.rp, g->G(g->conv_off), 48);
}
// ---- AutoInt: the attention stack on the token-major buffers [3 rows_pad][d], beside the DNN on x
int autoint_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    for (int l = 0; l < 3; ++l) {
        const int d_in = l == 0 ? EMB : ATT_OUT;
        GemmArgs a = gemm_args(l == 0 ? g->xt : g->attY[l - 1], d_in, g->params + g->att_w[l], ATT_P, g->attP[l], ATT_P, d_in);
        a.n_cols = ATT_P;
        launch_gemm(0, a, 3 * sc.rp, ATT_P, g->stream);
        AttArgs aa;
        fill_att(g, l, sc, false, aa);
        GLAUNCH(k_graph_att_fwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, aa);
    }
    single_dnn_forward(g, t, sc);
    return g->top_col;
}
void autoint_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    single_dnn_backward(g, t, sc);
    for (int l = 2; l >= 0; --l) {          // from the head's d [attention output] down to d x
        const int d_in = l == 0 ? EMB : ATT_OUT;
        AttArgs aa;
        fill_att(g, l, sc, true, aa);
        GLAUNCH(k_graph_att_bwd, dim3(sc.rp / 4), dim3(256), 0, g->stream, aa);
        const float *xin = l == 0 ? g->xt : g->attY[l - 1], *W = g->params + g->att_w[l];
        float* dxin = l == 0 ? g->dxt : g->attdY[l - 1];
        // dW = X^T dP over the 3 B token rows; d X = dP W^T
        if (l == 0) launch_wgrad(g, xin, d_in, g->attdP[l], ATT_P, g->G(g->att_w[l]), d_in, ATT_P, 3 * sc.rp, nullptr, nullptr);
        else small_tn(g, xin, d_in, g->attdP[l], ATT_P, 3 * sc.rp, d_in, ATT_P, g->G(g->att_w[l]));
        if (l == 0 || use_tile32(3 * sc.rp, d_in))
            launch_gemm(1, gemm_args(g->attdP[l], ATT_P, W, ATT_P, dxin, d_in, ATT_P), 3 * sc.rp, d_in, g->stream);
        else
            GLAUNCH(k_graph_small_nt, dim3((3 * sc.rp * d_in + 255) / 256), dim3(256), 0, g->stream, g->attdP[l], ATT_P, W, d_in,
                    3 * sc.rp, dxin);
    }
    const int first = g->tables ? 0 : 2 * EMB, n = g->tables ? XDIM : EMB;
    GLAUNCH(k_graph_add_x, dim3((sc.rp * n + 255) / 256), dim3(256), 0, g->stream, g->dact, g->ld, g->dxt, sc.rp, first, n);
}
// ---- shared-bottom: one expert, the tower on its last layer
int shared_bottom_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    dnn_forward(g, layers_of(g, g->dnns[t.mix[0]]), t.col[0].data(), 0, sc);
    dnn_forward(g, layers_of(g, g->dnns[t.tower]), t.col[1].data(), t.col[0].back(), sc);
    return t.col[1].back();
}
void shared_bottom_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    // the tower's input IS the bottom's output: its gradient passes through the bottom's last relu / dropout gate
    const int b = t.col[0].back();
    dnn_backward(g, layers_of(g, g->dnns[t.tower]), t.col[1].data(), b, b, b, false, 0, 0, sc);
    dnn_backward(g, layers_of(g, g->dnns[t.mix[0]]), t.col[0].data(), 0, 0, -1, false, g->dx_first(), g->dx_n(), sc);
}
// ---- MMOE / PLE: the experts (one grid per layer when they share a shape), the gate and its mixture, the tower.  The x
// columns of the gradient workspace collect d x from every first layer: the gate's overwrites, the experts' add
int gated_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    const size_t gi = t.mix.size(), ti = gi + 1;
    if (same_shape(g, t.mix))
        dnn_forward_group(g, t.mix, t.col.data(), 0, sc);
    else
        for (size_t e = 0; e < gi; ++e) dnn_forward(g, layers_of(g, g->dnns[t.mix[e]]), t.col[e].data(), 0, sc);
    dnn_forward(g, layers_of(g, g->dnns[t.gate]), t.col[gi].data(), 0, sc);
    GateArgs ga;
    fill_gate(g, t, sc, ga);
    GLAUNCH(k_graph_gate_fwd, dim3(sc.rp), dim3(256), 0, g->stream, ga);
    dnn_forward(g, layers_of(g, g->dnns[t.tower]), t.col[ti].data(), t.m_col, sc);
    return t.col[ti].back();
}
void gated_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    const size_t gi = t.mix.size(), ti = gi + 1;
    const int dx_first = g->dx_first(), dx_n = g->dx_n();
    dnn_backward(g, layers_of(g, g->dnns[t.tower]), t.col[ti].data(), t.m_col, t.m_col, -1, false, 0, 0, sc);
    GateArgs ga;
    fill_gate(g, t, sc, ga);
    GLAUNCH(k_graph_gate_bwd, dim3(sc.rp), dim3(256), 0, g->stream, ga);
    small_tn(g, g->act + ga.q_col, g->ld, g->dact + t.g_col, g->ld, sc.rp, ga.n_q, ga.n_e, g->G(t.wg_off));
    dnn_backward(g, layers_of(g, g->dnns[t.gate]), t.col[gi].data(), 0, 0, -1, false, dx_first, dx_n, sc);
    if (same_shape(g, t.mix))
        dnn_backward_group(g, t.mix, t.col.data(), 0, true, dx_first, dx_n, sc);
    else
        for (size_t e = 0; e < gi; ++e) dnn_backward(g, layers_of(g, g->dnns[t.mix[e]]), t.col[e].data(), 0, 0, -1, true, dx_first, dx_n, sc);
}
// ---- one dispatch per direction
int task_forward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    switch (g->cfg.kind) {
        case MAMDR_GRAPH_SHARED_BOTTOM: return shared_bottom_forward(g, t, sc);
        case MAMDR_GRAPH_MMOE:
        case MAMDR_GRAPH_PLE: return gated_forward(g, t, sc);
        case MAMDR_GRAPH_NFM:
        case MAMDR_GRAPH_PNN:
        case MAMDR_GRAPH_DEEPFM: return feat_forward(g, t, sc);
        case MAMDR_GRAPH_CCPM: return ccpm_forward(g, t, sc);
        case MAMDR_GRAPH_AUTOINT: return autoint_forward(g, t, sc);
        case MAMDR_GRAPH_MLP:
        case MAMDR_GRAPH_WDL: return single_dnn_forward(g, t, sc);      // (WDL's linear part rides in `extra`)
        default: return star_forward(g, t, sc);
    }
}
void task_backward(mamdr_graph* g, const Task& t, const StepCtx& sc) {
    switch (g->cfg.kind) {
        case MAMDR_GRAPH_SHARED_BOTTOM: shared_bottom_backward(g, t, sc); break;
        case MAMDR_GRAPH_MMOE:
        case MAMDR_GRAPH_PLE: gated_backward(g, t, sc); break;
        case MAMDR_GRAPH_NFM:
        case MAMDR_GRAPH_PNN:
        case MAMDR_GRAPH_DEEPFM: feat_backward(g, t, sc); break;
        case MAMDR_GRAPH_CCPM: ccpm_backward(g, t, sc); break;
        case MAMDR_GRAPH_AUTOINT: autoint_backward(g, t, sc); break;
        case MAMDR_GRAPH_MLP:
        case MAMDR_GRAPH_WDL: single_dnn_backward(g, t, sc); break;
        default: star_backward(g, t, sc); break;
    }
    // the 1-d linear domain table's gradient: the last launch of every tower that has one (in the tail launch when deferred)
    if (g->has_lin && !g->defer_w)
        launch_lin_domain_grad(g->stream, g->dlogit, g->domrow, sc.rows, g->params + g->lin_d_off, 2.0f * g->cfg.l2_linear,
                               g->cfg.n_domain, g->G(g->lin_d_off));
}

int check(const mamdr_graph* g) {
    if (!g) return gfail(MAMDR_EINVAL, "null graph context");
    return MAMDR_OK;
}
// trainable tables: the regulariser term of a reported loss needs their current sums of squares
void refresh_sumsq(mamdr_graph* g) {
    launch_sumsq(g->params, (int64_t)g->cfg.n_user * g->emb, g->sumsq_partials, g->frozen_sumsq + 0, g->stream);
    launch_sumsq(g->params + (size_t)g->cfg.n_user * g->emb, (int64_t)g->cfg.n_item * g->emb, g->sumsq_partials, g->frozen_sumsq + 1,
                 g->stream);
    if (g->has_lin) {
        launch_sumsq(g->params + g->lin_u_off, g->cfg.n_user, g->sumsq_partials, g->frozen_sumsq + 2, g->stream);
        launch_sumsq(g->params + g->lin_i_off, g->cfg.n_item, g->sumsq_partials, g->frozen_sumsq + 3, g->stream);
    }
}
int ready(const mamdr_graph* g) {
    if (!g->params) return gfail(MAMDR_ESTATE, "mamdr_graph_bind_state has not been called");
    if (!g->tables && (!g->user_tab || !g->item_tab)) return gfail(MAMDR_ESTATE, "frozen user / item tables are not bound");
    if (g->aux_count && !g->aux) return gfail(MAMDR_ESTATE, "mamdr_graph_bind_aux has not been called (the norm layer's moving statistics)");
    return MAMDR_OK;
}
SplitData* split_of(mamdr_graph* g, int domain, int split) {
    if (domain < 0 || domain >= g->cfg.n_domain || split < 0 || split > 2) return nullptr;
    return &g->data[(size_t)domain * 3 + split];
}

// ================================================================== the parts of a step, in the order the step loop runs them
// rows [row_base, row_base + batch) of a pass over `n_rows` rows; the dropout of a training step that is no meta pass
// (MAMDR_OPT_ACCUMULATE runs in learning phase 0: maml.py:107-109)
StepCtx step_ctx(const mamdr_graph* g, int64_t n_rows, int64_t row_base, int batch, bool train, uint32_t seed, bool dropout) {
    StepCtx sc;
    memset(&sc, 0, sizeof(sc));
    sc.rows = (int)((n_rows - row_base) < batch ? (n_rows - row_base) : batch);
    sc.rp = (sc.rows + GT - 1) / GT * GT;
    sc.train = train;
    sc.keep_scale = 1.0f;
    if (!train) return sc;
    const float rate = g->cfg.dropout;
    const double thr = (double)rate * 4294967296.0;
    sc.seed = seed;
    sc.step = g->global_step;
    sc.drop_thresh = thr >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(int64_t)thr;
    sc.use_dropout = rate > 0.f && dropout;
    if (sc.use_dropout) sc.keep_scale = (float)(1.0 / (1.0 - (double)rate));
    return sc;
}
// ONE optimizer object for all domain models: its beta powers advance with every Adam step, whichever task it trains
OptStep advance_optimizer(mamdr_graph* g, int optimizer, float lr) {
    OptStep o{optimizer, lr, 1.0f - g->cfg.adam_beta1, 1.0f - g->cfg.adam_beta2, g->cfg.adam_eps,
              optimizer == MAMDR_OPT_ACCUMULATE ? g->accum : g->adam_m};
    if (optimizer == MAMDR_OPT_ADAM) {
        g->adam_t += 1;
        g->b1p *= g->cfg.adam_beta1;
        g->b2p *= g->cfg.adam_beta2;
        o.alpha = lr * sqrtf(1.0f - g->b2p) / (1.0f - g->b1p);
    }
    return o;
}
// the tail launch steps every parameter where its gradient is finished -- unless the step has gradients that the tail does
// not finish: the weighted loss (k_graph_loss writes d / d log_var), the Star forms (their weight gradients land in scratch
// and pass through k_star_chain), the per-layer plan.  Closed (p null): gradients are stored, k_graph_adam steps the vector
void open_sink(mamdr_graph* g, const OptStep& o) {
    g->sink.p = nullptr;
    if (!(g->defer_w && g->tail_opt && g->lv_off < 0 && !g->star)) return;
    g->sink.g_base = g->grad;
    g->sink.p = g->params + g->table_floats;
    g->sink.m = o.slot_m + g->table_floats;
    g->sink.v = g->adam_v + g->table_floats;
    g->sink.optimizer = o.optimizer;
    g->sink.alpha = o.alpha;
    g->sink.omb1 = o.omb1;
    g->sink.omb2 = o.omb2;
    g->sink.eps = o.eps;
}
void launch_gather(mamdr_graph* g, const SplitData& d, const int32_t* perm, int64_t row_base, const StepCtx& sc) {
    GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.user_tab = g->user_tab;
    ga.item_tab = g->item_tab;
    ga.dm = g->params + g->dm_off;
    ga.uid = d.uid;
    ga.pid = d.pid;
    ga.dom = d.dom;
    ga.perm = perm;
    ga.label = d.label;
    ga.row_base = row_base;
    ga.n_rows_split = d.n;
    ga.rows = sc.rows;
    ga.rows_pad = sc.rp;
    ga.n_user = g->cfg.n_user;
    ga.n_item = g->cfg.n_item;
    ga.n_domain = g->cfg.n_domain;
    ga.x = g->act;
    ga.ld = g->ld;
    ga.domrow = g->domrow;
    ga.y = g->y;
    ga.xt = g->xt;
    if (g->extra) {
        ga.extra = g->extra;
        ga.lin_d = g->params + g->lin_d_off;
        if (g->tables) {
            ga.lin_u = g->params + g->lin_u_off;
            ga.lin_i = g->params + g->lin_i_off;
        }
    }
    if (g->tables && sc.train) {
        ga.urow = g->urow;
        ga.irow = g->irow;
        ga.map_u = g->map_u;
        ga.map_i = g->map_i;
    }
    launch_graph_gather(ga, g->emb, g->stream);
}
// the head over columns [t_col, ...) of the activation workspace (AutoInt: [attention output | last DNN layer]).  A training
// step leaves d logit and the head's d input; evaluation counts the histogram and writes the predictions.  -> its width
HeadArgs head_args(const mamdr_graph* g, const Task& t, const StepCtx& sc, int t_col) {
    const bool autoint = g->cfg.kind == MAMDR_GRAPH_AUTOINT;
    HeadArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.act = g->act;
    ha.dact = g->dact;
    ha.ld = g->ld;
    ha.t_col = t_col;
    ha.n_plain = autoint ? 3 * ATT_OUT : 0;
    ha.n_t = g->dnns[t.tower].layers.back().out + ha.n_plain;
    ha.w = g->params + t.head_w;
    ha.gb = g->params + t.head_gb;
    ha.y = g->y;
    ha.rows = sc.rows;
    ha.rows_pad = sc.rp;
    ha.dlogit = g->dlogit;
    ha.rowloss = g->rowloss;
    ha.extra = g->extra;
    ha.train = sc.train ? 1 : 0;
    ha.gate_scale = sc.keep_scale;
    return ha;
}
int launch_head(mamdr_graph* g, const Task& t, const StepCtx& sc, int t_col, uint32_t* hist, float* pred_out) {
    HeadArgs ha = head_args(g, t, sc, t_col);
    if (sc.train && g->lv_off >= 0) {
        ha.log_var = g->params + g->lv_off;
        ha.domrow = g->domrow;
    }
    if (!sc.train) {
        ha.thresholds = g->thresholds;
        ha.hist = hist;
        ha.pred_out = pred_out;
    }
    GLAUNCH(k_graph_head, dim3(sc.rp / 4), dim3(256), 0, g->stream, ha);
    return ha.n_t;
}
// batch loss into out[0] (accumulate: added to it); the weighted loss of a training step also leaves d / d log_var
void launch_loss(mamdr_graph* g, const StepCtx& sc, float* out, bool accumulate) {
    const bool weighted = sc.train && g->lv_off >= 0;
    GLAUNCH(k_graph_loss, dim3(1), dim3(256), 0, g->stream, g->rowloss, sc.rows, g->params + g->dm_off, g->cfg.n_domain * g->emb,
            g->cfg.l2_emb, g->frozen_sumsq, out, accumulate ? 1 : 0, g->extra ? g->params + g->lin_d_off : nullptr, g->cfg.n_domain,
            g->cfg.l2_linear, weighted ? g->params + g->lv_off : nullptr, g->domrow, weighted ? g->G(g->lv_off) : nullptr,
            g->cfg.n_domain);
}
// every layer's dW / db of the step, the narrow contractions, the domain table's and the linear table's gradients: one pair
// of launches (the tail steps the parameters when the sink is open); per-layer plan: the domain table's gradient alone
void finish_grads(mamdr_graph* g, const StepCtx& sc) {
    if (g->defer_w)
        flush_wgrads(g, &sc);
    else
        GLAUNCH(k_graph_domain_grad, dim3(g->emb / CS_COLS, g->cfg.n_domain), dim3(256), 0, g->stream, g->dact, g->ld, 2 * g->emb,
                g->domrow, sc.rows, g->params + g->dm_off, 2.0f * g->cfg.l2_emb, g->G(g->dm_off), g->emb);
}
// Star: scratch gradients -> the flat gradient (zeros for the other domains' slices)
void star_chain(mamdr_graph* g) {
    if (g->stab.n)
        GLAUNCH(k_star_chain, dim3((g->stab.first4[g->stab.n] + 255) / 256), dim3(256), 0, g->stream, g->stab, g->params, g->domrow,
                g->deff, g->grad - g->table_floats, g->cfg.n_domain);
}
// TF1's dense step over both trainable tables: g = 2 l2 p + scatter-add of d x[:, user | item columns]; their 1-d linear
// tables by the same rule from d loss / d logit
void table_step(mamdr_graph* g, const StepCtx& sc, const OptStep& o) {
    EmbStepArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.p = g->params;
    ea.m = o.slot_m;
    ea.v = g->adam_v;
    ea.dxe = g->dact;
    ea.dx_ld = g->ld;
    ea.dlogit = g->dlogit;
    ea.rows = sc.rows;
    ea.opt.optimizer = o.optimizer;
    ea.opt.alpha = o.alpha;
    ea.opt.omb1 = o.omb1;
    ea.opt.omb2 = o.omb2;
    ea.opt.eps = o.eps;
    ea.opt.two_l2 = 2.0f * g->cfg.l2_emb;
    const int n_rows[2] = {g->cfg.n_user, g->cfg.n_item};
    int32_t *const brow[2] = {g->urow, g->irow}, *const map[2] = {g->map_u, g->map_i}, *const hasdup[2] = {g->hasdup_u, g->hasdup_i};
    float *const gbuf[2] = {g->gbuf_u, g->gbuf_i}, *const glin[2] = {g->glin_u, g->glin_i};
    const int64_t lin_off[2] = {g->lin_u_off, g->lin_i_off};
    if (g->has_lin) ea.two_l2_lin = 2.0f * g->cfg.l2_linear;
    for (int k = 0; k < 2; ++k) {
        ea.t[k].n_rows = n_rows[k];
        ea.t[k].brow = brow[k];
        ea.t[k].map = map[k];
        ea.t[k].gbuf = gbuf[k];
        ea.t[k].hasdup = hasdup[k];
        ea.t[k].dx_off = k * g->emb;
        if (g->has_lin) {
            ea.t[k].lin_p = g->params + lin_off[k];
            ea.t[k].lin_m = o.slot_m + lin_off[k];
            ea.t[k].lin_v = g->adam_v + lin_off[k];
            ea.t[k].glin = glin[k];
        }
    }
    launch_emb_reduce(ea, g->stream, g->emb);
    launch_emb_sweep(ea, g->stream, g->emb);
    if (g->has_lin) launch_lin_sweep(ea, g->stream);      // (reads the row maps, then resets them)
}
// the optimiser on the two ranges this task's model trains, in one launch
void adam_step(mamdr_graph* g, const Task& t, const OptStep& o) {
    AdamArgs aa;
    aa.p = g->params;
    aa.m = o.slot_m;
    aa.v = g->adam_v;
    aa.g = g->grad - g->table_floats;       // G(off) = grad + off - table_floats
    aa.off4[0] = g->dm_off / 4;
    aa.n4[0] = (g->shared_end - g->dm_off) / 4;
    aa.off4[1] = t.blk_off / 4;
    aa.n4[1] = (t.blk_end - t.blk_off) / 4;
    aa.optimizer = o.optimizer;
    aa.alpha = o.alpha;
    aa.omb1 = o.omb1;
    aa.omb2 = o.omb2;
    aa.eps = o.eps;
    const int64_t n4 = aa.n4[0] + aa.n4[1];
    if (n4 > 0) GLAUNCH(k_graph_adam, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g->stream, aa);
}

// ================================================================== mamdr_graph_create in three steps
// experts every task shares / owns (multi-task towers)
void expert_counts(const mamdr_graph_config& cfg, int& n_shared, int& n_specific) {
    n_shared = cfg.kind == MAMDR_GRAPH_MMOE ? cfg.num_experts : (cfg.kind == MAMDR_GRAPH_PLE ? cfg.shared_expert_num : 1);
    n_specific = cfg.kind == MAMDR_GRAPH_PLE ? cfg.specific_expert_num : 0;
}
int validate_config(const mamdr_graph_config* cfg) {
    if (cfg->abi_version != MAMDR_ABI_VERSION) return gfail(MAMDR_EINVAL, "abi_version %d != %d", cfg->abi_version, MAMDR_ABI_VERSION);
    if (cfg->n_user <= 0 || cfg->n_item <= 0 || cfg->n_domain <= 0 || cfg->max_batch <= 0) return gfail(MAMDR_EINVAL, "bad sizes");
    if (cfg->emb_trainable && cfg->max_batch > 16384) return gfail(MAMDR_EINVAL, "trainable tables: max_batch <= 16384");
    if (cfg->kind < MAMDR_GRAPH_SHARED_BOTTOM || cfg->kind > MAMDR_GRAPH_STAR)
        return gfail(MAMDR_EINVAL, "unknown graph tower kind %d", cfg->kind);
    {       // the field width: gather, FM term and table updates are instantiated for the accepted widths alone
        const bool any_width = cfg->kind == MAMDR_GRAPH_MLP || cfg->kind == MAMDR_GRAPH_WDL || cfg->kind == MAMDR_GRAPH_DEEPFM;
        const int e = cfg->emb_dim;
        if (e != EMB && !(any_width && (e == 32 || e == 64 || e == 256)))
            return gfail(MAMDR_EINVAL, "emb_dim %d: the mlp / wdl / deepfm towers take emb_dim 32, 64, 128 or 256, every other tower "
                                       "emb_dim 128 only", e);
    }
    if (!(cfg->dropout >= 0.f && cfg->dropout < 1.f)) return gfail(MAMDR_EINVAL, "dropout rate must be in [0,1)");
    const bool single = cfg->kind >= MAMDR_GRAPH_NFM;
    const bool gated = cfg->kind == MAMDR_GRAPH_MMOE || cfg->kind == MAMDR_GRAPH_PLE;
    auto depth_ok = [](int n) { return n >= 1 && n <= MAX_LAYERS; };
    if (!depth_ok(cfg->n_expert_hidden) || (!single && !depth_ok(cfg->n_tower_hidden)) || (gated && !depth_ok(cfg->n_gate_hidden)))
        return gfail(MAMDR_EINVAL, "hidden_dim%s need 1..4 layers", single ? "" : (gated ? " / tower_hidden_dim / gate_dnn_hidden_units"
                                                                                           : " / tower_hidden_dim"));
    auto widths_ok = [](const int32_t* h, int n) {
        for (int i = 0; i < n; ++i)
            if (h[i] <= 0 || h[i] % 64) return false;
        return true;
    };
    if (!widths_ok(cfg->expert_hidden, cfg->n_expert_hidden) || (!single && !widths_ok(cfg->tower_hidden, cfg->n_tower_hidden)) ||
        (gated && !widths_ok(cfg->gate_hidden, cfg->n_gate_hidden)))
        return gfail(MAMDR_EINVAL, "layer widths must be multiples of 64 (the reference's configs use 64 ... 512)");
    int n_shared, n_specific;
    expert_counts(*cfg, n_shared, n_specific);
    if (!single && (n_shared < 0 || n_specific < 0 || n_shared + n_specific < 1 || n_shared + n_specific > MAX_MIX))
        return gfail(MAMDR_EINVAL, "a task must mix 1..%d experts", MAX_MIX);
    if (!single && cfg->uncertainty_weight)     // uncertainty_weight.py:41-45 wraps model.inputs / outputs[0] of ONE Keras model
        return gfail(MAMDR_ENOTBUILT, "the weighted loss wraps a single-output tower (the multi-task towers are a dict of models)");
    if (cfg->kind == MAMDR_GRAPH_STAR) {
        if (cfg->star_norm < 0 || cfg->star_norm > 2) return gfail(MAMDR_EINVAL, "star_norm %d: 0 none, 1 pn, 2 bn", cfg->star_norm);
        if (cfg->star_dense < 0 || cfg->star_dense > 1) return gfail(MAMDR_EINVAL, "star_dense %d: 0 dense, 1 star", cfg->star_dense);
        const int last = cfg->expert_hidden[cfg->n_expert_hidden - 1];
        if (cfg->auxiliary_dim < 0 || (cfg->auxiliary_dim > 0 && cfg->auxiliary_dim != last))
            return gfail(MAMDR_EINVAL, "auxiliary_dim %d != the last hidden width %d (star.py:92-93 adds the two outputs)",
                         cfg->auxiliary_dim, last);
        if (cfg->uncertainty_weight) return gfail(MAMDR_ENOTBUILT, "the weighted loss is not built for the Star forms");
    }
    return MAMDR_OK;
}

// ---- the flat vector behind the tables and the domain table, and the column plan of the workspaces: one layout per family.
// -> columns the widest task needs
// the single towers' DNN as ONE block: every kernel, then every bias (oracle/fmnets.py, oracle/star.py param_names);
// `extra_rows` more rows in the first kernel (PNN's inner products)
Dnn& add_dnn_wb(mamdr_graph* g, const char* w, const char* b, int in_dim, int extra_rows) {
    Dnn d;
    d.name = "dnn";
    d.in_dim = in_dim;
    int in = in_dim;
    for (int l = 0; l < g->cfg.n_expert_hidden; ++l) {
        Layer L;
        L.in = in;
        L.out = g->cfg.expert_hidden[l];
        L.w_off = add_tensor(g, w + std::to_string(l), l == 0 ? in + extra_rows : in, L.out);
        L.b_off = 0;
        L.id = (uint32_t)l;
        d.layers.push_back(L);
        in = L.out;
    }
    for (size_t l = 0; l < d.layers.size(); ++l) d.layers[l].b_off = add_tensor(g, b + std::to_string(l), 1, d.layers[l].out);
    g->dnns.push_back(d);
    return g->dnns.back();
}
// the columns of one DNN's layer outputs, from column c on
void plan_cols(Task& t, const Dnn& d, int& c) {
    std::vector<int> cols;
    for (const Layer& L : d.layers) {
        cols.push_back(c);
        c += L.out;
    }
    t.col.push_back(cols);
}
// oracle/star.param_names generalised: domain_emb | Ws0.. bs0.. (or W0.. b0..) | the norm's tensors | Wd0.. bd0.. | wo | gb |
// aux_W aux_b -- the reference's Star filter (emb, kernel_shared, bias_shared) selects a prefix
int layout_star(mamdr_graph* g) {
    const mamdr_graph_config& cfg = g->cfg;
    Task& t = g->tasks[0];
    const bool sf = cfg.star_dense == 1;
    const int D = cfg.n_domain, A = cfg.auxiliary_dim;
    const Dnn& d = add_dnn_wb(g, sf ? "Ws" : "W", sf ? "bs" : "b", XDIM, 0);
    if (cfg.star_norm == 1) {
        g->norm_off[0] = add_tensor(g, "pn_gamma_shared", 1, XDIM);
        g->norm_off[1] = add_tensor(g, "pn_beta_shared", 1, XDIM);
        g->norm_off[2] = add_tensor(g, "pn_gamma_spec", D, XDIM);
        g->norm_off[3] = add_tensor(g, "pn_beta_spec", D, XDIM);
        g->aux_count = ((int64_t)4 * D * XDIM + D + 3) & ~(int64_t)3;
    } else if (cfg.star_norm == 2) {
        g->norm_off[0] = add_tensor(g, "bn_gamma", 1, XDIM);
        g->norm_off[1] = add_tensor(g, "bn_beta", 1, XDIM);
        g->aux_count = 2 * XDIM;
    }
    StarTab& st = g->stab;
    auto add_seg = [&](int64_t shared, int64_t spec, int cnt, int op) {
        st.shared[st.n] = shared;
        st.spec[st.n] = spec;
        st.cnt[st.n] = cnt;
        st.op[st.n] = op;
        st.first4[st.n + 1] = st.first4[st.n] + cnt / 4;
        return st.n++;
    };
    const int nl = (int)d.layers.size();
    for (int l = 0; sf && l < nl; ++l) {
        const Layer& L = d.layers[l];
        g->seg_k[l] = add_seg(L.w_off, add_tensor(g, "Wd" + std::to_string(l), (int64_t)D * L.in, L.out), L.in * L.out, SSEG_MUL);
    }
    for (int l = 0; sf && l < nl; ++l) {
        const Layer& L = d.layers[l];
        g->seg_b[l] = add_seg(L.b_off, add_tensor(g, "bd" + std::to_string(l), D, L.out), L.out, SSEG_ADD);
    }
    t.head_w = add_tensor(g, "wo", d.layers.back().out, 1);
    t.head_gb = add_tensor(g, "gb", 1, 1);
    if (A) {
        g->seg_aw = add_seg(0, add_tensor(g, "aux_W", (int64_t)D * XDIM, A), XDIM * A, SSEG_COPY);
        g->seg_ab = add_seg(0, add_tensor(g, "aux_b", D, A), A, SSEG_COPY);
    }
    int c = XDIM;
    if (cfg.star_norm) { g->xn_col = c; c += XDIM; }
    plan_cols(t, d, c);
    if (A) {
        g->a_col = c; c += A;
        g->jtop_col = c; c += A;
    }
    return c;
}
// oracle/fmnets.py param_names: domain_emb | W0 W1 W2 | b0 b1 b2 | wo | gb | (NFM) lin_domain -- one block, all of it
// trained by every step.  NFM: DNN on the 128 interaction columns; PNN: on x (+ 3 inner products into W0's last rows)
int layout_single(mamdr_graph* g) {
    const mamdr_graph_config& cfg = g->cfg;
    Task& t = g->tasks[0];
    const bool nfm = cfg.kind == MAMDR_GRAPH_NFM, pnn = cfg.kind == MAMDR_GRAPH_PNN, ccpm = cfg.kind == MAMDR_GRAPH_CCPM,
               autoint = cfg.kind == MAMDR_GRAPH_AUTOINT;
    if (ccpm) {         // conv1_w [6][4] | conv1_b [4] | conv2_w [4 in][4 out] | conv2_b [4]: 48 contiguous floats
        g->conv_off = add_tensor(g, "conv1_w", 6, 4);
        add_tensor(g, "conv1_b", 1, 4);
        add_tensor(g, "conv2_w", 4, 4);
        add_tensor(g, "conv2_b", 1, 4);
    }
    if (autoint) {      // [W_query | W_key | W_value | W_res] per layer: [128][128], then [32][128] twice
        g->att_w[0] = add_tensor(g, "att0_w", EMB, ATT_P);
        g->att_w[1] = add_tensor(g, "att1_w", ATT_OUT, ATT_P);
        g->att_w[2] = add_tensor(g, "att2_w", ATT_OUT, ATT_P);
    }
    // (NFM / CCPM: 128-wide fields only)
    const Dnn& d = add_dnn_wb(g, "W", "b", nfm ? EMB : (ccpm ? 4 * EMB : 3 * g->emb), pnn ? 3 : 0);
    t.head_w = add_tensor(g, "wo", (autoint ? 3 * ATT_OUT : 0) + d.layers.back().out, 1);
    t.head_gb = add_tensor(g, "gb", 1, 1);
    if (g->has_lin) g->lin_d_off = add_tensor(g, "lin_domain", cfg.n_domain, 1);
    if (cfg.uncertainty_weight) g->lv_off = add_tensor(g, "log_var", cfg.n_domain, 1);
    int c = 3 * g->emb;
    g->f_col = c;
    if (nfm || ccpm) g->in_col = c;
    if (pnn) g->xe_col = c;
    c += nfm ? EMB : (ccpm ? 4 * EMB : 4);
    if (ccpm) { g->cg_col = c; c += 64; }
    std::vector<int> cols;
    for (size_t l = 0; l < d.layers.size(); ++l) {
        if (autoint && l + 1 == d.layers.size()) {      // head input = [attention output 96 | last DNN layer]
            g->top_col = c;
            c += 3 * ATT_OUT;
        }
        cols.push_back(c);
        c += d.layers[l].out;
    }
    t.col.push_back(cols);
    return c;
}
// Star and the deepctr towers: ONE task whose block is the shared one (all of it trained by every step)
int layout_one_task(mamdr_graph* g) {
    Task& t = g->tasks[0];
    t.tower = 0;
    t.path.push_back(0);
    const int c = g->star ? layout_star(g) : layout_single(g);
    g->shared_end = g->n_params;
    t.blk_off = t.blk_end = g->n_params;
    t.n_cols = c;
    return c;
}
// oracle/mtl.py Spec.tensors: the block every task's model trains (the shared experts), then one block per task: its own
// experts, gate, tower, head.  Columns: x | every layer output on the path | gate probabilities | mixture
int layout_multi_task(mamdr_graph* g) {
    const mamdr_graph_config& cfg = g->cfg;
    int n_shared, n_specific;
    expert_counts(cfg, n_shared, n_specific);
    uint32_t next_id = 0;
    std::vector<int> shared;
    for (int e = 0; e < n_shared; ++e) {
        const std::string nm = cfg.kind == MAMDR_GRAPH_SHARED_BOTTOM ? "bottom"
                               : (cfg.kind == MAMDR_GRAPH_MMOE ? "expert_" + std::to_string(e) : "shared_expert_" + std::to_string(e));
        shared.push_back(add_dnn(g, nm, XDIM, cfg.expert_hidden, cfg.n_expert_hidden, next_id));
    }
    g->shared_end = g->n_params;
    int max_cols = 0;
    for (int d = 0; d < cfg.n_domain; ++d) {
        Task& t = g->tasks[d];
        const std::string ds = std::to_string(d);
        t.blk_off = g->n_params;
        for (int e = 0; e < n_specific; ++e)
            t.mix.push_back(add_dnn(g, "task_" + ds + "_expert_" + std::to_string(e), XDIM, cfg.expert_hidden, cfg.n_expert_hidden, next_id));
        for (int s : shared) t.mix.push_back(s);
        if (g->gated) {
            t.gate = add_dnn(g, "gate_" + ds, XDIM, cfg.gate_hidden, cfg.n_gate_hidden, next_id);
            t.wg_off = add_tensor(g, "gate_" + ds + "/Wg", cfg.gate_hidden[cfg.n_gate_hidden - 1], (int64_t)t.mix.size());
        }
        t.tower = add_dnn(g, "tower_" + ds, g->n_h, cfg.tower_hidden, cfg.n_tower_hidden, next_id);
        t.head_w = add_tensor(g, "head_" + ds + "/w", cfg.tower_hidden[cfg.n_tower_hidden - 1], 1);
        t.head_gb = add_tensor(g, "head_" + ds + "/gb", 1, 1);
        t.blk_end = g->n_params;
        int c = XDIM;
        t.path = t.mix;
        if (g->gated) t.path.push_back(t.gate);
        t.path.push_back(t.tower);
        for (int di : t.path) plan_cols(t, g->dnns[di], c);
        if (g->gated) {
            t.g_col = c; c += ((int)t.mix.size() + 3) & ~3;
            t.m_col = c; c += g->n_h;
        }
        t.n_cols = c;
        if (c > max_cols) max_cols = c;
    }
    return max_cols;
}

// every device allocation of a context goes through its record (DevAllocs, host_common.h): mamdr_graph_destroy frees what
// it holds (after the first failure nothing more is allocated; reported below)
hipError_t alloc_workspace(mamdr_graph* g) {
    const mamdr_graph_config& cfg = g->cfg;
    float thr[500];
    auc_thresholds(thr);
    const size_t rp = (size_t)g->rows_pad_max, n_grad = (size_t)(g->n_params - g->table_floats);
    g->dev.alloc(&g->act, rp * g->ld);
    g->dev.alloc(&g->dact, rp * g->ld);
    g->dev.alloc(&g->grad, n_grad);
    size_t max_w = (size_t)EMB * ATT_P;
    for (const Dnn& d : g->dnns)
        for (const Layer& L : d.layers) max_w = std::max(max_w, (size_t)L.in * L.out);
    g->wpart_floats = 16 * max_w;
    if (g->defer_w) {       // the queue holds every problem's partial products at once: 8 splits of the widest step's kernels
        size_t max_path = 3 * (size_t)EMB * ATT_P;
        for (const Task& t : g->tasks) {
            size_t w = cfg.kind == MAMDR_GRAPH_AUTOINT ? 3 * (size_t)EMB * ATT_P : 0;
            for (int id : t.path)
                for (const Layer& L : g->dnns[id].layers) w += (size_t)L.in * L.out;
            max_path = std::max(max_path, w);
        }
        g->wpart_floats = std::max(g->wpart_floats, 8 * max_path);
    }
    g->wpart_floats += 16 * (size_t)XDIM * cfg.auxiliary_dim;       // Star: the auxiliary kernel's splits
    g->dev.alloc(&g->wpart, g->wpart_floats);
    if (g->stab.n) {
        g->dev.alloc(&g->eff, 4 * (size_t)g->stab.first4[g->stab.n]);
        g->dev.alloc(&g->deff, 4 * (size_t)g->stab.first4[g->stab.n]);
    }
    if (cfg.star_norm) {
        g->dev.alloc(&g->spart, (rp + SN_ROWS - 1) / SN_ROWS * 2 * XDIM);
        g->dev.alloc(&g->pnv, (size_t)3 * XDIM);
    }
    size_t max_mix = 0;
    for (const Task& t : g->tasks) max_mix = std::max(max_mix, t.mix.size());
    if (g->gated && max_mix > 1) {
        g->dxpart_floats = max_mix * rp * (size_t)(g->tables ? XDIM : EMB);
        g->dev.alloc(&g->dxpart, g->dxpart_floats);
    }
    if (g->tables) {
        g->dev.alloc(&g->urow, rp);
        g->dev.alloc(&g->irow, rp);
        g->dev.alloc(&g->hasdup_u, rp);
        g->dev.alloc(&g->hasdup_i, rp);
        g->dev.alloc(&g->map_u, (size_t)cfg.n_user);
        g->dev.alloc(&g->map_i, (size_t)cfg.n_item);
        g->dev.alloc(&g->gbuf_u, rp * g->emb);
        g->dev.alloc(&g->gbuf_i, rp * g->emb);
    }
    g->dev.alloc(&g->dlogit, rp);
    g->dev.alloc(&g->rowloss, rp);
    g->dev.alloc(&g->y, rp);
    g->dev.alloc(&g->domrow, rp);
    g->dev.alloc(&g->thresholds, (size_t)500);
    g->dev.alloc(&g->frozen_sumsq, (size_t)4);
    g->dev.alloc(&g->sumsq_partials, (size_t)1024);
    g->dev.alloc(&g->eval_acc, (size_t)4);
    if (cfg.kind == MAMDR_GRAPH_AUTOINT) {
        g->dev.alloc(&g->xt, rp * XDIM);
        g->dev.alloc(&g->dxt, rp * XDIM);
        for (int l = 0; l < 3; ++l) {
            g->dev.alloc(&g->attP[l], 3 * rp * ATT_P);
            g->dev.alloc(&g->attdP[l], 3 * rp * ATT_P);
            g->dev.alloc(&g->attA[l], rp * 36);
            g->dev.alloc(&g->attY[l], 3 * rp * ATT_OUT);
            g->dev.alloc(&g->attdY[l], 3 * rp * ATT_OUT);
        }
    }
    if (g->has_lin) {
        g->dev.alloc(&g->extra, rp);
        if (g->tables) {
            g->dev.alloc(&g->glin_u, rp);
            g->dev.alloc(&g->glin_i, rp);
        }
    }
    hipError_t e = g->dev.err;
    if (e == hipSuccess) e = hipMemsetAsync(g->grad, 0, n_grad * sizeof(float), g->stream);
    if (g->tables && e == hipSuccess) {
        e = hipMemsetAsync(g->hasdup_u, 0, rp * sizeof(int32_t), g->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->hasdup_i, 0, rp * sizeof(int32_t), g->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->urow, 0xff, rp * sizeof(int32_t), g->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->irow, 0xff, rp * sizeof(int32_t), g->stream);
        launch_emb_map_init(g->map_u, cfg.n_user, g->stream);
        launch_emb_map_init(g->map_i, cfg.n_item, g->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(g->dact, 0, rp * g->ld * sizeof(float), g->stream);
    if (e == hipSuccess) e = hipMemsetAsync(g->frozen_sumsq, 0, 4 * sizeof(float), g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(g->thresholds, thr, sizeof(thr), hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    return e;
}

// every environment switch of this engine (env_registry.h), read at mamdr_graph_create
void read_switches(mamdr_graph* g) {
    if (const char* ev = getenv("MAMDR_GRAPH_NO_DEFER")) g->defer_w = atoi(ev) == 0;
    {
        const char* ev = getenv("MAMDR_GRAPH_TILE32_BELOW");
        g_tile32_below.store(ev ? atoi(ev) : TILE32_BELOW_DEFAULT, std::memory_order_relaxed);
    }
    if (const char* ev = getenv("MAMDR_GRAPH_NO_TAIL_OPT")) g->tail_opt = atoi(ev) == 0;
    if (const char* ev = getenv("MAMDR_REC_CHUNK"))
        if (atoi(ev) > 0) g->rec_chunk = (int)std::min<int64_t>(((int64_t)atoi(ev) + REC_TILE - 1) / REC_TILE * REC_TILE, 1 << 20);
}

// ================================================================== retrieval from the single-output towers (graph_retrieval.h)
const char* kind_name(int kind) {
    static const char* const names[] = {"shared_bottom", "mmoe", "ple", "nfm", "pnn", "ccpm", "autoint", "mlp", "wdl", "deepfm", "star"};
    return kind >= 0 && kind < (int)(sizeof(names) / sizeof(names[0])) ? names[kind] : "?";
}
// the kinds these calls serve: ONE task for every domain and no state outside the flat vector
int retrieval_kind(const mamdr_graph* g, const char* fn) {
    if (g->single && !g->star) return MAMDR_OK;
    return gfail(MAMDR_ENOTBUILT, "%s: the %s tower is not built for retrieval (%s); nfm, pnn, ccpm, autoint, mlp, wdl and deepfm are",
                 fn, kind_name(g->cfg.kind),
                 g->star ? "its per-domain tensors and norm state are not prepared for inference here" : "it holds one task per domain");
}
// the handle's retrieval workspaces: the per-batch columns on first use; `part_keys` keys of per-tile lists and `n_tkey`
// target / slate keys grown on demand (0: not needed by this call)
int grow_retrieval(mamdr_graph* g, size_t part_keys, size_t n_tkey) {
    const size_t rp = (size_t)g->rows_pad_max;
    if (!g->ret_uid) {
        g->dev.alloc(&g->ret_uid, rp);
        g->dev.alloc(&g->ret_pid, rp);
        g->dev.alloc(&g->ret_dom, rp);
        g->dev.alloc(&g->ret_rowq, rp);
        g->dev.alloc(&g->ret_label, rp);
        g->dev.alloc(&g->ret_keys, rp);
        g->dev.alloc(&g->ret_best, (size_t)REC_QBLOCK * REC_KMAX);
        if (g->dev.err != hipSuccess) {     // all or nothing: the next call starts over
            for (void* p : {(void*)g->ret_uid, (void*)g->ret_pid, (void*)g->ret_dom, (void*)g->ret_rowq, (void*)g->ret_label,
                            (void*)g->ret_keys, (void*)g->ret_best})
                g->dev.release(p);
            g->ret_uid = g->ret_pid = g->ret_dom = g->ret_rowq = nullptr;
            g->ret_label = nullptr;
            g->ret_keys = g->ret_best = nullptr;
            return g->dev.check(g_gerr);
        }
    }
    if (const int rc = g->ret_part.grow(g->dev, g_gerr, part_keys)) return rc;
    return g->ret_tkey.grow(g->dev, g_gerr, n_tkey);
}
// the pair kernels' view of a block of queries (b.dom null: every query in b.domain)
PairArgs pair_args(const mamdr_graph* g, const RetCall& b) {
    PairArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.uid = g->ret_uid;
    pa.pid = g->ret_pid;
    pa.dom = g->ret_dom;
    pa.label = g->ret_label;
    pa.rowq = g->ret_rowq;
    pa.n_user = g->cfg.n_user;
    pa.n_item = g->cfg.n_item;
    pa.n_domain = g->cfg.n_domain;
    pa.q_uid = b.uid;
    pa.q_dom = b.dom;
    pa.dom_all = b.domain;
    pa.n_query = b.n_query;
    return pa;
}
// the inference forward over the `rows` pair rows in the workspace -- ALWAYS at the full padded height: a layer picks its
// tile form, and with it its rounding, from the padded row count (use_tile32), so every batch of these calls runs as a full
// evaluation batch does and a pair's logit does not depend on where the pair sits.  -> the head's operands
HeadArgs retrieval_forward(mamdr_graph* g, int rows) {
    StepCtx sc;
    memset(&sc, 0, sizeof(sc));
    sc.rows = rows;
    sc.rp = g->rows_pad_max;
    sc.keep_scale = 1.0f;
    SplitData d;
    d.uid = g->ret_uid;
    d.pid = g->ret_pid;
    d.dom = g->ret_dom;
    d.label = g->ret_label;
    d.n = g->rows_pad_max;
    d.bound = true;
    launch_gather(g, d, nullptr, 0, sc);
    const Task& t = g->tasks[0];
    return head_args(g, t, sc, task_forward(g, t, sc));
}
// the generic layers as retrieval_host.h's backend: every pair is a row of a forward batch
struct GraphRetrieval : RetStream {
    mamdr_graph* g;
    const int n_item = g->cfg.n_item, n_domain = g->cfg.n_domain, rec_chunk = g->rec_chunk;
    RetCall b{};                    // the block under way
    RecArgs ma;                     // what k_rec_merge reads
    TileArgs ta;                    // the ending's operands (k_graph_tile_topk / k_graph_rank_count)
    SlateArgs sa;

    int ready() { return ::ready(g); }
    // top-K: the per-tile lists of a block's queries x a chunk; ranks and slates: the list's keys
    int prepare(const RetCall& r) {
        const bool topk = r.kind == RET_TOPK;
        const int kt = std::min<int>(r.k, REC_TILE), tiles_cap = r.chunk / REC_TILE;
        const size_t part_keys = topk ? (size_t)std::min<int32_t>(REC_QBLOCK, r.n_query) * tiles_cap * REC_TILE : 0;
        if (const int rc = grow_retrieval(g, part_keys, (size_t)r.n_list)) return rc;
        memset(&ma, 0, sizeof(ma));
        memset(&ta, 0, sizeof(ta));
        if (!topk) {
            ta.tkey = sa.tkey = g->ret_tkey.p;
            ta.rank_out = r.rank_out;
            sa.pos_out = r.pos_out;
            sa.order_out = r.order_out;
            return MAMDR_OK;
        }
        ma.k = r.k;
        ma.kt = ta.kt = kt;
        ma.tiles_cap = ta.tiles_cap = tiles_cap;
        ma.part = ta.part = g->ret_part.p;
        ma.best = g->ret_best;
        return MAMDR_OK;
    }
    void begin_block(const RetCall& blk) {
        b = blk;
        ma.n_query = sa.n_query = b.n_query;
        ma.ids_out = b.ids_out;
        ma.scores_out = b.scores_out;
        ta.tgt_off = sa.off = b.list_off;
        ta.live_out = b.live_out;
    }
    // one chunk of candidates x the block's queries: the [n_query][chunk_pad] grid of pairs, query-major, a forward batch
    // at a time, each with its ending (ranks: k_graph_rank_count; top-K: k_graph_tile_topk, then the chunk's k_rec_merge)
    int cand_pass(int64_t c0, int n_chunk, int tiles, bool first, bool last) {
        const bool count = b.kind == RET_RANK;
        const int chunk_pad = tiles * REC_TILE;
        const int64_t total = (int64_t)b.n_query * chunk_pad;
        PairArgs pa = pair_args(g, b);
        pa.ids = b.cand;
        pa.c_base = c0;
        pa.chunk_pad = chunk_pad;
        pa.n_chunk = n_chunk;
        for (int64_t base = 0; base < total; base += g->rows_pad_max) {
            const int rows = (int)std::min<int64_t>(g->rows_pad_max, total - base);
            pa.rows = rows;
            pa.row_base = base;
            GLAUNCH(k_graph_pair_rows<false>, dim3((rows + 255) / 256), dim3(256), 0, g->stream, pa);
            KeyArgs ka;
            memset(&ka, 0, sizeof(ka));
            ka.h = retrieval_forward(g, rows);
            ka.pid = g->ret_pid;
            ka.rowq = g->ret_rowq;
            ka.excl_off = b.excl_off;
            ka.excl_ids = b.excl_ids;
            ka.scores_all = b.scores_all;
            ka.n_cand = b.n_cand;
            ka.c_base = c0;
            ka.row_base = base;
            ka.chunk_pad = chunk_pad;
            ka.keys = g->ret_keys;
            GLAUNCH(k_graph_head_keys<false>, dim3((rows + 3) / 4), dim3(256), 0, g->stream, ka);
            ta.keys = g->ret_keys;
            ta.n_tiles = rows / REC_TILE;
            ta.row_base = base;
            ta.chunk_pad = chunk_pad;
            if (count) GLAUNCH(k_graph_rank_count, dim3((ta.n_tiles + 3) / 4), dim3(256), 0, g->stream, ta);
            else GLAUNCH(k_graph_tile_topk, dim3((ta.n_tiles + 3) / 4), dim3(256), 0, g->stream, ta);
        }
        if (count) return MAMDR_OK;
        ma.tiles = tiles;
        ma.first_chunk = first;
        ma.last_chunk = last;
        ++g_graph_launches;
        launch_rec_merge(ma, g->stream);
        return MAMDR_OK;
    }
    // entries [j0, j1) of the call's flat list (targets, slate entries; b.list_off: the block's CSR with the call's absolute
    // positions), a forward batch at a time: their keys into ret_tkey, their scores into score_out when asked
    int list_pass(int64_t j0, int64_t j1) {
        PairArgs pa = pair_args(g, b);
        pa.ids = b.list_ids;
        pa.off = b.list_off;
        for (int64_t base = j0; base < j1; base += g->rows_pad_max) {
            const int rows = (int)std::min<int64_t>(g->rows_pad_max, j1 - base);
            pa.rows = rows;
            pa.list_base = base;
            GLAUNCH(k_graph_pair_rows<true>, dim3((rows + 255) / 256), dim3(256), 0, g->stream, pa);
            KeyArgs ka;
            memset(&ka, 0, sizeof(ka));
            ka.h = retrieval_forward(g, rows);
            ka.pid = g->ret_pid;
            ka.rowq = g->ret_rowq;
            ka.tkey = g->ret_tkey.p;
            ka.score_out = b.score_out;
            ka.list_base = base;
            GLAUNCH(k_graph_head_keys<true>, dim3((rows + 3) / 4), dim3(256), 0, g->stream, ka);
        }
        return MAMDR_OK;
    }
    void slate_order(int64_t max_len, bool any_short) {
        g_graph_launches += (any_short ? 1 : 0) + (max_len > SLATE_WAVE ? 1 : 0);
        launch_slate_order(sa, max_len, any_short, g->stream);
    }
    int finish() {
        GHIP(hipGetLastError());
        return MAMDR_OK;
    }
};

}  // namespace

extern "C" {

const char* mamdr_graph_last_error(void) { return g_gerr.text; }

int mamdr_graph_create(const mamdr_graph_config* cfg, void* stream, mamdr_graph** out) {
    if (!cfg || !out) return gfail(MAMDR_EINVAL, "null argument");
    *out = nullptr;
    (void)mamdr::env_warn_unknown();
    if (const int rc = validate_config(cfg)) return rc;
    mamdr_graph* g = new (std::nothrow) mamdr_graph();
    if (!g) return gfail(MAMDR_EHIP, "out of host memory");
    g->cfg = *cfg;
    g->star = cfg->kind == MAMDR_GRAPH_STAR;
    memset(&g->stab, 0, sizeof(g->stab));
    if (g->star) {          // star.py:70-96 builds no dropout and no regulariser: the config's values are ignored
        g->cfg.dropout = 0.f;
        g->cfg.l2_emb = 0.f;
        g->cfg.l2_linear = 0.f;
    } else {
        g->cfg.star_norm = g->cfg.star_dense = g->cfg.auxiliary_dim = 0;
    }
    g->emb = cfg->emb_dim;
    g->stream = (hipStream_t)stream;
    read_switches(g);
    g->sink.p = nullptr;
    g->gated = cfg->kind == MAMDR_GRAPH_MMOE || cfg->kind == MAMDR_GRAPH_PLE;
    g->single = cfg->kind >= MAMDR_GRAPH_NFM;
    g->has_lin = cfg->kind == MAMDR_GRAPH_NFM || cfg->kind == MAMDR_GRAPH_CCPM || cfg->kind == MAMDR_GRAPH_AUTOINT ||
                 cfg->kind == MAMDR_GRAPH_WDL || cfg->kind == MAMDR_GRAPH_DEEPFM;
    g->n_h = cfg->expert_hidden[cfg->n_expert_hidden - 1];
    g->data.resize((size_t)cfg->n_domain * 3);
    g->tables = cfg->emb_trainable != 0;
    if (g->tables) {        // [user table | item table] contiguous at the head (k_emb_sweep walks them as one range)
        add_tensor(g, "user_emb", cfg->n_user, g->emb);
        add_tensor(g, "item_emb", cfg->n_item, g->emb);
        if (g->has_lin) {   // their 1-d linear tables train with them (deepctr: same feature column)
            g->lin_u_off = add_tensor(g, "lin_user", cfg->n_user, 1);
            g->lin_i_off = add_tensor(g, "lin_item", cfg->n_item, 1);
        }
        g->table_floats = g->n_params;
    }
    g->dm_off = add_tensor(g, "domain_emb", cfg->n_domain, g->emb);
    g->tasks.resize(g->single ? 1 : cfg->n_domain);
    const int max_cols = g->single ? layout_one_task(g) : layout_multi_task(g);
    g->ld = (max_cols + 3) & ~3;
    g->rows_pad_max = (cfg->max_batch + GT - 1) / GT * GT;
    const hipError_t e = alloc_workspace(g);
    if (e != hipSuccess) {
        mamdr_graph_destroy(g);
        return gfail(MAMDR_EHIP, "workspace: %s", hipGetErrorString(e));
    }
    *out = g;
    return MAMDR_OK;
}

int mamdr_graph_destroy(mamdr_graph* g) {
    if (!g) return MAMDR_OK;
    (void)hipStreamSynchronize(g->stream);
    g->dev.free_all();
    delete g;
    return MAMDR_OK;
}

int64_t mamdr_graph_param_count(const mamdr_graph* g) { return g ? g->n_params : 0; }
int32_t mamdr_graph_tensor_count(const mamdr_graph* g) { return g ? (int32_t)g->tensors.size() : 0; }
int mamdr_graph_tensor_info(const mamdr_graph* g, int32_t i, char* name, int32_t name_cap, int64_t* offset, int64_t* rows,
                            int64_t* cols) {
    if (check(g)) return MAMDR_EINVAL;
    if (i < 0 || i >= (int32_t)g->tensors.size() || !name || name_cap < 2 || !offset || !rows || !cols)
        return gfail(MAMDR_EINVAL, "bad tensor query");
    const TensorInfo& t = g->tensors[i];
    snprintf(name, (size_t)name_cap, "%s", t.name.c_str());
    *offset = t.off;
    *rows = t.rows;
    *cols = t.cols;
    return MAMDR_OK;
}
/* the two ranges of the flat vector a step of task `domain` trains */
int mamdr_graph_task_ranges(const mamdr_graph* g, int domain, int64_t* shared_off, int64_t* shared_count, int64_t* task_off,
                            int64_t* task_count) {
    if (check(g)) return MAMDR_EINVAL;
    if (domain < 0 || domain >= g->cfg.n_domain) return gfail(MAMDR_EINVAL, "domain out of range");
    *shared_off = g->dm_off;
    *shared_count = g->shared_end - g->dm_off;
    const Task& t = g->tasks[g->single ? 0 : domain];
    *task_off = t.blk_off;
    *task_count = t.blk_end - t.blk_off;
    return MAMDR_OK;
}

int mamdr_graph_bind_state(mamdr_graph* g, float* d_params, float* d_m, float* d_v) {
    if (check(g)) return MAMDR_EINVAL;
    if (const int rc = check_state_ptrs(g_gerr, d_params, d_m, d_v)) return rc;
    g->params = d_params;
    g->adam_m = d_m;
    g->adam_v = d_v;
    if (g->tables) {
        g->user_tab = d_params;
        g->item_tab = d_params + (size_t)g->cfg.n_user * g->emb;
    }
    return MAMDR_OK;
}
int mamdr_graph_optimizer_reset(mamdr_graph* g) {
    if (check(g)) return MAMDR_EINVAL;
    if (!g->params) return gfail(MAMDR_ESTATE, "state not bound");
    GHIP(hipMemsetAsync(g->adam_m, 0, (size_t)g->n_params * sizeof(float), g->stream));
    GHIP(hipMemsetAsync(g->adam_v, 0, (size_t)g->n_params * sizeof(float), g->stream));
    g->adam_t = 0;
    g->b1p = g->b2p = 1.f;
    return MAMDR_OK;
}
// the counterpart of mamdr_set_counters for the generic-layer engine: TF's running beta powers after `optimizer_steps` steps
// (one optimizer object for all D compiled models: deep_mtl_ctr.py:52-55) and the position of the dropout stream
int mamdr_graph_set_counters(mamdr_graph* g, int64_t optimizer_steps, int64_t dropout_steps) {
    if (check(g)) return MAMDR_EINVAL;
    if (optimizer_steps < 0 || optimizer_steps > (int64_t)0x7ffffff0 || dropout_steps < 0 || dropout_steps > (int64_t)0xffffffffLL)
        return gfail(MAMDR_EINVAL, "mamdr_graph_set_counters(%lld, %lld): out of range", (long long)optimizer_steps, (long long)dropout_steps);
    g->adam_t = optimizer_steps;
    tf_beta_powers(g->cfg.adam_beta1, g->cfg.adam_beta2, optimizer_steps, &g->b1p, &g->b2p);
    g->global_step = (uint32_t)dropout_steps;
    return MAMDR_OK;
}
int mamdr_graph_set_adam_eps(mamdr_graph* g, float eps) {
    if (check(g)) return MAMDR_EINVAL;
    if (!(eps > 0.f)) return gfail(MAMDR_EINVAL, "adam epsilon %g", (double)eps);
    g->cfg.adam_eps = eps;
    return MAMDR_OK;
}
/* non-trainable state of the Star forms' norm layer (layout: include/mamdr_hip.h) */
int64_t mamdr_graph_aux_count(const mamdr_graph* g) { return g ? g->aux_count : 0; }
int mamdr_graph_bind_aux(mamdr_graph* g, float* d_aux) {
    if (check(g)) return MAMDR_EINVAL;
    if (!g->aux_count) return gfail(MAMDR_ESTATE, "this tower has no state outside the flat vector");
    if (!d_aux || ((uintptr_t)d_aux & 15)) return gfail(MAMDR_EINVAL, "aux pointer null or not 16-byte aligned");
    g->aux = d_aux;
    return MAMDR_OK;
}
int64_t mamdr_graph_launch_count(void) { return (int64_t)g_graph_launches.load(); }
int64_t mamdr_graph_optimizer_steps(const mamdr_graph* g) { return g ? g->adam_t : 0; }
int64_t mamdr_graph_dropout_steps(const mamdr_graph* g) { return g ? (int64_t)g->global_step : 0; }

int mamdr_graph_bind_table(mamdr_graph* g, int seg, const float* d_rows, int64_t n_rows) {
    if (check(g)) return MAMDR_EINVAL;
    if (const int rc = check_bind_table(g_gerr, g->tables, seg, d_rows, n_rows, g->cfg.n_user, g->cfg.n_item)) return rc;
    const int item = seg == MAMDR_SEG_ITEM_EMB;
    (item ? g->item_tab : g->user_tab) = d_rows;
    launch_sumsq(d_rows, n_rows * g->emb, g->sumsq_partials, g->frozen_sumsq + item, g->stream);
    GHIP(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_graph_bind_domain_data(mamdr_graph* g, int domain, int split, const int32_t* d_uid, const int32_t* d_pid,
                                 const int32_t* d_domain, const float* d_label, int64_t n_rows) {
    if (check(g)) return MAMDR_EINVAL;
    return bind_columns(g_gerr, split_of(g, domain, split), domain, split, d_uid, d_pid, d_domain, d_label, n_rows);
}

int mamdr_graph_train_steps(mamdr_graph* g, int domain, const int32_t* d_perm, int64_t first_step, int64_t n_steps,
                            int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr, float* d_loss_out) {
    return mamdr_graph_train_steps_n(g, domain, d_perm, -1, first_step, n_steps, batch, dropout_seed, optimizer, lr, d_loss_out);
}

int mamdr_graph_train_steps_n(mamdr_graph* g, int domain, const int32_t* d_perm, int64_t pass_rows, int64_t first_step,
                              int64_t n_steps, int32_t batch, uint32_t dropout_seed, int32_t optimizer, float lr,
                              float* d_loss_out) {
    if (check(g)) return MAMDR_EINVAL;
    if (ready(g)) return MAMDR_ESTATE;
    SplitData* d = split_of(g, domain, MAMDR_SPLIT_TRAIN);
    if (const int rc = check_train_call(g_gerr, d, domain, batch, g->cfg.max_batch, optimizer, g->accum,
                                        "mamdr_graph_bind_accumulator", first_step, n_steps, &pass_rows))
        return rc;
    if (pass_rows < d->n && !d_perm) return gfail(MAMDR_EINVAL, "a pass over part of a split needs its permutation");
    if (const int rc = check_step_range(g_gerr, domain, pass_rows, batch, first_step, n_steps)) return rc;
    if (n_steps == 0) return MAMDR_OK;
    const Task& t = g->tasks[g->single ? 0 : domain];
    for (int64_t s = 0; s < n_steps; ++s) {
        const int64_t row_base = (first_step + s) * batch;
        g->wq.clear();          // (a step that failed half-way leaves its queues behind)
        g->tq.clear();
        const StepCtx sc = step_ctx(g, pass_rows, row_base, batch, true, dropout_seed, optimizer != MAMDR_OPT_ACCUMULATE);
        const OptStep opt = advance_optimizer(g, optimizer, lr);
        open_sink(g, opt);
        launch_gather(g, *d, d_perm, row_base, sc);
        const int t_col = task_forward(g, t, sc);
        const int n_t = launch_head(g, t, sc, t_col, nullptr, nullptr);
        if (d_loss_out && g->tables) refresh_sumsq(g);
        if (d_loss_out || g->lv_off >= 0)       // the weighted loss takes d / d log_var from the batch's mean BCE: this launch, always
            launch_loss(g, sc, d_loss_out ? d_loss_out + s : g->eval_acc + 1, false);
        small_tn(g, g->act + t_col, g->ld, g->dlogit, 1, sc.rp, n_t, 1, g->G(t.head_w), g->G(t.head_gb));   // head: dw = t^T dlogit, dgb = sum dlogit
        task_backward(g, t, sc);
        finish_grads(g, sc);
        if (g->star) star_chain(g);
        if (g->tables) table_step(g, sc, opt);
        if (!g->sink.p) adam_step(g, t, opt);   // (closed from the start, or dropped: a queue overflowed in mid-step)
        g->global_step += 1;
    }
    GHIP(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_graph_bind_accumulator(mamdr_graph* g, float* d_acc) {
    if (check(g)) return MAMDR_EINVAL;
    if (d_acc && ((uintptr_t)d_acc & 15)) return gfail(MAMDR_EINVAL, "accumulator is not 16-byte aligned");
    g->accum = d_acc;
    return MAMDR_OK;
}

int mamdr_graph_eval_domain(mamdr_graph* g, int domain, int split, int32_t batch, float* d_loss_out, uint32_t* d_hist,
                            float* d_pred_out) {
    if (check(g)) return MAMDR_EINVAL;
    if (ready(g)) return MAMDR_ESTATE;
    SplitData* d = split_of(g, domain, split);
    if (!d || !d->bound) return gfail(MAMDR_ESTATE, "split %d of domain %d is not bound", split, domain);
    if (batch <= 0 || batch > g->cfg.max_batch) return gfail(MAMDR_EINVAL, "batch %d outside (0, max_batch=%d]", batch, g->cfg.max_batch);
    if (!d_loss_out || !d_hist) return gfail(MAMDR_EINVAL, "null output pointer");
    if (d->n <= 0) return gfail(MAMDR_EINVAL, "empty split");
    const Task& t = g->tasks[g->single ? 0 : domain];
    GHIP(hipMemsetAsync(d_hist, 0, 2 * 501 * sizeof(uint32_t), g->stream));
    GHIP(hipMemsetAsync(g->eval_acc, 0, sizeof(float), g->stream));
    if (g->tables) refresh_sumsq(g);
    const int64_t n_batches = (d->n + batch - 1) / batch;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t row_base = b * batch;
        const StepCtx sc = step_ctx(g, d->n, row_base, batch, false, 0, false);
        launch_gather(g, *d, nullptr, row_base, sc);
        const int t_col = task_forward(g, t, sc);
        launch_head(g, t, sc, t_col, d_hist, d_pred_out ? d_pred_out + row_base : nullptr);
        launch_loss(g, sc, g->eval_acc, true);
    }
    GLAUNCH(k_graph_scale, dim3(1), dim3(1), 0, g->stream, g->eval_acc, 1.0f / (float)n_batches);
    GHIP(hipMemcpyAsync(d_loss_out, g->eval_acc, sizeof(float), hipMemcpyDeviceToDevice, g->stream));
    GHIP(hipGetLastError());
    return MAMDR_OK;
}

// ---- retrieval from the single-output towers (include/mamdr_hip.h; the calls: retrieval_host.h; device side: graph_retrieval.h)
static int graph_retrieval(mamdr_graph* g, RetCall& r) {
    if (check(g)) return MAMDR_EINVAL;
    if (const int rc = retrieval_kind(g, r.fn)) return rc;
    GraphRetrieval b{{g->stream, g_gerr}, g};
    return retrieval_call(b, r);
}

int mamdr_graph_recommend(mamdr_graph* g, int32_t n_query, const int32_t* d_uid, const int32_t* d_domain, const int32_t* d_cand,
                          int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out,
                          float* d_scores_out, float* d_scores_all) {
    RetCall r{RET_TOPK, __func__};
    r.per_query = true, r.n_query = n_query, r.uid = d_uid, r.dom = d_domain, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids;
    r.k = k, r.ids_out = d_ids_out, r.scores_out = d_scores_out, r.scores_all = d_scores_all;
    return graph_retrieval(g, r);
}

int mamdr_graph_recommend_domain(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                                 int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k,
                                 int32_t* d_ids_out, float* d_scores_out, float* d_scores_all) {
    RetCall r{RET_TOPK, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids;
    r.k = k, r.ids_out = d_ids_out, r.scores_out = d_scores_out, r.scores_all = d_scores_all;
    return graph_retrieval(g, r);
}

int mamdr_graph_rank_domain(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                            int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                            const int32_t* d_tgt_ids, int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out) {
    RetCall r{RET_RANK, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids, r.list_off = d_tgt_off, r.list_ids = d_tgt_ids;
    r.rank_out = d_rank_out, r.score_out = d_score_out, r.live_out = d_live_out;
    return graph_retrieval(g, r);
}

int mamdr_graph_rank_slates(mamdr_graph* g, int32_t domain, int32_t n_query, const int32_t* d_uid, const int64_t* d_slate_off,
                            const int32_t* d_slate_ids, float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out) {
    RetCall r{RET_SLATES, __func__};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.list_off = d_slate_off, r.list_ids = d_slate_ids;
    r.score_out = d_score_out, r.pos_out = d_pos_out, r.order_out = d_order_out;
    return graph_retrieval(g, r);
}

}  // extern "C"
