// C ABI of libmamdr_hip.so, the metrics of an evaluation's predictions: mamdr_group_auc, mamdr_exact_metrics,
// mamdr_auc_bootstrap(_bounded), mamdr_isotonic_fit(_bounded), mamdr_isotonic_apply and mamdr_score_sums, and of top-K lists:
// mamdr_id_counts, mamdr_list_similarity, mamdr_list_diversify and mamdr_row_neighbours(_bounded), and of the baselines:
// mamdr_item_cooc, mamdr_history_scores, mamdr_rank_scores and mamdr_topk_scores.  Stateless, like the outer updates: no context, the caller's stream.  Host code
// only.
#include "step_ctx.h"

// a call's own scratch, ordered on its stream: `bytes` are allocated (nothing for 0), `run(ws)` launches and returns its
// first HIP error, the scratch is freed -> MAMDR_OK, or MAMDR_EHIP with the first error of (allocation, run, free) behind `fn`
template <typename F>
static int with_scratch(const char* fn, size_t bytes, hipStream_t s, F run) {
    char* ws = nullptr;
    hipError_t e = bytes ? hipMallocAsync((void**)&ws, bytes, s) : hipSuccess;
    if (e == hipSuccess) e = run(ws);
    const hipError_t ef = ws ? hipFreeAsync(ws, s) : hipSuccess;
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) return fail(MAMDR_EHIP, "%s: %s", fn, hipGetErrorString(e));
    return MAMDR_OK;
}

extern "C" {

// ---- per-user grouped AUC (gauc_kernels.hip)
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
    if (misaligned(3, d_pred, d_label, d_order, d_tile_group, d_P) || misaligned(7, d_group_off, d_tile_first, d_T, d_result))
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
    // the scratch: [T if not given | partial sums | P if not given]
    const size_t t_bytes = d_T ? 0 : (size_t)n_groups * sizeof(uint64_t);
    const size_t part_bytes = (size_t)a.n_parts * (sizeof(double) + 2 * sizeof(uint64_t));
    const size_t p_bytes = d_P ? 0 : (size_t)n_groups * sizeof(uint32_t);
    return with_scratch("mamdr_group_auc", t_bytes + part_bytes + p_bytes, s, [&](char* ws) {
        a.T = d_T ? reinterpret_cast<unsigned long long*>(d_T) : reinterpret_cast<unsigned long long*>(ws);
        a.part_num = reinterpret_cast<double*>(ws + t_bytes);
        a.part_rows = reinterpret_cast<unsigned long long*>(a.part_num + a.n_parts);
        a.part_valid = a.part_rows + a.n_parts;
        a.P = d_P ? d_P : reinterpret_cast<uint32_t*>(ws + t_bytes + part_bytes);
        if (n_groups > 0) {
            if (hipError_t e = hipMemsetAsync(a.T, 0, (size_t)n_groups * sizeof(uint64_t), s)) return e;
            if (hipError_t e = hipMemsetAsync(a.P, 0, (size_t)n_groups * sizeof(uint32_t), s)) return e;
        }
        launch_gauc(a, s);
        return hipGetLastError();
    });
}

// ---- exact AUC, average precision and calibration bins of one split (exact_kernels.hip)
int mamdr_exact_metrics(const float* d_pred, const float* d_label, int64_t n, int32_t n_bins, int64_t* d_counts, double* d_ap,
                        int64_t* d_bins, int64_t* d_sorted_out, void* stream) {
    if (!d_counts || !d_ap || !d_bins) return fail(MAMDR_EINVAL, "mamdr_exact_metrics: null counts / ap / bins pointer");
    if (n < 0 || n > INT32_MAX) return fail(MAMDR_EINVAL, "mamdr_exact_metrics: n %lld outside [0, 2^31)", (long long)n);
    if (n_bins < 1 || n_bins > MAMDR_EXACT_MAX_BINS)
        return fail(MAMDR_EINVAL, "mamdr_exact_metrics: n_bins %d outside 1..%d", (int)n_bins, MAMDR_EXACT_MAX_BINS);
    if (n > 0 && (!d_pred || !d_label)) return fail(MAMDR_EINVAL, "mamdr_exact_metrics: null pred / label pointer");
    if (misaligned(3, d_pred, d_label) || misaligned(7, d_counts, d_ap, d_bins, d_sorted_out))
        return fail(MAMDR_EINVAL, "mamdr_exact_metrics: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    ExactArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = d_pred;
    a.label = d_label;
    a.n = n;
    a.n_bins = n_bins;
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.ap = d_ap;
    a.bins = reinterpret_cast<unsigned long long*>(d_bins);
    a.sorted_out = reinterpret_cast<unsigned long long*>(d_sorted_out);
    HIP_TRY(hipMemsetAsync(d_counts, 0, 5 * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(d_ap, 0, sizeof(double), s));
    HIP_TRY(hipMemsetAsync(d_bins, 0, 3 * (size_t)n_bins * sizeof(int64_t), s));
    if (n == 0) return MAMDR_OK;
    return with_scratch("mamdr_exact_metrics", exact_workspace_bytes(n), s, [&](char* ws) {
        a.ws = ws;
        launch_exact(a, s);
        return hipGetLastError();
    });
}

// ---- bootstrap replicates of the exact AUC's integers (bootstrap_kernels.hip)
int mamdr_auc_bootstrap_bounded(const float* d_pred, const float* d_label, const int32_t* d_unit, int64_t n, int32_t n_rep,
                                uint64_t seed, uint64_t* d_T, int64_t* d_P, int64_t* d_N, int64_t part_words, void* stream) {
    if (!d_T || !d_P || !d_N) return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: null T / P / N pointer");
    if (n < 0 || n >= ((int64_t)1 << 27)) return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: n %lld outside [0, 2^27)", (long long)n);
    if (n_rep < 0 || n_rep > 65535) return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: n_rep %d outside 0..65535", (int)n_rep);
    if (part_words <= 0) return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: part_words %lld is not positive", (long long)part_words);
    if (n > 0 && (!d_pred || !d_label)) return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: null pred / label pointer");
    if (misaligned(3, d_pred, d_label, d_unit) || misaligned(7, d_T, d_P, d_N))
        return fail(MAMDR_EINVAL, "mamdr_auc_bootstrap: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    const size_t out_bytes = ((size_t)n_rep + 1) * sizeof(uint64_t);
    HIP_TRY(hipMemsetAsync(d_T, 0, out_bytes, s));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_P, 0, out_bytes, s));
        HIP_TRY(hipMemsetAsync(d_N, 0, out_bytes, s));
        return MAMDR_OK;
    }
    BootArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = d_pred;
    a.label = d_label;
    a.unit = d_unit;
    a.n = n;
    a.n_rep = n_rep;
    a.seed = seed;
    a.T = reinterpret_cast<unsigned long long*>(d_T);
    a.P = reinterpret_cast<long long*>(d_P);
    a.N = reinterpret_cast<long long*>(d_N);
    a.part_words = part_words;
    return with_scratch("mamdr_auc_bootstrap", boot_workspace_bytes(n, n_rep, part_words), s, [&](char* ws) {
        a.ws = ws;
        launch_boot(a, s);
        return hipGetLastError();
    });
}

int mamdr_auc_bootstrap(const float* d_pred, const float* d_label, const int32_t* d_unit, int64_t n, int32_t n_rep,
                        uint64_t seed, uint64_t* d_T, int64_t* d_P, int64_t* d_N, void* stream) {
    return mamdr_auc_bootstrap_bounded(d_pred, d_label, d_unit, n, n_rep, seed, d_T, d_P, d_N, BOOT_PART_WORDS, stream);
}

// ---- isotonic fit, its application and the score sums (isotonic_kernels.hip)
int mamdr_isotonic_fit_bounded(const float* d_pred, const float* d_label, int64_t n, int64_t* d_counts, uint32_t* d_first_key,
                               int64_t* d_rows, int64_t* d_positives, int32_t tile_points, void* stream) {
    if (!d_counts) return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: null counts pointer");
    if (n < 0 || n > INT32_MAX) return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: n %lld outside [0, 2^31)", (long long)n);
    if (tile_points < MAMDR_ISOTONIC_MIN_TILE)
        return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: tile_points %d below %d", (int)tile_points, MAMDR_ISOTONIC_MIN_TILE);
    if (n > 0 && (!d_pred || !d_label)) return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: null pred / label pointer");
    if (n > 0 && (!d_first_key || !d_rows || !d_positives))
        return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: null first_key / rows / positives pointer");
    if (misaligned(3, d_pred, d_label, d_first_key) || misaligned(7, d_counts, d_rows, d_positives))
        return fail(MAMDR_EINVAL, "mamdr_isotonic_fit: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * sizeof(int64_t), s));
    if (n == 0) return MAMDR_OK;
    IsoFitArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = d_pred;
    a.label = d_label;
    a.n = n;
    a.tile = tile_points;
    a.counts = reinterpret_cast<long long*>(d_counts);
    a.first_key = d_first_key;
    a.rows = reinterpret_cast<long long*>(d_rows);
    a.positives = reinterpret_cast<long long*>(d_positives);
    return with_scratch("mamdr_isotonic_fit", iso_fit_workspace_bytes(n, tile_points), s, [&](char* ws) {
        a.ws = ws;
        launch_iso_fit(a, s);
        return hipGetLastError();
    });
}

int mamdr_isotonic_fit(const float* d_pred, const float* d_label, int64_t n, int64_t* d_counts, uint32_t* d_first_key,
                       int64_t* d_rows, int64_t* d_positives, void* stream) {
    return mamdr_isotonic_fit_bounded(d_pred, d_label, n, d_counts, d_first_key, d_rows, d_positives, ISO_HULL_TILE, stream);
}

int mamdr_isotonic_apply(const uint32_t* d_first_key, const int64_t* d_rows, const int64_t* d_positives, int64_t n_blocks,
                         const float* d_pred, int64_t n, float* d_out, void* stream) {
    if (n < 0 || n > INT32_MAX) return fail(MAMDR_EINVAL, "mamdr_isotonic_apply: n %lld outside [0, 2^31)", (long long)n);
    if (n_blocks < 0 || n_blocks > INT32_MAX || (n > 0 && n_blocks == 0))
        return fail(MAMDR_EINVAL, "mamdr_isotonic_apply: %lld blocks for %lld rows", (long long)n_blocks, (long long)n);
    if (n > 0 && (!d_first_key || !d_rows || !d_positives || !d_pred || !d_out))
        return fail(MAMDR_EINVAL, "mamdr_isotonic_apply: null first_key / rows / positives / pred / out pointer");
    if (misaligned(3, d_first_key, d_pred, d_out) || misaligned(7, d_rows, d_positives))
        return fail(MAMDR_EINVAL, "mamdr_isotonic_apply: a pointer is not aligned to its element size");
    if (n == 0) return MAMDR_OK;
    IsoApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.first_key = d_first_key;
    a.rows = reinterpret_cast<const long long*>(d_rows);
    a.positives = reinterpret_cast<const long long*>(d_positives);
    a.n_blocks = n_blocks;
    a.pred = d_pred;
    a.n = n;
    a.out = d_out;
    launch_iso_apply(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_score_sums(const float* d_pred, const float* d_label, int64_t n, double* d_out, void* stream) {
    if (!d_out) return fail(MAMDR_EINVAL, "mamdr_score_sums: null out pointer");
    if (n < 0 || n > INT32_MAX) return fail(MAMDR_EINVAL, "mamdr_score_sums: n %lld outside [0, 2^31)", (long long)n);
    if (n > 0 && (!d_pred || !d_label)) return fail(MAMDR_EINVAL, "mamdr_score_sums: null pred / label pointer");
    if (misaligned(3, d_pred, d_label) || misaligned(7, d_out))
        return fail(MAMDR_EINVAL, "mamdr_score_sums: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_out, 0, 2 * sizeof(double), s));
        return MAMDR_OK;
    }
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = d_pred;
    a.label = d_label;
    a.n = n;
    a.out = d_out;
    return with_scratch("mamdr_score_sums", score_workspace_bytes(n), s, [&](char* ws) {
        a.part = reinterpret_cast<double*>(ws);
        launch_score_sums(a, s);
        return hipGetLastError();
    });
}

// ---- what top-K lists are made of: id counts and intra-list similarity (list_kernels.hip)
int mamdr_id_counts(const int32_t* d_ids, const float* d_label, int64_t n, int64_t n_bins, uint32_t* d_counts, void* stream) {
    if (!d_counts) return fail(MAMDR_EINVAL, "mamdr_id_counts: null counts pointer");
    if (n < 0 || n >= ((int64_t)1 << 32)) return fail(MAMDR_EINVAL, "mamdr_id_counts: n %lld outside [0, 2^32)", (long long)n);
    if (n_bins <= 0) return fail(MAMDR_EINVAL, "mamdr_id_counts: n_bins %lld is not positive", (long long)n_bins);
    if (n > 0 && !d_ids) return fail(MAMDR_EINVAL, "mamdr_id_counts: null ids pointer");
    if (misaligned(3, d_ids, d_label, d_counts))
        return fail(MAMDR_EINVAL, "mamdr_id_counts: a pointer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_bins * sizeof(uint32_t), s));
    if (n == 0) return MAMDR_OK;
    IdCountArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.label = d_label;
    a.n = n;
    a.n_bins = n_bins;
    a.counts = d_counts;
    launch_id_counts(a, s);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_list_similarity(const int32_t* d_ids, int32_t n_list, int32_t k, const float* d_rows, int64_t n_rows, int32_t emb_dim,
                          double* d_sim_sum, int32_t* d_pairs, void* stream) {
    if (!d_ids || !d_rows || !d_sim_sum || !d_pairs)
        return fail(MAMDR_EINVAL, "mamdr_list_similarity: null ids / rows / sim_sum / pairs pointer");
    if (n_list <= 0) return fail(MAMDR_EINVAL, "mamdr_list_similarity: n_list %d is not positive", (int)n_list);
    if (k < 1 || k > MAMDR_LIST_MAX_K)
        return fail(MAMDR_EINVAL, "mamdr_list_similarity: k %d outside 1..%d", (int)k, MAMDR_LIST_MAX_K);
    if (emb_dim != 32 && emb_dim != 64 && emb_dim != 128 && emb_dim != 256)
        return fail(MAMDR_EINVAL, "mamdr_list_similarity: emb_dim %d is not 32, 64, 128 or 256", (int)emb_dim);
    if (n_rows <= 0) return fail(MAMDR_EINVAL, "mamdr_list_similarity: n_rows %lld is not positive", (long long)n_rows);
    if (misaligned(3, d_ids, d_pairs) || misaligned(7, d_sim_sum) || misaligned(15, d_rows))
        return fail(MAMDR_EINVAL, "mamdr_list_similarity: a pointer is not aligned (ids / pairs 4, sim_sum 8, rows 16 bytes)");
    ListSimArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.n_list = n_list;
    a.k = k;
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.emb_dim = emb_dim;
    a.sim_sum = d_sim_sum;
    a.pairs = d_pairs;
    launch_list_sim(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

// ---- greedy MMR re-ranking of candidate lists (diversify_kernels.hip)
int mamdr_list_diversify(const int32_t* d_ids, const float* d_rel, int32_t n_list, int32_t n, int32_t k, float lambda,
                         const float* d_rows, int64_t n_rows, int32_t emb_dim, int32_t* d_pos_out, float* d_value_out,
                         void* stream) {
    if (!d_ids || !d_rel || !d_rows || !d_pos_out)
        return fail(MAMDR_EINVAL, "mamdr_list_diversify: null ids / rel / rows / pos_out pointer");
    if (n_list <= 0) return fail(MAMDR_EINVAL, "mamdr_list_diversify: n_list %d is not positive", (int)n_list);
    if (n < 1 || n > MAMDR_LIST_MAX_K)
        return fail(MAMDR_EINVAL, "mamdr_list_diversify: n %d outside 1..%d", (int)n, MAMDR_LIST_MAX_K);
    if (k < 1 || k > n) return fail(MAMDR_EINVAL, "mamdr_list_diversify: k %d outside 1..n = %d", (int)k, (int)n);
    if (!(lambda >= 0.f && lambda <= 1.f))
        return fail(MAMDR_EINVAL, "mamdr_list_diversify: lambda %g outside [0, 1]", (double)lambda);
    if (emb_dim != 32 && emb_dim != 64 && emb_dim != 128 && emb_dim != 256)
        return fail(MAMDR_EINVAL, "mamdr_list_diversify: emb_dim %d is not 32, 64, 128 or 256", (int)emb_dim);
    if (n_rows <= 0) return fail(MAMDR_EINVAL, "mamdr_list_diversify: n_rows %lld is not positive", (long long)n_rows);
    if (misaligned(3, d_ids, d_rel, d_pos_out, d_value_out) || misaligned(15, d_rows))
        return fail(MAMDR_EINVAL, "mamdr_list_diversify: a pointer is not aligned (ids / rel / pos_out / value_out 4, rows 16 bytes)");
    ListDivArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_ids;
    a.rel = d_rel;
    a.n_list = n_list;
    a.n = n;
    a.k = k;
    a.lambda = lambda;
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.emb_dim = emb_dim;
    a.pos_out = d_pos_out;
    a.value_out = d_value_out;
    launch_list_div(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

// ---- exact cosine nearest neighbours of table rows (knn_kernels.hip)
constexpr int64_t KNN_DEFAULT_CHUNK = (int64_t)1 << 20;     // candidates of a pass of the plain call
constexpr int KNN_GRID_TARGET = 256;                         // workgroups the tile kernel aims at: one per CU
constexpr int KNN_MAX_SPLITS = 64;

static int row_neighbours(const char* fn, const float* d_rows, int64_t n_rows, int32_t emb_dim, const int32_t* d_query,
                          int32_t n_query, const int32_t* d_cand, int64_t n_cand, int32_t exclude_self, int32_t k,
                          int32_t* d_ids_out, float* d_sim_out, int64_t chunk, void* stream) {
    if (!d_rows || !d_query || !d_ids_out || !d_sim_out)
        return fail(MAMDR_EINVAL, "%s: null d_rows / d_query / d_ids_out / d_sim_out pointer", fn);
    if (misaligned(15, d_rows)) return fail(MAMDR_EINVAL, "%s: d_rows is not 16-byte aligned", fn);
    if (misaligned(3, d_query, d_cand, d_ids_out, d_sim_out))
        return fail(MAMDR_EINVAL, "%s: d_query / d_cand / d_ids_out / d_sim_out is not 4-byte aligned", fn);
    if (n_rows <= 0 || n_rows > INT32_MAX) return fail(MAMDR_EINVAL, "%s: n_rows %lld outside [1, 2^31)", fn, (long long)n_rows);
    if (emb_dim != 32 && emb_dim != 64 && emb_dim != 128 && emb_dim != 256)
        return fail(MAMDR_EINVAL, "%s: emb_dim %d is not 32, 64, 128 or 256", fn, (int)emb_dim);
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d is not positive", fn, (int)n_query);
    if (n_cand <= 0) return fail(MAMDR_EINVAL, "%s: n_cand %lld is not positive", fn, (long long)n_cand);
    if (!d_cand && n_cand != n_rows)
        return fail(MAMDR_EINVAL, "%s: n_cand %lld with a null d_cand (every row: n_cand = n_rows = %lld)", fn, (long long)n_cand,
                    (long long)n_rows);
    if (k < 1 || k > MAMDR_KNN_MAX_K) return fail(MAMDR_EINVAL, "%s: k %d outside 1..%d", fn, (int)k, MAMDR_KNN_MAX_K);
    if (chunk <= 0) return fail(MAMDR_EINVAL, "%s: chunk %lld is not positive", fn, (long long)chunk);
    static_assert(KNN_MAX_K == MAMDR_KNN_MAX_K, "the running lists hold the longest list");
    hipStream_t s = (hipStream_t)stream;
    chunk = (chunk + KNN_TILE - 1) / KNN_TILE * KNN_TILE;
    if (chunk > n_cand) chunk = (n_cand + KNN_TILE - 1) / KNN_TILE * KNN_TILE;
    const int64_t q_blocks = ((int64_t)n_query + KNN_QBLOCK - 1) / KNN_QBLOCK, tiles = chunk / KNN_TILE;
    int64_t splits = KNN_GRID_TARGET / q_blocks;
    if (splits > KNN_MAX_SPLITS) splits = KNN_MAX_SPLITS;
    if (splits > tiles) splits = tiles;
    if (splits < 1) splits = 1;
    KnnArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.emb_dim = emb_dim;
    a.query = d_query;
    a.n_query = n_query;
    a.cand = d_cand;
    a.exclude_self = exclude_self != 0;
    a.k = k;
    a.splits = (int)splits;
    a.ids_out = d_ids_out;
    a.sim_out = d_sim_out;
    // the scratch: [running lists | query norms | candidate norms of a pass]
    const size_t best_bytes = (size_t)q_blocks * KNN_QBLOCK * splits * KNN_MAX_K * sizeof(unsigned long long);
    const size_t qn_bytes = ((size_t)n_query * sizeof(float) + 15) / 16 * 16;
    bool lds_ok = true;
    const int rc = with_scratch(fn, best_bytes + qn_bytes + (size_t)chunk * sizeof(float), s, [&](char* ws) {
        a.best = reinterpret_cast<unsigned long long*>(ws);
        a.qn2 = reinterpret_cast<float*>(ws + best_bytes);
        a.cn2 = reinterpret_cast<float*>(ws + best_bytes + qn_bytes);
        launch_knn_query_norms(a, s);
        for (int64_t c0 = 0; c0 < n_cand; c0 += chunk) {
            a.c_base = c0;
            a.n_chunk = (int)(n_cand - c0 < chunk ? n_cand - c0 : chunk);
            a.first_chunk = c0 == 0;
            launch_knn_cand_norms(a, s);
            if (!launch_knn_tile(a, s)) {
                lds_ok = false;
                return hipGetLastError();
            }
        }
        launch_knn_merge(a, s);
        return hipGetLastError();
    });
    if (rc == MAMDR_OK && !lds_ok) return fail(MAMDR_EHIP, "%s: the tile kernel's LDS was refused", fn);
    return rc;
}

int mamdr_row_neighbours(const float* d_rows, int64_t n_rows, int32_t emb_dim, const int32_t* d_query, int32_t n_query,
                         const int32_t* d_cand, int64_t n_cand, int32_t exclude_self, int32_t k, int32_t* d_ids_out,
                         float* d_sim_out, void* stream) {
    return row_neighbours("mamdr_row_neighbours", d_rows, n_rows, emb_dim, d_query, n_query, d_cand, n_cand, exclude_self, k,
                          d_ids_out, d_sim_out, KNN_DEFAULT_CHUNK, stream);
}
int mamdr_row_neighbours_bounded(const float* d_rows, int64_t n_rows, int32_t emb_dim, const int32_t* d_query,
                                 int32_t n_query, const int32_t* d_cand, int64_t n_cand, int32_t exclude_self, int32_t k,
                                 int32_t* d_ids_out, float* d_sim_out, int32_t chunk, void* stream) {
    return row_neighbours("mamdr_row_neighbours_bounded", d_rows, n_rows, emb_dim, d_query, n_query, d_cand, n_cand,
                          exclude_self, k, d_ids_out, d_sim_out, chunk, stream);
}

// ---- baselines: item co-occurrence, ItemKNN scores, ranks and top-K lists from a score matrix (baseline_kernels.hip)
static int check_histories(const char* fn, const int64_t* d_hist_off, const int32_t* d_hist_pos, int64_t nnz, int32_t n_user,
                           int32_t m, int64_t max_user) {
    if (!d_hist_off) return fail(MAMDR_EINVAL, "%s: null d_hist_off pointer", fn);
    if (nnz < 0) return fail(MAMDR_EINVAL, "%s: nnz %lld is negative", fn, (long long)nnz);
    if (nnz > 0 && !d_hist_pos) return fail(MAMDR_EINVAL, "%s: null d_hist_pos pointer with nnz %lld", fn, (long long)nnz);
    if (misaligned(7, d_hist_off) || misaligned(3, d_hist_pos))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned (d_hist_off 8, the others 4 bytes)", fn);
    if (m <= 0 || m > BASE_MAX_ITEMS) return fail(MAMDR_EINVAL, "%s: m %d outside 1..%d", fn, (int)m, BASE_MAX_ITEMS);
    if (n_user <= 0 || n_user >= max_user)
        return fail(MAMDR_EINVAL, "%s: n_user %d outside [1, %lld)", fn, (int)n_user, (long long)max_user);
    return MAMDR_OK;
}

int mamdr_item_cooc(const int64_t* d_hist_off, const int32_t* d_hist_pos, int64_t nnz, int32_t n_user, int32_t m,
                    uint32_t* d_cooc, void* stream) {
    if (!d_cooc) return fail(MAMDR_EINVAL, "mamdr_item_cooc: null d_cooc pointer");
    if (misaligned(3, d_cooc)) return fail(MAMDR_EINVAL, "mamdr_item_cooc: a pointer is not aligned (d_hist_off 8, the others 4 bytes)");
    if (const int rc = check_histories("mamdr_item_cooc", d_hist_off, d_hist_pos, nnz, n_user, m, (int64_t)1 << 31)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_cooc, 0, (size_t)m * m * sizeof(uint32_t), s));
    HistArgs a;
    memset(&a, 0, sizeof(a));
    a.hist_off = d_hist_off;
    a.hist_pos = d_hist_pos;
    a.nnz = nnz;
    a.n_user = n_user;
    a.m = m;
    a.cooc = d_cooc;
    if (nnz > 0) launch_item_cooc(a, s);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_history_scores(const uint32_t* d_cooc, int32_t m, const int64_t* d_hist_off, const int32_t* d_hist_pos,
                         int64_t nnz, int32_t n_user, const int32_t* d_query, int32_t n_query, float shrink,
                         float* d_scores, void* stream) {
    const char* fn = "mamdr_history_scores";
    if (!d_cooc || !d_query || !d_scores) return fail(MAMDR_EINVAL, "%s: null d_cooc / d_query / d_scores pointer", fn);
    if (misaligned(3, d_cooc, d_query, d_scores))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned (d_hist_off 8, the others 4 bytes)", fn);
    if (const int rc = check_histories(fn, d_hist_off, d_hist_pos, nnz, n_user, m, (int64_t)1 << 24)) return rc;
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d is not positive", fn, (int)n_query);
    if (!(shrink >= 0.f && shrink <= 1048576.f)) return fail(MAMDR_EINVAL, "%s: shrink %g outside [0, 2^20]", fn, (double)shrink);
    HistArgs a;
    memset(&a, 0, sizeof(a));
    a.hist_off = d_hist_off;
    a.hist_pos = d_hist_pos;
    a.nnz = nnz;
    a.n_user = n_user;
    a.m = m;
    a.cooc = const_cast<uint32_t*>(d_cooc);
    a.query = d_query;
    a.n_query = n_query;
    a.shrink = shrink;
    a.scores = d_scores;
    a.vec4 = m % 4 == 0 && !misaligned(15, d_cooc, d_scores);
    // (one workgroup per query and column tile, in one grid dimension)
    const int64_t tiles = ((int64_t)m + (a.vec4 ? 1024 : 256) - 1) / (a.vec4 ? 1024 : 256);
    if ((int64_t)n_query * tiles > INT32_MAX)
        return fail(MAMDR_EINVAL, "%s: n_query %d x %lld column tiles exceed one grid: score in blocks of queries", fn,
                    (int)n_query, (long long)tiles);
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(fn, (size_t)m * sizeof(float), s, [&](char* ws) {
        a.root = reinterpret_cast<float*>(ws);
        launch_hist_scores(a, s);
        return hipGetLastError();
    });
}

static int check_score_call(const char* fn, const float* d_scores, int64_t row_stride, int32_t n_query, const int32_t* d_cand,
                            int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, int64_t per_tile) {
    if (!d_scores) return fail(MAMDR_EINVAL, "%s: null d_scores pointer", fn);
    if (misaligned(3, d_scores, d_cand, d_excl_ids) || misaligned(7, d_excl_off))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned (the offsets 8, the others 4 bytes)", fn);
    if ((d_excl_off == nullptr) != (d_excl_ids == nullptr))
        return fail(MAMDR_EINVAL, "%s: the exclusion lists need both their offsets and their ids", fn);
    if (n_query <= 0) return fail(MAMDR_EINVAL, "%s: n_query %d is not positive", fn, (int)n_query);
    if (n_cand <= 0 || n_cand > INT32_MAX) return fail(MAMDR_EINVAL, "%s: n_cand %lld outside [1, 2^31)", fn, (long long)n_cand);
    if (row_stride < 0 || (row_stride > 0 && row_stride < n_cand))
        return fail(MAMDR_EINVAL, "%s: row_stride %lld is neither 0 nor at least n_cand = %lld", fn, (long long)row_stride,
                    (long long)n_cand);
    if ((int64_t)n_query * ((n_cand + per_tile - 1) / per_tile) > INT32_MAX)
        return fail(MAMDR_EINVAL, "%s: n_query %d x n_cand %lld exceed one grid: rank in blocks of queries", fn, (int)n_query,
                    (long long)n_cand);
    return MAMDR_OK;
}

int mamdr_rank_scores(const float* d_scores, int64_t row_stride, int32_t n_query, const int32_t* d_cand, int64_t n_cand,
                      const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                      const int32_t* d_tgt_ids, int64_t n_tgt, int32_t* d_rank_out, float* d_score_out,
                      int32_t* d_live_out, void* stream) {
    const char* fn = "mamdr_rank_scores";
    if (!d_tgt_off || !d_live_out) return fail(MAMDR_EINVAL, "%s: null d_tgt_off / d_live_out pointer", fn);
    if (n_tgt < 0) return fail(MAMDR_EINVAL, "%s: n_tgt %lld is negative", fn, (long long)n_tgt);
    if (n_tgt > 0 && (!d_tgt_ids || !d_rank_out)) return fail(MAMDR_EINVAL, "%s: null d_tgt_ids / d_rank_out pointer with targets", fn);
    if (misaligned(3, d_tgt_ids, d_rank_out, d_score_out, d_live_out) || misaligned(7, d_tgt_off))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned (the offsets 8, the others 4 bytes)", fn);
    if (const int rc = check_score_call(fn, d_scores, row_stride, n_query, d_cand, n_cand, d_excl_off, d_excl_ids, 1024)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_tgt > 0) HIP_TRY(hipMemsetAsync(d_rank_out, 0, (size_t)n_tgt * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(d_live_out, 0, (size_t)n_query * sizeof(int32_t), s));
    ScoreRankArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = d_scores;
    a.row_stride = row_stride;
    a.n_query = n_query;
    a.cand = d_cand;
    a.n_cand = (int)n_cand;
    a.excl_off = d_excl_off;
    a.excl_ids = d_excl_ids;
    a.tgt_off = d_tgt_off;
    a.tgt_ids = d_tgt_ids;
    a.n_tgt = n_tgt;
    a.rank_out = d_rank_out;
    a.score_out = d_score_out;
    a.live_out = d_live_out;
    launch_rank_scores(a, s);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

int mamdr_topk_scores(const float* d_scores, int64_t row_stride, int32_t n_query, const int32_t* d_cand, int64_t n_cand,
                      const int64_t* d_excl_off, const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out,
                      float* d_scores_out, void* stream) {
    const char* fn = "mamdr_topk_scores";
    if (!d_ids_out || !d_scores_out) return fail(MAMDR_EINVAL, "%s: null d_ids_out / d_scores_out pointer", fn);
    if (misaligned(3, d_ids_out, d_scores_out))
        return fail(MAMDR_EINVAL, "%s: a pointer is not aligned (the offsets 8, the others 4 bytes)", fn);
    if (const int rc = check_score_call(fn, d_scores, row_stride, n_query, d_cand, n_cand, d_excl_off, d_excl_ids, INT32_MAX)) return rc;
    if (k < 1 || k > MAMDR_SCORES_MAX_K) return fail(MAMDR_EINVAL, "%s: k %d outside 1..%d", fn, (int)k, MAMDR_SCORES_MAX_K);
    static_assert(BASE_MAX_K == MAMDR_SCORES_MAX_K, "the running list holds the longest list");
    ScoreRankArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = d_scores;
    a.row_stride = row_stride;
    a.n_query = n_query;
    a.cand = d_cand;
    a.n_cand = (int)n_cand;
    a.excl_off = d_excl_off;
    a.excl_ids = d_excl_ids;
    a.k = k;
    a.ids_out = d_ids_out;
    a.topk_out = d_scores_out;
    launch_topk_scores(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return MAMDR_OK;
}

}  // extern "C"
