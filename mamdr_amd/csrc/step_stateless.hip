// C ABI of libmamdr_hip.so, the entry points that hold no state of their own: the outer updates of the meta loops (the one
// that advances a context's live weights among them), Adam on a caller's vectors, the PCGrad projection, the copy, the fp64
// Gram matrices (mamdr_gram) and the host-side shuffle order.
#include <cmath>

#include "step_ctx.h"

extern "C" {

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
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MAMDR_OK;
}

// ---- fp64 Gram matrices of flat vectors over column ranges (gram_kernels.hip)
static_assert(MAMDR_GRAM_SLAB == GRAM_SLAB && MAMDR_GRAM_MAX_VEC == GRAM_MAX_VEC, "include/mamdr_hip.h and mamdr_kernels.h agree");
// the checks mamdr_gram_work and mamdr_gram share (n_cols < 0: the vectors' length is not known); *slabs = slabs of all ranges
static int gram_check(const char* fn, int32_t n_vec, int64_t n_cols, const int64_t* h_off, const int64_t* h_count,
                      int32_t n_range, int64_t* slabs) {
    if (n_vec < 1 || n_vec > GRAM_MAX_VEC) return fail(MAMDR_EINVAL, "%s: n_vec %d outside [1, %d]", fn, n_vec, GRAM_MAX_VEC);
    if (n_range < 0 || (n_range > 0 && (!h_off || !h_count)))
        return fail(MAMDR_EINVAL, "%s: n_range %d / null h_off or h_count", fn, n_range);
    *slabs = 0;
    for (int32_t r = 0; r < n_range; ++r) {
        if (h_off[r] < 0 || h_count[r] < 0 || h_count[r] > INT64_MAX - h_off[r] || (n_cols >= 0 && h_off[r] + h_count[r] > n_cols))
            return fail(MAMDR_EINVAL, "%s: range %d (h_off %lld, h_count %lld) is negative or outside the %lld columns", fn, r,
                        (long long)h_off[r], (long long)h_count[r], (long long)n_cols);
        *slabs += (h_count[r] + GRAM_SLAB - 1) / GRAM_SLAB;
    }
    return MAMDR_OK;
}
int64_t mamdr_gram_work(int32_t n_vec, const int64_t* h_off, const int64_t* h_count, int32_t n_range) {
    int64_t slabs = 0;
    if (const int rc = gram_check("mamdr_gram_work", n_vec, -1, h_off, h_count, n_range, &slabs)) return rc;
    return slabs * n_vec * n_vec;
}
int mamdr_gram(const float* d_vecs, int64_t stride, int32_t n_vec, int64_t n_cols, const int64_t* h_off, const int64_t* h_count,
               int32_t n_range, double* d_work, int64_t work_doubles, double* d_out, void* stream) {
    const char* fn = "mamdr_gram";
    if (n_cols < 0 || stride < n_cols) return fail(MAMDR_EINVAL, "%s: n_cols %lld negative or above stride %lld", fn, (long long)n_cols, (long long)stride);
    int64_t slabs = 0;
    if (const int rc = gram_check(fn, n_vec, n_cols, h_off, h_count, n_range, &slabs)) return rc;
    if (n_range == 0) return MAMDR_OK;
    if (!d_out || ((uintptr_t)d_out & 7)) return fail(MAMDR_EINVAL, "%s: d_out is null or not 8-byte aligned", fn);
    if (slabs > 0) {
        if (!d_vecs || ((uintptr_t)d_vecs & 3)) return fail(MAMDR_EINVAL, "%s: d_vecs is null or not 4-byte aligned", fn);
        if (work_doubles < slabs * n_vec * n_vec)
            return fail(MAMDR_EINVAL, "%s: work_doubles %lld below the %lld of mamdr_gram_work", fn, (long long)work_doubles,
                        (long long)(slabs * n_vec * n_vec));
        if (!d_work || ((uintptr_t)d_work & 7)) return fail(MAMDR_EINVAL, "%s: d_work is null or not 8-byte aligned", fn);
        if (slabs > 0x7fffffff) return fail(MAMDR_EINVAL, "%s: %lld slabs exceed one grid", fn, (long long)slabs);
    }
    GramArgs a;
    memset(&a, 0, sizeof(a));
    a.vecs = d_vecs;
    a.stride = stride;
    a.n_vec = n_vec;
    a.work = d_work;
    a.out = d_out;
    for (int32_t r0 = 0; r0 < n_range; r0 += GRAM_MAX_RANGES) {
        a.n_range = std::min<int32_t>(GRAM_MAX_RANGES, n_range - r0);
        a.out_first = r0;
        for (int r = 0; r < a.n_range; ++r) {
            a.off[r] = h_off[r0 + r];
            a.count[r] = h_count[r0 + r];
            a.first[r + 1] = a.first[r] + (a.count[r] + GRAM_SLAB - 1) / GRAM_SLAB;
        }
        launch_gram(a, (hipStream_t)stream);
        a.work_first += a.first[a.n_range];
    }
    HIP_TRY(hipGetLastError());
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

}  // extern "C"
