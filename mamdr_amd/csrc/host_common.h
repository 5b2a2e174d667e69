// Host-side pieces the two engines share (the step kernels' C ABI in mamdr_api.hip and its sibling files, the
// generic-layer engine in graph_engine.hip): the bound data columns, the error buffer behind *_last_error, the record of a
// context's device allocations, the two host-computed tables (AUC thresholds, TF's running beta powers) and the argument
// checks both C-ABI front ends make with the same texts; and WsCursor, with which the launchers of the evaluation kernel
// files (exact, isotonic, bootstrap) lay out a call's workspace.  Host code only: nothing here runs in a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_base.h"      // ErrBuf, misaligned, the retrieval sizes: the HIP-free part

namespace mamdr {

// the columns of one (domain, split) as bound by *_bind_domain_data
struct SplitData {
    const int32_t* uid = nullptr;
    const int32_t* pid = nullptr;
    const int32_t* dom = nullptr;
    const float* label = nullptr;
    int64_t n = 0;
    bool bound = false;     // an EMPTY split (n = 0, null columns) is bound too: a pass over it has no steps
};

// a failing HIP call ends the calling function with MAMDR_EHIP and the call's text in `err` (each engine forwards its own
// one-argument macro here, stringising the call before any macro in it expands)
#define MAMDR_HIP_TRY(err, expr, text)                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return (err).fail(MAMDR_EHIP, "%s: %s", text, hipGetErrorString(e_)); \
    } while (0)

// every device allocation of a context: what its destroy frees.  After the first failure nothing more is allocated; the
// caller asks once, after its last alloc (check, or `err` itself)
struct DevAllocs {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    size_t err_bytes = 0;       // the size that failed
    template <typename T>
    void alloc(T** p, size_t count) {
        if (err != hipSuccess) return;
        err = hipMalloc((void**)p, count * sizeof(T));
        if (err == hipSuccess) ptrs.push_back(*p);
        else err_bytes = count * sizeof(T);
    }
    // MAMDR_OK, or MAMDR_EHIP with the first failure since the last call explained in `e` -- and cleared: a buffer that
    // failed to grow may be asked for again
    int check(ErrBuf& e) {
        if (err == hipSuccess) return MAMDR_OK;
        const hipError_t was = err;
        err = hipSuccess;
        return e.fail(MAMDR_EHIP, "hipMalloc(%zu): %s", err_bytes, hipGetErrorString(was));
    }
    // a buffer that grows on demand gives its old allocation back (null: nothing to do)
    void release(void* p) {
        if (!p) return;
        ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end());
        (void)hipFree(p);
    }
    void free_all() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// a device buffer that grows on demand: at least n elements after grow().  A failed grow leaves no buffer (the old one is
// gone, cap = 0) and the error in `err`; a later call may ask again
template <typename T>
struct GrowBuf {
    T* p = nullptr;
    size_t cap = 0;
    int grow(DevAllocs& dev, ErrBuf& err, size_t n) {
        if (n <= cap) return MAMDR_OK;
        dev.release(p);
        p = nullptr;
        cap = 0;
        dev.alloc(&p, n);
        if (const int rc = dev.check(err)) return rc;
        cap = n;
        return MAMDR_OK;
    }
};

// the stream side of both engines' retrieval backends (retrieval_host.h): n int64 read back and waited for; a fill
struct RetStream {
    hipStream_t stream;
    ErrBuf& err;
    int read_back(int64_t* host, const int64_t* dev, size_t n) {
        MAMDR_HIP_TRY(err, hipMemcpyAsync(host, dev, n * sizeof(int64_t), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(offsets)");
        MAMDR_HIP_TRY(err, hipStreamSynchronize(stream), "hipStreamSynchronize(stream)");
        return MAMDR_OK;
    }
    int fill(void* dev, int byte, size_t bytes) {
        MAMDR_HIP_TRY(err, hipMemsetAsync(dev, byte, bytes, stream), "hipMemsetAsync(dev, byte, bytes, stream)");
        return MAMDR_OK;
    }
};

// carves one workspace allocation into parts: take(bytes) is where the part starts, `at` the bytes used so far.  Every part
// starts 16-byte aligned (given an aligned base and start)
struct WsCursor {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    }
};

// the 500 AUC thresholds each context uploads once: -1e-7, i / 499, 1 + 1e-7
inline void auc_thresholds(float thr[500]) {
    thr[0] = (float)(0.0 - 1e-7);
    for (int i = 0; i < 498; ++i) thr[i + 1] = (float)((double)(i + 1) * 1.0 / (double)(500 - 1));
    thr[499] = (float)(1.0 + 1e-7);
}

// TF's running beta powers after `steps` Adam steps: one fp32 rounding per step, as the step loops form them
inline void tf_beta_powers(float beta1, float beta2, int64_t steps, float* b1p, float* b2p) {
    float b1 = 1.0f, b2 = 1.0f;
    for (int64_t t = 0; t < steps; ++t) {
        const float n1 = b1 * beta1, n2 = b2 * beta2;
        // both products at a fixed point: every further step leaves them as they are.  0.9 / 0.999 end on denormal fixed
        // points (4 and 500 x 2^-149) after ~1,000 / ~1.6e5 steps; beta = 1 keeps the product at 1 from the start
        if (n1 == b1 && n2 == b2) break;
        b1 = n1;
        b2 = n2;
    }
    *b1p = b1;
    *b2p = b2;
}

// ---- argument checks of both C ABIs (MAMDR_OK or the code that `err` now explains)
inline int check_state_ptrs(ErrBuf& err, const float* p, const float* m, const float* v) {
    if (!p || !m || !v) return err.fail(MAMDR_EINVAL, "null state pointer");
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) return err.fail(MAMDR_EINVAL, "state pointers must be 16-byte aligned");
    return MAMDR_OK;
}
// *_bind_table: frozen tables only, an aligned pointer, the user or the item table with the row count of the config
inline int check_bind_table(ErrBuf& err, bool trainable, int seg, const float* d_rows, int64_t n_rows, int n_user, int n_item) {
    if (trainable) return err.fail(MAMDR_ESTATE, "tables are trainable: they live in the flat vector");
    if (!d_rows || ((uintptr_t)d_rows & 15)) return err.fail(MAMDR_EINVAL, "table pointer null or not 16-byte aligned");
    if (seg == MAMDR_SEG_USER_EMB) {
        if (n_rows != n_user) return err.fail(MAMDR_EINVAL, "user table has %lld rows, config says %d", (long long)n_rows, n_user);
    } else if (seg == MAMDR_SEG_ITEM_EMB) {
        if (n_rows != n_item) return err.fail(MAMDR_EINVAL, "item table has %lld rows, config says %d", (long long)n_rows, n_item);
    } else {
        return err.fail(MAMDR_EINVAL, "segment %d is not a bindable table", seg);
    }
    return MAMDR_OK;
}
// *_bind_domain_data: `d` is the context's slot of (domain, split), null when either is out of range
inline int bind_columns(ErrBuf& err, SplitData* d, int domain, int split, const int32_t* d_uid, const int32_t* d_pid,
                        const int32_t* d_domain, const float* d_label, int64_t n_rows) {
    if (!d) return err.fail(MAMDR_EINVAL, "domain %d / split %d out of range", domain, split);
    if (n_rows < 0 || n_rows > 0x7fffffff) return err.fail(MAMDR_EINVAL, "n_rows out of range");
    if (n_rows > 0 && (!d_uid || !d_pid || !d_domain || !d_label)) return err.fail(MAMDR_EINVAL, "null column pointer");
    d->bound = true;
    d->uid = d_uid;
    d->pid = d_pid;
    d->dom = d_domain;
    d->label = d_label;
    d->n = n_rows;
    return MAMDR_OK;
}
// *_train_steps_n, first half: the split, the batch, the optimiser and the pass (*pass_rows < 0: the whole split)
inline int check_train_call(ErrBuf& err, const SplitData* d, int domain, int32_t batch, int32_t max_batch, int32_t optimizer,
                            const float* accum, const char* bind_accumulator, int64_t first_step, int64_t n_steps,
                            int64_t* pass_rows) {
    if (!d || !d->bound) return err.fail(MAMDR_ESTATE, "train split of domain %d is not bound", domain);
    if (batch <= 0 || batch > max_batch) return err.fail(MAMDR_EINVAL, "batch %d outside (0, max_batch=%d]", batch, max_batch);
    if (optimizer != MAMDR_OPT_ADAM && optimizer != MAMDR_OPT_SGD && optimizer != MAMDR_OPT_ACCUMULATE)
        return err.fail(MAMDR_EINVAL, "unknown optimizer %d", optimizer);
    if (optimizer == MAMDR_OPT_ACCUMULATE && !accum)
        return err.fail(MAMDR_ESTATE, "MAMDR_OPT_ACCUMULATE needs %s first", bind_accumulator);
    if (first_step < 0 || n_steps < 0) return err.fail(MAMDR_EINVAL, "negative step range");
    if (*pass_rows < 0) *pass_rows = d->n;
    if (*pass_rows > d->n) return err.fail(MAMDR_EINVAL, "pass of %lld rows exceeds the %lld rows of domain %d",
                                           (long long)*pass_rows, (long long)d->n, domain);
    return MAMDR_OK;
}
// ... second half (the generic-layer engine asks for the pass's permutation in between): the steps lie inside the pass
inline int check_step_range(ErrBuf& err, int domain, int64_t pass_rows, int32_t batch, int64_t first_step, int64_t n_steps) {
    const int64_t pass_steps = (pass_rows + batch - 1) / batch;
    if (first_step + n_steps > pass_steps)
        return err.fail(MAMDR_EINVAL, "steps [%lld,%lld) exceed the %lld batches of domain %d", (long long)first_step,
                        (long long)(first_step + n_steps), (long long)pass_steps, domain);
    return MAMDR_OK;
}

}  // namespace mamdr
