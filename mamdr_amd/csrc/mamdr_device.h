// Device-side helpers shared by the MAMDR gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mamdr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- fixed architecture of the hot path (model_zoo/DeepCTR/deepctr.py:95-136 with
//      the BASELINE configs: three 128-d embeddings -> 384 -> 256 -> 128 -> 64 -> 1)
constexpr int EMB = 128;
constexpr int XDIM = 3 * EMB;   // 384
constexpr int H1 = 256;
constexpr int H2 = 128;
constexpr int H3 = 64;
constexpr int ACT_LD = XDIM + H1 + H2 + H3;   // 832: [x | h1 | h2 | h3] per row
constexpr int DZ_LD = H1 + H2 + H3;           // 448: [dz1 | dz2 | dz3] per row
constexpr int TILE_ROWS = 16;                 // batch rows per workgroup in the step kernel
// transposed copies of W1 / W2 for the 4-row tower's backward layers (workspace, kept by k_update)
constexpr int W1T_OFF = 0;                    // [128][256]
constexpr int W2T_OFF = H1 * H2;              // [64][128]
constexpr int W0T_OFF = H1 * H2 + H2 * H3;    // [256][256]: W0[0:256, :]^T (user | item rows), trainable tables only
constexpr int WT_FLOATS = H1 * H2 + H2 * H3 + 2 * EMB * H1;

// dense block of the flat trainable vector, relative to the domain table start
// (DeepFM appends its 1-d linear table of the domain feature, `ld`, behind the global bias)
// (uncertainty weighting appends one trainable scalar per domain, `lv`, at the very end)
// (PNN appends the three rows of its first kernel that the field pairs' inner products feed, `wx` [3][H1], at the end:
// W0 itself keeps its [XDIM][H1] place, so every contraction of the mlp tower reads the same addresses)
struct DenseLayout {
    int dm, w0, w1, w2, b0, b1, b2, wo, gb, ld, ld_count, lv, lv_count, wx, wx_count, count, alloc;
    __host__ __device__ static DenseLayout make(int n_domain, bool deepfm = false, bool uncertainty = false, bool pnn = false) {
        DenseLayout L;
        L.dm = 0;
        L.w0 = n_domain * EMB;
        L.w1 = L.w0 + XDIM * H1;
        L.w2 = L.w1 + H1 * H2;
        L.b0 = L.w2 + H2 * H3;
        L.b1 = L.b0 + H1;
        L.b2 = L.b1 + H2;
        L.wo = L.b2 + H3;
        L.gb = L.wo + H3;
        L.ld = L.gb + 1;
        L.ld_count = deepfm ? n_domain : 0;
        L.lv = L.ld + L.ld_count;
        L.lv_count = uncertainty ? n_domain : 0;
        L.wx = (L.lv + L.lv_count + 3) & ~3;        // (16-B aligned rows)
        L.wx_count = pnn ? 3 * H1 : 0;
        L.count = pnn ? L.wx + L.wx_count : L.lv + L.lv_count;
        L.alloc = (L.count + 3) & ~3;
        return L;
    }
};

// Star tower (model_zoo/Star): block of the flat trainable vector behind the (optional) tables.
// The meta parameters of the reference's name filter ("emb", "kernel_shared", "bias_shared",
// config/Taobao-10/star_taobao.json:37-41) come first, so theta / phi are a prefix of the vector.
struct StarLayout {
    int dm, ws[3], bs[3], n_meta;
    int pgs, pbs, pgd, pbd;        // PartitionedNorm gamma / beta: shared [384], specific [D][384]
    int wd[3], bd[3];              // specific kernels [D][in*out] and biases [D][out]
    int wo, gb, count, alloc;
    __host__ __device__ static int ksize(int l) { return l == 0 ? XDIM * H1 : (l == 1 ? H1 * H2 : H2 * H3); }
    __host__ __device__ static int bsize(int l) { return l == 0 ? H1 : (l == 1 ? H2 : H3); }
    __host__ __device__ static StarLayout make(int n_domain) {
        StarLayout S;
        int o = 0;
        S.dm = o; o += n_domain * EMB;
        for (int l = 0; l < 3; ++l) { S.ws[l] = o; o += ksize(l); }
        for (int l = 0; l < 3; ++l) { S.bs[l] = o; o += bsize(l); }
        S.n_meta = o;
        S.pgs = o; o += XDIM;
        S.pbs = o; o += XDIM;
        S.pgd = o; o += n_domain * XDIM;
        S.pbd = o; o += n_domain * XDIM;
        for (int l = 0; l < 3; ++l) { S.wd[l] = o; o += n_domain * ksize(l); }
        for (int l = 0; l < 3; ++l) { S.bd[l] = o; o += n_domain * bsize(l); }
        S.wo = o; o += H3;
        S.gb = o; o += 1;
        S.count = o;
        S.alloc = (o + 3) & ~3;
        return S;
    }
};
// non-trainable PartitionedNorm state per domain (partitioned_norm.py:71-87 + the zero-debias slots
// of TF 1.12's assign_moving_average): [mov_mean | mov_var | biased_mean | biased_var] each [D][384], steps [D]
struct StarAuxLayout {
    int mov_mean, mov_var, biased_mean, biased_var, steps, count;
    __host__ __device__ static StarAuxLayout make(int n_domain) {
        StarAuxLayout A;
        A.mov_mean = 0;
        A.mov_var = n_domain * XDIM;
        A.biased_mean = 2 * n_domain * XDIM;
        A.biased_var = 3 * n_domain * XDIM;
        A.steps = 4 * n_domain * XDIM;
        A.count = (A.steps + n_domain + 3) & ~3;
        return A;
    }
};
constexpr float PN_EPS = 1e-3f;
constexpr float PN_MOMENTUM = 0.99f;
constexpr int STAR_CHUNK = 16;        // batch rows per partial of the column statistics
constexpr int PN_XDOM_OFF = 5 * XDIM;    // the batch's normalised domain-embedding row (what every sample's x[256:384] is)
constexpr int PN_WS_FLOATS = 5 * XDIM + EMB;   // scale | shift | mean | inv | coef = gamma_eff * inv | xdom

// ---- counter-based dropout stream (restated in oracle/rng.py)
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ inline uint32_t dropout_layer_key(uint32_t seed, uint32_t step, uint32_t layer) {
    uint32_t k0 = fmix32(seed + 0x9E3779B9u * (step + 1u));
    return fmix32(k0 ^ (0x85EBCA6Bu * (layer + 1u)));
}
__device__ __forceinline__ uint32_t mamdr_dropout_u32(uint32_t key, uint32_t elem) {
    return fmix32(key + 0x9E3779B9u * elem);
}

#define MAMDR_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define MAMDR_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// ---- small helpers every step-kernel source uses
template <int N> struct VecT;
template <> struct VecT<4> { typedef f32x4 type; };
template <> struct VecT<2> { typedef f32x2 type; };
template <> struct VecT<1> { typedef float type; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Workspace stores (activations, gradients, gradient slabs): WRITE-THROUGH (agent-scope relaxed atomic store =
// global_store ... sc1).  With plain stores the 3.7 MB a step of k_tower4 writes sit dirty in the eight L2s until the
// kernel ends and are written back between that kernel and k_wgrad_adam: 3.6 us from the tower's last workgroup to the
// next kernel's first one, 1.5 us with no stores at all, 2.2 us with write-through stores (tools/stamp_wall.py;
// nontemporal stores: 2.6 us; plain-, nontemporal- and no-store variants since removed).  The next kernel reads these
// rows from other XCDs anyway.  4-byte pieces only (wider vectors are stored piecewise).
// The OPPOSITE boundary keeps plain stores: k_wgrad_adam leaves ~2 MB of parameters and slots dirty, yet the next tower's
// first workgroup starts 1.3 - 1.4 us after its last one ends.  Written through (4-byte pieces, or 16-byte pieces staged
// through LDS) that gap is 1.1 - 1.3 us, but k_wgrad_adam itself takes about 1.7 us longer -- its last stores are
// acknowledged by memory, not by the L2 -- and the headline drops from 44.8 K to 42.6 K domain-steps/s
// (profiles/ab_param_handoff.txt; both variants removed).
__device__ __forceinline__ void ws_store1(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename V>
__device__ __forceinline__ void ws_store(float* p, const V& v) {
    if constexpr (sizeof(V) == 4) {
        ws_store1(p, v);
    } else {
#pragma unroll
        for (int t = 0; t < (int)(sizeof(V) / 4); ++t) ws_store1(p + t, v[t]);
    }
}

// The plain optimiser step of one element.  TF1 ApplyAdam: m += (g - m)(1-b1); v += (g^2 - v)(1-b2);
// p -= (m * alpha) / (sqrt(v) + eps), alpha = lr sqrt(1-b2^t)/(1-b1^t) from the host.  SGD: p -= g alpha.
// Accumulate only: `m` is the meta-gradient accumulator, p and v are untouched.
// (It contracts, or not, as the including translation unit is compiled.  The sites that fix their roundings -- dm_apply1,
// adam_zero_step, emb_bodies.h's adam_elem -- keep arithmetic of their own.)
__device__ __forceinline__ void opt_step(const int optimizer, const float g, float& p, float& m, float& v, const float alpha,
                                         const float omb1, const float omb2, const float eps) {
    if (optimizer == 0) {             // MAMDR_OPT_ADAM
        m = m + (g - m) * omb1;
        v = v + (g * g - v) * omb2;
        p = p - (m * alpha) / (sqrtf(v) + eps);
    } else if (optimizer == 1) {      // MAMDR_OPT_SGD
        p = p - g * alpha;
    } else {                          // MAMDR_OPT_ACCUMULATE
        m = m + g;
    }
}
// (the same with the hyperparameters taken from the launch's argument block)
template <typename Args>
__device__ __forceinline__ void opt_step(const Args& a, const float g, float& p, float& m, float& v) {
    opt_step(a.optimizer, g, p, m, v, a.alpha, a.omb1, a.omb2, a.eps);
}

// Diagnostic build only (-DMAMDR_STAMPS; tools/stamp_*.py): one counter stamp into a buffer nothing else reads.  `counter`
// is MAMDR_CYCLES (s_memtime, the XCD's cycle counter) or MAMDR_REALTIME (s_memrealtime: one 100 MHz counter for the whole
// device, comparable across XCDs and kernels); the stamp goes to `slot` where `cond` holds.  The production library has
// no stamp code.
#ifdef MAMDR_STAMPS
#define MAMDR_CYCLES "s_memtime"
#define MAMDR_REALTIME "s_memrealtime"
#define MAMDR_STAMP(counter, cond, slot)                                                      \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        unsigned long long t_;                                                                \
        asm volatile(counter " %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        if (cond) (slot) = t_;                                                                \
    } while (0)
#else
#define MAMDR_STAMP(counter, cond, slot) do { } while (0)
#endif

}  // namespace mamdr
