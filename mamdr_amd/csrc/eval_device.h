// Device pieces the evaluation kernel files share (exact_kernels.hip, isotonic_kernels.hip, gauc_kernels.hip,
// bootstrap_kernels.hip; nothing else includes this): the wave reduction and scan, the workgroup scan, the three-launch
// device-wide exclusive scan, and the fixed-order workgroup sum.  Everything sits in an unnamed namespace: each of the four
// translation units keeps its own copy with internal linkage, compiled with that file's flags (-ffp-contract=off where
// the file carries it).  Workgroups are 256 threads, four waves of 64.
//
// THE SUMMATION ORDER (block_sum) is the contract behind "the same bits from run to run and under any permutation of the
// rows" of AP, the GAUC numerator and the Brier / log-loss sums.  For every field of S on its own:
//   lanes   v += shuffle_down(v, o) for o = 32, 16, 8, 4, 2, 1: lane 0 of a wave ends with
//           ((((((l0 + l32) + (l16 + l48)) + ...: the pairs 32 apart first, then 16 apart, ... then neighbours
//   waves   ((w0 + w1) + w2) + w3, every thread reading the four wave results from LDS
// The result is valid in thread 0 (every thread computes the waves' part; only lane 0 of a wave held a wave total).  What a
// thread adds up BEFORE the tree -- which positions, in which order -- is each kernel's own and stated there.
#pragma once
#include "mamdr_kernels.h"

namespace mamdr {
namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

// ------------------------------------------------------------------------------------------------------------ operators
// a combine operator over T: identity, combine(earlier, later), and the wave shuffles of a T
template <class V>
struct ScalarOp {
    typedef V T;
    static __device__ __forceinline__ T identity() { return (T)0; }
    static __device__ __forceinline__ T up(T v, int o) { return __shfl_up(v, o); }
    static __device__ __forceinline__ T down(T v, int o) { return __shfl_down(v, o); }
};
struct AddU32 : ScalarOp<uint32_t> {
    static __device__ __forceinline__ T combine(T a, T b) { return a + b; }
};
struct AddU64 : ScalarOp<u64> {
    static __device__ __forceinline__ T combine(T a, T b) { return a + b; }
};
struct MaxU32 : ScalarOp<uint32_t> {
    static __device__ __forceinline__ T combine(T a, T b) { return b > a ? b : a; }
};

// exact_kernels.hip's element over the sorted composites (what the three words mean: that file's header)
struct ExactRun {
    uint32_t cp, rs, cs;         // positives; last start of a run of equal keys; last start of a run of equal composites
};
struct RunOp {
    typedef ExactRun T;
    static __device__ __forceinline__ T identity() { return T{0u, 0u, 0u}; }
    static __device__ __forceinline__ T combine(T a, T b) { return T{a.cp + b.cp, a.rs > b.rs ? a.rs : b.rs, a.cs > b.cs ? a.cs : b.cs}; }
    static __device__ __forceinline__ T up(T v, int o) { return T{__shfl_up(v.cp, o), __shfl_up(v.rs, o), __shfl_up(v.cs, o)}; }
};

// ----------------------------------------------------------------------------------------------------------------- wave
// shuffle-down tree: the wave's combined value, valid in lane 0 (a caller that needs it in every lane broadcasts it)
template <class Op>
__device__ __forceinline__ typename Op::T wave_reduce(typename Op::T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::combine(v, Op::down(v, o));
    return v;
}

// inclusive shuffle-up scan: lanes 0 .. `lane` combined, in lane order
template <class Op>
__device__ __forceinline__ typename Op::T wave_scan(typename Op::T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const typename Op::T up = Op::up(v, o);
        if (lane >= o) v = Op::combine(up, v);
    }
    return v;
}

// ----------------------------------------------------------------------------------------------------------------- scan
// exclusive scan of one value per thread over the workgroup (lanes by shuffles, the four waves through LDS) -> what lies
// before this thread's value; `total` is the whole workgroup's.  Ends behind a barrier: `lds` may be reused at once
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T v, typename Op::T* lds, typename Op::T& total) {
    typedef typename Op::T T;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // wave_scan's loop, written out: through the call k_scan_apply<RunOp> takes two more registers than it did
    // (profiles/eval_device_refactor.txt, section 7)
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = Op::up(inc, o);
        if (lane >= o) inc = Op::combine(up, inc);
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    T before = Op::identity();
    total = Op::identity();
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const T s = lds[i];
        if (i < w) before = Op::combine(before, s);
        total = Op::combine(total, s);
    }
    __syncthreads();
    T excl = Op::up(inc, 1);
    if (lane == 0) excl = Op::identity();
    return Op::combine(before, excl);
}

// The device-wide exclusive scan, three launches: k_scan_sums (the totals of the tiles of TILE elements), the scan of the
// totals (the same two kernels again while they do not fit one tile), k_scan_apply (in place, with the tile's carry).  The
// kernel boundary is the only hand-off between workgroups.
template <class Op, int TILE>
__global__ __launch_bounds__(THREADS) void k_scan_sums(const typename Op::T* in, typename Op::T* sums, int64_t len) {
    typedef typename Op::T T;
    constexpr int ITEMS = TILE / THREADS;
    __shared__ T lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * TILE + threadIdx.x * ITEMS;
    T v = Op::identity();
#pragma unroll
    for (int j = 0; j < ITEMS; ++j)
        if (first + j < len) v = Op::combine(v, in[first + j]);
    T total;
    block_scan<Op>(v, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// exclusive scan in place; carry (nullable: a single tile) holds what lies before every tile
template <class Op, int TILE>
__global__ __launch_bounds__(THREADS) void k_scan_apply(typename Op::T* data, const typename Op::T* carry, int64_t len) {
    typedef typename Op::T T;
    constexpr int ITEMS = TILE / THREADS;
    __shared__ T lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * TILE + threadIdx.x * ITEMS;
    T item[ITEMS];
    T v = Op::identity();
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        item[j] = first + j < len ? data[first + j] : Op::identity();
        v = Op::combine(v, item[j]);
    }
    T total;
    T running = block_scan<Op>(v, lds, total);
    if (carry) running = Op::combine(carry[blockIdx.x], running);
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        if (first + j < len) data[first + j] = running;
        running = Op::combine(running, item[j]);
    }
}

// elements of the workspace the levels above `len` need: the tile totals of every level
inline int64_t scan_work(int64_t len, int tile) {
    int64_t total = 0;
    while (len > tile) {
        len = (len + tile - 1) / tile;
        total += len;
    }
    return total;
}

template <class Op, int TILE>
void scan_exclusive(typename Op::T* data, int64_t len, typename Op::T* work, hipStream_t s) {
    typedef typename Op::T T;
    if (len <= TILE) {
        MAMDR_LAUNCH((k_scan_apply<Op, TILE>), dim3(1), dim3(THREADS), 0, s, data, (const T*)nullptr, len);
        return;
    }
    const int64_t tiles = (len + TILE - 1) / TILE;
    MAMDR_LAUNCH((k_scan_sums<Op, TILE>), dim3((unsigned)tiles), dim3(THREADS), 0, s, (const T*)data, work, len);
    scan_exclusive<Op, TILE>(work, tiles, work + tiles, s);
    MAMDR_LAUNCH((k_scan_apply<Op, TILE>), dim3((unsigned)tiles), dim3(THREADS), 0, s, data, (const T*)work, len);
}

// ------------------------------------------------------------------------------------------------------------------ sum
// the fixed tree over one workgroup, in the order of this file's header; the result is thread 0's.  S supplies
// add(const S&), += of every field in declaration order, and down(o), a shuffle-down of every field.  No barrier behind
// the read of `lds`: a caller that writes it again puts one in between
template <class S>
__device__ __forceinline__ S block_sum(S v, S* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v.add(v.down(o));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    S s = lds[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s.add(lds[i]);
    return s;
}

}  // namespace
}  // namespace mamdr
