// Exact AUC, average precision and equal-mass calibration bins of one split's predictions (mamdr_exact_metrics,
// include/mamdr_hip.h, which carries the definition in full; the host definition is mamdr_amd/exact.py).  No reference
// counterpart: the reference's pipeline ends at one 500-threshold AUC per domain.
//
// Per row the composite is (u64) key << 1 | positive, key = GAUC's order-preserving 32-bit key (NaN lowest, -0 == +0).
// The chain, one launch per phase; the kernel boundary is the ONLY hand-off between workgroups (no look-back, no flags,
// nothing waits on another workgroup):
//   sort     least-significant-digit radix sort of the 33-bit composites, 5 passes of 8-bit digits.  Per pass:
//            k_exact_hist     per tile of 2,048 composites the count of every digit (LDS integer atomics) -> hist[digit][tile]
//            scan<AddU32>     exclusive sum over hist, digit-major: where (digit, tile) starts in the output
//            k_exact_scatter  stable ranks inside the tile: wave w owns 512 consecutive composites, 64 per round; the lanes
//                             of equal digit find each other by one __ballot per digit bit, a lane's rank among them is
//                             popcount(peers & lanes below), the wave's running count per digit lives in LDS; thread d
//                             then turns the four waves' counts of digit d into their start offsets.
//            Pass 0 forms the composites from pred / label on the fly; the last pass writes d_sorted_out when it is given.
//            The same five passes sort mamdr_auc_bootstrap's wider word, key << 32 | positive << 31 | row, on its upper
//            33 bits (launch_exact_sort with `rows`: every digit sits 31 bits higher, pass 0 forms that word).  The sort is
//            stable and starts from file order, so the rows ascend inside equal (key, positive) pairs.
//   scan     the device-wide scans are eval_device.h's three-launch scan_exclusive<Op, EXACT_SCAN_TILE> over a combine
//            operator: AddU32 for the histograms, RunOp for the sorted array.
//   RunOp    element i of the sorted array is (positive_i, i if i starts a run of equal keys else 0, i if i starts a run of
//            equal composites else 0), combined as (sum, max, max): its scan yields cp(i), rs(i) and cs(i), the first
//            position of i's composite.  For a positive i the positives of its run below it are i - cs(i), so
//            cp(rs(i)) = cp(i) - (i - cs(i)).
//            k_exact_runs     per tile of 1,024 sorted positions the combined element; P by one integer atomic per tile
//            scan<RunOp>      exclusive, over the tiles
//            k_exact_metrics  the scan inside the tile from its carry, then per position the terms of T, n_runs, n_nan,
//                             AP and the bins.  Reduced in the workgroup; ONE 64-bit integer atomic per workgroup and
//                             quantity; the bins through LDS slots (bins ascend with the position, a tile of n >= n_bins
//                             rows touches at most 1,026 -- a row of a smaller split whose bin lies beyond the slots
//                             adds to the global bin directly), then one integer atomic per workgroup and touched bin.
//            k_exact_finish   one workgroup adds the tiles' AP partials and writes N = n - P.
//
// Determinism: every integer is exact and integer atomics commute.  The AP term of a position is one division of two
// integers converted to fp64; the sum has ONE order per n -- thread t of tile b adds positions 1024 b + 4 t + j for j = 0 .. 3
// in turn, then block_sum's tree (eval_device.h), then thread t of k_exact_finish adds tiles t + 256 i in turn and the same
// tree -- so it is the same bits from run to run and, since the sorted array is unique, under any permutation of the rows.
// No floating-point atomics.  Compiled with -ffp-contract=off.
#include "eval_device.h"
#include "host_common.h"

namespace mamdr {
namespace {

constexpr int RADIX = 1 << EXACT_RADIX_BITS;
constexpr int PASSES = (33 + EXACT_RADIX_BITS - 1) / EXACT_RADIX_BITS;
constexpr int SORT_ITEMS = EXACT_SORT_TILE / THREADS;          // composites per thread, in registers
constexpr int SORT_ROUNDS = EXACT_SORT_TILE / WAVES / 64;      // rounds of 64 per wave
constexpr int METRIC_ITEMS = EXACT_METRIC_TILE / THREADS;
constexpr int SLOTS = EXACT_METRIC_TILE + 2;                   // LDS bin slots of k_exact_metrics
static_assert(RADIX == THREADS, "thread d owns digit d");
static_assert(SORT_ITEMS == SORT_ROUNDS, "one composite per thread and round");

// ---------------------------------------------------------------------------------------------------------------- sort
struct SortPass {
    const float* pred;           // pass 0 (src == nullptr) forms the composites from these
    const float* label;
    const u64* src;              // the previous pass's output
    u64* dst;
    uint32_t* hist;              // [RADIX][n_tiles]; counts, then (scanned in place) start offsets
    int64_t n, n_tiles;
    int shift;
    int rows;                    // pass 0 forms key << 32 | positive << 31 | row (bootstrap_kernels.hip), not key << 1 | positive
};

// (key: score_key, mamdr_kernels.h)
__device__ __forceinline__ u64 exact_load(const SortPass& p, int64_t i) {
    if (p.src) return p.src[i];
    const u64 key = score_key(p.pred[i]), positive = p.label[i] != 0.f ? 1ull : 0ull;
    return p.rows ? ((key << 32) | (positive << 31) | (u64)i) : ((key << 1) | positive);
}

__global__ __launch_bounds__(THREADS) void k_exact_hist(const SortPass p) {
    __shared__ uint32_t cnt[RADIX];
    const int tid = threadIdx.x;
    cnt[tid] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * EXACT_SORT_TILE;
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const int64_t i = base + r * THREADS + tid;
        if (i < p.n) atomicAdd(&cnt[(uint32_t)(exact_load(p, i) >> p.shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    p.hist[(int64_t)tid * p.n_tiles + blockIdx.x] = cnt[tid];
}

__global__ __launch_bounds__(THREADS) void k_exact_scatter(const SortPass p) {
    __shared__ uint32_t cnt[WAVES][RADIX];           // per wave and digit: composites so far, then the start offset
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) cnt[i][tid] = 0u;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * EXACT_SORT_TILE + w * (EXACT_SORT_TILE / WAVES);
    const u64 below = (1ull << lane) - 1ull;
    u64 item[SORT_ROUNDS];
    uint32_t rank[SORT_ROUNDS];                      // (constant indices only: registers)
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int64_t i = i0 + r * 64 + lane;
        const bool valid = i < p.n;
        item[r] = valid ? exact_load(p, i) : 0ull;
        const uint32_t d = (uint32_t)(item[r] >> p.shift) & (RADIX - 1);
        u64 peers = __ballot(valid);                 // the valid lanes of equal digit
#pragma unroll
        for (int b = 0; b < EXACT_RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t lower = (uint32_t)__popcll(peers & below);
        const uint32_t prior = cnt[w][d];
        rank[r] = prior + lower;
        if (valid && lower == 0u) cnt[w][d] = prior + (uint32_t)__popcll(peers);       // the lowest peer writes for all
        __syncthreads();                             // (the next round reads the counts this one wrote)
    }
    {   // thread d: digit d's start in the output, then wave by wave
        uint32_t running = p.hist[(int64_t)tid * p.n_tiles + blockIdx.x];
#pragma unroll
        for (int i = 0; i < WAVES; ++i) {
            const uint32_t c = cnt[i][tid];
            cnt[i][tid] = running;
            running += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int64_t i = i0 + r * 64 + lane;
        if (i >= p.n) continue;
        const uint32_t d = (uint32_t)(item[r] >> p.shift) & (RADIX - 1);
        const int64_t at = (int64_t)cnt[w][d] + rank[r];
        if (at < p.n) p.dst[at] = item[r];            // (a permutation of [0, n) by construction; never beyond the buffer)
    }
}

// ------------------------------------------------------------------------------------------------------------- metrics
struct MetricPass {
    const u64* sorted;           // [n]
    ExactRun* runs;              // [n_tiles] the tiles' combined elements, then (scanned in place) their carries
    double* ap_part;             // [n_tiles]
    int64_t n, n_tiles;
    int n_bins;
    u64* counts;                 // T, P, N, n_runs, n_nan
    double* ap;
    u64* bins;                   // [3][n_bins]
};

__device__ __forceinline__ ExactRun exact_elem(int64_t i, u64 c, u64 prev) {
    ExactRun x;
    x.cp = (uint32_t)(c & 1ull);
    x.rs = (i > 0 && (c >> 1) != (prev >> 1)) ? (uint32_t)i : 0u;          // (position 0 starts a run: max with 0)
    x.cs = (i > 0 && c != prev) ? (uint32_t)i : 0u;
    return x;
}

// Q32 of the prediction behind a key: floor(clamp(p, 0, 1) * 2^32 + 0.5) in fp64; a NaN adds 0
__device__ __forceinline__ u64 exact_q32(uint32_t key) {
    if (key == 0u) return 0ull;
    const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    const double p = (double)__uint_as_float(b);
    const double c = p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
    return (u64)floor(c * 4294967296.0 + 0.5);
}

__global__ __launch_bounds__(THREADS) void k_exact_runs(const MetricPass m) {
    __shared__ ExactRun lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * EXACT_METRIC_TILE + threadIdx.x * METRIC_ITEMS;
    u64 prev = (first > 0 && first < m.n) ? m.sorted[first - 1] : 0ull;
    ExactRun v = RunOp::identity();
#pragma unroll
    for (int j = 0; j < METRIC_ITEMS; ++j) {
        const int64_t i = first + j;
        if (i >= m.n) continue;
        const u64 c = m.sorted[i];
        v = RunOp::combine(v, exact_elem(i, c, prev));
        prev = c;
    }
    ExactRun total;
    block_scan<RunOp>(v, lds, total);
    if (threadIdx.x == 0) {
        m.runs[blockIdx.x] = total;
        atomicAdd(m.counts + 1, (u64)total.cp);          // P: k_exact_metrics reads it behind the kernel boundary
    }
}

struct BinAcc {
    int slot, bin;               // slot < 0: nothing pending
    uint32_t rows, positives;
    u64 sum;
};
struct BinSlots {
    uint32_t rows[SLOTS], positives[SLOTS];
    u64 sum[SLOTS];
};
__device__ __forceinline__ void bin_flush(const BinAcc& b, BinSlots& lds, const MetricPass& m) {
    if (b.slot < 0 || b.rows == 0u) return;
    if (b.slot < SLOTS) {
        atomicAdd(&lds.rows[b.slot], b.rows);
        atomicAdd(&lds.positives[b.slot], b.positives);
        atomicAdd(&lds.sum[b.slot], b.sum);
    } else {                     // (n < n_bins only: the bins of one tile spread beyond the slots)
        atomicAdd(m.bins + b.bin, (u64)b.rows);
        atomicAdd(m.bins + m.n_bins + b.bin, (u64)b.positives);
        atomicAdd(m.bins + 2 * (int64_t)m.n_bins + b.bin, b.sum);
    }
}

struct ExactSum {                // (block_sum, eval_device.h)
    double ap;
    u64 T;
    uint32_t runs, nan;
    __device__ __forceinline__ void add(const ExactSum& o) {
        ap += o.ap;
        T += o.T;
        runs += o.runs;
        nan += o.nan;
    }
    __device__ __forceinline__ ExactSum down(int o) const {
        return ExactSum{__shfl_down(ap, o), __shfl_down(T, o), __shfl_down(runs, o), __shfl_down(nan, o)};
    }
};

__global__ __launch_bounds__(THREADS) void k_exact_metrics(const MetricPass m) {
    __shared__ ExactRun lds_run[WAVES];
    __shared__ ExactSum lds_sum[WAVES];
    __shared__ BinSlots slots;
    const int tid = threadIdx.x;
    const int64_t tile_first = (int64_t)blockIdx.x * EXACT_METRIC_TILE;
    const int64_t first = tile_first + tid * METRIC_ITEMS;
    for (int s = tid; s < SLOTS; s += THREADS) {
        slots.rows[s] = 0u;
        slots.positives[s] = 0u;
        slots.sum[s] = 0ull;
    }
    u64 item[METRIC_ITEMS];
    const u64 before = (first > 0 && first < m.n) ? m.sorted[first - 1] : 0ull;
    ExactRun v = RunOp::identity();
    {
        u64 prev = before;
#pragma unroll
        for (int j = 0; j < METRIC_ITEMS; ++j) {
            const int64_t i = first + j;
            item[j] = i < m.n ? m.sorted[i] : 0ull;
            if (i < m.n) v = RunOp::combine(v, exact_elem(i, item[j], prev));
            prev = item[j];
        }
    }
    const ExactRun carry = m.runs[blockIdx.x];
    ExactRun total;
    ExactRun run = RunOp::combine(carry, block_scan<RunOp>(v, lds_run, total));      // (its barriers cover the slots' zeroes)
    const int64_t n = m.n;
    const int64_t P = (int64_t)m.counts[1];
    const int64_t bin_base = tile_first * m.n_bins / n;
    ExactSum acc = {0.0, 0ull, 0u, 0u};
    BinAcc pend = {-1, 0, 0u, 0u, 0ull};
    {
        u64 prev = before;
#pragma unroll
        for (int j = 0; j < METRIC_ITEMS; ++j) {
            const int64_t i = first + j;
            if (i >= n) continue;
            const u64 c = item[j];
            const int64_t cp = run.cp;                   // positives below i
            run = RunOp::combine(run, exact_elem(i, c, prev));
            const int64_t rs = run.rs, cs = run.cs;
            const uint32_t key = (uint32_t)(c >> 1);
            const bool positive = (c & 1ull) != 0ull;
            acc.runs += (i == 0 || (c >> 1) != (prev >> 1)) ? 1u : 0u;
            acc.nan += key == 0u ? 1u : 0u;
            if (positive) {
                const int64_t cp_rs = cp - (i - cs);     // the positives below the run
                acc.T += (u64)((rs - cp_rs) + (i - cp));
                acc.ap += (double)(P - cp_rs) / (double)(n - rs);
            }
            const int bin = (int)(rs * m.n_bins / n);
            // the run that reaches into the tile from before it has slot 0; the bins of the tile's own positions follow
            const int64_t wide = rs < tile_first ? 0 : 1 + (int64_t)bin - bin_base;
            const int slot = wide < SLOTS ? (int)wide : SLOTS;
            if (slot != pend.slot || bin != pend.bin) {
                bin_flush(pend, slots, m);
                pend = BinAcc{slot, bin, 0u, 0u, 0ull};
            }
            pend.rows += 1u;
            pend.positives += positive ? 1u : 0u;
            pend.sum += exact_q32(key);
            prev = c;
        }
    }
    {   // what every thread still holds: one add per wave where the wave's positions share a bin (the common case)
        const int slot0 = __shfl(pend.slot, 0), bin0 = __shfl(pend.bin, 0);      // (lane 0 holds rows whenever a lane of its wave does)
        if (pend.slot < 0) {
            pend.slot = slot0;
            pend.bin = bin0;
        }
        if (__all(pend.slot == slot0 && pend.bin == bin0)) {
            pend.rows = wave_reduce<AddU32>(pend.rows);
            pend.positives = wave_reduce<AddU32>(pend.positives);
            pend.sum = wave_reduce<AddU64>(pend.sum);
            if ((tid & 63) == 0) bin_flush(pend, slots, m);
        } else {
            bin_flush(pend, slots, m);
        }
    }
    const ExactSum sum = block_sum(acc, lds_sum);          // (its barrier: every slot add has landed)
    if (tid == 0) {
        m.ap_part[blockIdx.x] = sum.ap;
        atomicAdd(m.counts + 0, sum.T);
        atomicAdd(m.counts + 3, (u64)sum.runs);
        atomicAdd(m.counts + 4, (u64)sum.nan);
    }
    const int bin_first = (int)((int64_t)carry.rs * m.n_bins / n);
    for (int s = tid; s < SLOTS; s += THREADS) {
        if (slots.rows[s] == 0u) continue;
        const int64_t bin = s == 0 ? bin_first : bin_base + s - 1;
        if (bin >= m.n_bins) continue;                   // (cannot happen: rs < n; never beyond the buffer)
        atomicAdd(m.bins + bin, (u64)slots.rows[s]);
        atomicAdd(m.bins + m.n_bins + bin, (u64)slots.positives[s]);
        atomicAdd(m.bins + 2 * (int64_t)m.n_bins + bin, slots.sum[s]);
    }
}

__global__ __launch_bounds__(THREADS) void k_exact_finish(const MetricPass m) {
    __shared__ ExactSum lds[WAVES];
    ExactSum v = {0.0, 0ull, 0u, 0u};
    for (int64_t b = threadIdx.x; b < m.n_tiles; b += THREADS) v.ap += m.ap_part[b];
    const ExactSum s = block_sum(v, lds);
    if (threadIdx.x == 0) {
        m.ap[0] = s.ap;
        m.counts[2] = (u64)m.n - m.counts[1];
    }
}

// the call's workspace: two composite buffers, the histograms (the sort's part, which leads), the tiles' runs and AP
// partials, the scans' upper levels
struct ExactLayout {
    int64_t sort_tiles, metric_tiles;
    size_t buf_a, buf_b, hist, hist_work, sort_bytes, runs, runs_work, ap_part, bytes;
};
ExactLayout exact_layout(int64_t n) {
    ExactLayout l;
    l.sort_tiles = (n + EXACT_SORT_TILE - 1) / EXACT_SORT_TILE;
    l.metric_tiles = (n + EXACT_METRIC_TILE - 1) / EXACT_METRIC_TILE;
    WsCursor ws;
    l.buf_a = ws.take((size_t)n * sizeof(u64));
    l.buf_b = ws.take((size_t)n * sizeof(u64));
    l.hist = ws.take((size_t)RADIX * l.sort_tiles * sizeof(uint32_t));
    l.hist_work = ws.take((size_t)scan_work((int64_t)RADIX * l.sort_tiles, EXACT_SCAN_TILE) * sizeof(uint32_t));
    l.sort_bytes = ws.at;
    l.runs = ws.take((size_t)l.metric_tiles * sizeof(ExactRun));
    l.runs_work = ws.take((size_t)scan_work(l.metric_tiles, EXACT_SCAN_TILE) * sizeof(ExactRun));
    l.ap_part = ws.take((size_t)l.metric_tiles * sizeof(double));
    l.bytes = ws.at;
    return l;
}

}  // namespace

size_t exact_workspace_bytes(int64_t n) { return exact_layout(n).bytes; }
size_t exact_sort_workspace_bytes(int64_t n) { return exact_layout(n).sort_bytes; }

const unsigned long long* launch_exact_sort(const ExactSortArgs& a, hipStream_t s) {
    const ExactLayout l = exact_layout(a.n);
    u64* buf_a = reinterpret_cast<u64*>(a.ws + l.buf_a);
    u64* buf_b = reinterpret_cast<u64*>(a.ws + l.buf_b);
    SortPass p;
    p.pred = a.pred;
    p.label = a.label;
    p.hist = reinterpret_cast<uint32_t*>(a.ws + l.hist);
    p.n = a.n;
    p.n_tiles = l.sort_tiles;
    p.rows = a.rows;
    const u64* sorted = nullptr;
    for (int pass = 0; pass < PASSES; ++pass) {      // pred / label -> a -> b -> a -> b -> a (or the caller's array)
        p.src = pass == 0 ? nullptr : ((pass & 1) ? buf_a : buf_b);
        p.dst = (pass & 1) ? buf_b : buf_a;
        if (pass == PASSES - 1 && a.sorted_out) p.dst = a.sorted_out;
        p.shift = (a.rows ? 31 : 0) + pass * EXACT_RADIX_BITS;
        MAMDR_LAUNCH(k_exact_hist, dim3((unsigned)l.sort_tiles), dim3(THREADS), 0, s, p);
        scan_exclusive<AddU32, EXACT_SCAN_TILE>(p.hist, (int64_t)RADIX * l.sort_tiles, reinterpret_cast<uint32_t*>(a.ws + l.hist_work), s);
        MAMDR_LAUNCH(k_exact_scatter, dim3((unsigned)l.sort_tiles), dim3(THREADS), 0, s, p);
        sorted = p.dst;
    }
    return sorted;
}

void launch_exact(const ExactArgs& a, hipStream_t s) {
    const ExactLayout l = exact_layout(a.n);
    ExactSortArgs sort;
    sort.pred = a.pred;
    sort.label = a.label;
    sort.n = a.n;
    sort.rows = 0;
    sort.sorted_out = a.sorted_out;
    sort.ws = a.ws;
    const u64* sorted = launch_exact_sort(sort, s);
    MetricPass m;
    m.sorted = sorted;
    m.runs = reinterpret_cast<ExactRun*>(a.ws + l.runs);
    m.ap_part = reinterpret_cast<double*>(a.ws + l.ap_part);
    m.n = a.n;
    m.n_tiles = l.metric_tiles;
    m.n_bins = a.n_bins;
    m.counts = a.counts;
    m.ap = a.ap;
    m.bins = a.bins;
    MAMDR_LAUNCH(k_exact_runs, dim3((unsigned)l.metric_tiles), dim3(THREADS), 0, s, m);
    scan_exclusive<RunOp, EXACT_SCAN_TILE>(m.runs, l.metric_tiles, reinterpret_cast<ExactRun*>(a.ws + l.runs_work), s);
    MAMDR_LAUNCH(k_exact_metrics, dim3((unsigned)l.metric_tiles), dim3(THREADS), 0, s, m);
    MAMDR_LAUNCH(k_exact_finish, dim3(1), dim3(THREADS), 0, s, m);
}

}  // namespace mamdr
