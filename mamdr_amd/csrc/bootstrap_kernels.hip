// Poisson-bootstrap replicates of the exact AUC's integers T, P, N (mamdr_auc_bootstrap, include/mamdr_hip.h, which carries
// the definition in full; the host definition is mamdr_amd/bootstrap.py).  No reference counterpart: the reference reports
// point estimates only.
//
// Replicate b weighs row i by w(b, i) = poisson1(u32(b, unit(i))), a pure function of (seed, b, unit): nothing per row and
// replicate is ever stored -- n x n_rep weights in HBM would be 200 MB at the measured size (200,000 rows x 1,000
// replicates) and would be written once and read twice, where recomputing one costs two 64-bit multiplications and the
// table's 13 comparisons in registers.
//
// The chain:
//   sort          exact_kernels.hip's radix sort (launch_exact_sort, `rows`) of the word key << 32 | positive << 31 | row on
//                 its upper 33 bits: ascending in (key, positive, row), unique.
//   k_boot_parts  grid = tiles of BOOT_TILE = 1,024 sorted positions x groups of BOOT_GROUP = 16 replicates.  A WAVE, not the
//                 workgroup, is the unit of work: every wave holds the whole tile in registers -- lane l the 16 consecutive
//                 positions 16 l .. 16 l + 15: the unit id gathered through the row, and three 16-bit masks (valid, positive,
//                 starts a run of equal keys) -- and takes 4 of the group's replicates in turn.  No LDS, no barrier: the scans
//                 over the tile are a serial walk over a lane's 16 positions and wave-64 shuffles across the lanes
//                 (wave_reduce / wave_scan over AddU32 and MaxU32, eval_device.h).  Per
//                 (replicate, tile) it writes the tile's negative weight, positive weight, and `head`: 0 when no run starts
//                 in the tile, else 1 + the negative weight in front of the LAST run start of the tile.
//   k_boot_carry  one wave per replicate walks the tiles 64 at a time: the exclusive sum of the negative weights gives tile
//                 t its carry Cn(tile start); with it `head` becomes Cn(last run start of t), whose exclusive running
//                 maximum is Cn(rs) of the run that reaches into tile t from an earlier one (Cn never descends, so the
//                 maximum is the latest).  Both overwrite the partials in place; the totals are d_N[b] and d_P[b].
//   k_boot_T      k_boot_parts' grid and registers again: the weights recomputed, Cn(i) by the scan from the tile's carry,
//                 Cn(rs(i)) by the running maximum of Cn at run starts from the carried one, the tile's
//                 sum_{positive i} w (Cn(rs(i)) + Cn(i)) reduced in the wave and added to d_T[b] by ONE 64-bit integer atomic.
//   The partials take 3 words per (tile, replicate); BOOT_PART_WORDS bounds them, and more replicates than fit run in
//   chunks through the same buffers (a chunk is a multiple of BOOT_GROUP and at least one group).
//
// Determinism: integers only.  Integer atomics commute, every other value has one writer.  No floating-point instruction.
#include "eval_device.h"
#include "host_common.h"

namespace mamdr {
namespace {

constexpr int ITEMS = BOOT_TILE / 64;                  // positions per lane
constexpr int REPS = BOOT_GROUP / WAVES;               // replicates per wave
static_assert(ITEMS == 16, "the masks of a lane are 16 bits");
static_assert(BOOT_GROUP % WAVES == 0, "every wave takes the same number of replicates");

struct BootPass {
    const u64* sorted;           // [n] key << 32 | positive << 31 | row, ascending
    const int32_t* unit;         // nullable [n]
    int64_t n, n_tiles;
    u64 seed;
    int first, slots;            // the chunk: replicates first .. first + slots - 1
    uint32_t* part_n;            // [slots][n_tiles] negative weight of the tile, then (k_boot_carry) Cn at the tile's start
    uint32_t* part_p;            // [slots][n_tiles] positive weight of the tile
    uint32_t* part_h;            // [slots][n_tiles] head (see above), then Cn(rs) of the run that reaches into the tile
    u64* T;                      // [n_rep + 1]
    long long* P;
    long long* N;
};

__device__ __forceinline__ u64 boot_mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the replicate's half of the hash: mix64(seed + 0x9E3779B97F4A7C15 * b)
__device__ __forceinline__ u64 boot_replicate(u64 seed, int b) { return boot_mix64(seed + 0x9E3779B97F4A7C15ull * (u64)b); }

// poisson1(high 32 bits of mix64(hb ^ unit)): the number of thresholds at or below the draw (constants: unrolled)
__device__ __forceinline__ uint32_t boot_weight(u64 hb, uint32_t unit) {
    constexpr uint32_t thr[MAMDR_BOOT_WMAX] = MAMDR_BOOT_THR;
    const uint32_t u = (uint32_t)(boot_mix64(hb ^ (u64)unit) >> 32);
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < MAMDR_BOOT_WMAX; ++k) w += u >= thr[k] ? 1u : 0u;
    return w;
}

struct BootTile {
    uint32_t unit[ITEMS];
    uint32_t valid, positive, head;      // bit j: position 16 lane + j of the tile
};

__device__ __forceinline__ void boot_load(const BootPass& p, int64_t tile, int lane, BootTile& t) {
    const int64_t first = tile * BOOT_TILE + lane * ITEMS;
    u64 prev = (first > 0 && first < p.n) ? p.sorted[first - 1] : 0ull;
    t.valid = t.positive = t.head = 0u;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int64_t i = first + j;
        const bool ok = i < p.n;
        const u64 c = ok ? p.sorted[i] : 0ull;
        uint32_t row = (uint32_t)c & 0x7fffffffu;
        if ((int64_t)row >= p.n) row = 0u;                   // (cannot happen: the rows are a permutation; never beyond the column)
        t.unit[j] = !ok ? 0u : (p.unit ? (uint32_t)p.unit[row] : row);
        t.valid |= (ok ? 1u : 0u) << j;
        t.positive |= ((ok && ((c >> 31) & 1ull)) ? 1u : 0u) << j;
        t.head |= ((ok && (i == 0 || (c >> 32) != (prev >> 32))) ? 1u : 0u) << j;
        prev = c;
    }
}

// the weights of one replicate over the lane's positions; replicate 0 is the unweighted statistic
__device__ __forceinline__ void boot_weights(const BootTile& t, u64 seed, int b, uint32_t (&w)[ITEMS]) {
    const u64 hb = boot_replicate(seed, b);
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const uint32_t x = b == 0 ? 1u : boot_weight(hb, t.unit[j]);
        w[j] = ((t.valid >> j) & 1u) ? x : 0u;
    }
}

// the wave's sum / maximum, in every lane (wave_reduce, wave_scan: eval_device.h)
template <class Op>
__device__ __forceinline__ uint32_t wave_all(uint32_t v) {
    return __shfl(wave_reduce<Op>(v), 0);
}
// what lies in front of this lane's value
__device__ __forceinline__ uint32_t wave_excl_add(uint32_t v, int lane) { return wave_scan<AddU32>(v, lane) - v; }
__device__ __forceinline__ uint32_t wave_excl_max(uint32_t v, int lane) {
    const uint32_t before = __shfl_up(wave_scan<MaxU32>(v, lane), 1);
    return lane == 0 ? 0u : before;
}

__global__ __launch_bounds__(THREADS) void k_boot_parts(const BootPass p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    BootTile t;
    boot_load(p, tile, lane, t);
    // the tile's last run start, as 1 + its position in the tile (0: none), and the lane's positions in front of it
    const uint32_t mine = t.head ? (uint32_t)(lane * ITEMS + (31 - __clz((int)t.head)) + 1) : 0u;
    const uint32_t last = wave_all<MaxU32>(mine);
    uint32_t front = 0u;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) front |= ((uint32_t)(lane * ITEMS + j + 1) < last ? 1u : 0u) << j;
    for (int r = 0; r < REPS; ++r) {
        const int slot = blockIdx.y * BOOT_GROUP + r * WAVES + w;
        if (slot >= p.slots) break;                          // (the same for every lane of the wave)
        uint32_t wt[ITEMS];
        boot_weights(t, p.seed, p.first + slot, wt);
        uint32_t sn = 0u, sp = 0u, sf = 0u;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const bool positive = (t.positive >> j) & 1u;
            sp += positive ? wt[j] : 0u;
            sn += positive ? 0u : wt[j];
            sf += (!positive && ((front >> j) & 1u)) ? wt[j] : 0u;
        }
        sn = wave_all<AddU32>(sn);
        sp = wave_all<AddU32>(sp);
        sf = wave_all<AddU32>(sf);
        if (lane == 0) {
            const int64_t at = (int64_t)slot * p.n_tiles + tile;
            p.part_n[at] = sn;
            p.part_p[at] = sp;
            p.part_h[at] = last ? 1u + sf : 0u;
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_boot_carry(const BootPass p) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (slot >= p.slots) return;
    uint32_t* part_n = p.part_n + (int64_t)slot * p.n_tiles;
    uint32_t* part_h = p.part_h + (int64_t)slot * p.n_tiles;
    const uint32_t* part_p = p.part_p + (int64_t)slot * p.n_tiles;
    uint32_t carry = 0u, head = 0u, positives = 0u;          // (every weight of a replicate together is below 2^27 * 13 < 2^31)
    for (int64_t t0 = 0; t0 < p.n_tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool ok = t < p.n_tiles;
        const uint32_t wn = ok ? part_n[t] : 0u, wp = ok ? part_p[t] : 0u, h = ok ? part_h[t] : 0u;
        const uint32_t cn = carry + wave_excl_add(wn, lane);
        const uint32_t at_head = h ? cn + (h - 1u) : 0u;     // Cn at the tile's last run start
        const uint32_t before = wave_excl_max(at_head, lane);
        if (ok) {
            part_n[t] = cn;
            part_h[t] = before > head ? before : head;
        }
        carry += wave_all<AddU32>(wn);
        positives += wave_all<AddU32>(wp);
        const uint32_t m = wave_all<MaxU32>(at_head);
        head = m > head ? m : head;
    }
    if (lane == 0) {
        p.P[p.first + slot] = (long long)positives;
        p.N[p.first + slot] = (long long)carry;
    }
}

__global__ __launch_bounds__(THREADS) void k_boot_T(const BootPass p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    BootTile t;
    boot_load(p, tile, lane, t);
    for (int r = 0; r < REPS; ++r) {
        const int slot = blockIdx.y * BOOT_GROUP + r * WAVES + w;
        if (slot >= p.slots) break;
        uint32_t wt[ITEMS];
        boot_weights(t, p.seed, p.first + slot, wt);
        const int64_t at = (int64_t)slot * p.n_tiles + tile;
        uint32_t sn = 0u;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) sn += ((t.positive >> j) & 1u) ? 0u : wt[j];
        const uint32_t base = p.part_n[at] + wave_excl_add(sn, lane);        // Cn at the lane's first position
        uint32_t cn = base, at_head = 0u;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            if ((t.head >> j) & 1u) at_head = cn;            // (Cn never descends: the lane's last run start is its maximum)
            cn += ((t.positive >> j) & 1u) ? 0u : wt[j];
        }
        const uint32_t before = wave_excl_max(at_head, lane), carried = p.part_h[at];
        uint32_t cn_rs = before > carried ? before : carried;
        cn = base;
        u64 sum = 0ull;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            if ((t.head >> j) & 1u) cn_rs = cn;
            const bool positive = (t.positive >> j) & 1u;
            if (positive) sum += (u64)wt[j] * ((u64)cn_rs + (u64)cn);
            cn += positive ? 0u : wt[j];
        }
        sum = wave_reduce<AddU64>(sum);
        if (lane == 0 && sum) atomicAdd(p.T + p.first + slot, sum);
    }
}

int64_t boot_tiles(int64_t n) { return (n + BOOT_TILE - 1) / BOOT_TILE; }

// the call's workspace behind the sort's: the three partials of one chunk of replicates
struct BootLayout {
    int chunk;
    size_t part_n, part_p, part_h, bytes;
};
BootLayout boot_layout(int64_t n, int n_rep, int64_t part_words) {
    BootLayout l;
    l.chunk = boot_chunk(n, n_rep, part_words);
    const size_t part = (size_t)l.chunk * boot_tiles(n) * sizeof(uint32_t);
    WsCursor ws;
    ws.take(exact_sort_workspace_bytes(n));          // the sort's part leads
    l.part_n = ws.take(part);
    l.part_p = ws.take(part);
    l.part_h = ws.take(part);
    l.bytes = ws.at;
    return l;
}

}  // namespace

int boot_chunk(int64_t n, int n_rep, int64_t part_words) {
    const int64_t all = ((int64_t)n_rep + 1 + BOOT_GROUP - 1) / BOOT_GROUP * BOOT_GROUP;
    int64_t fit = part_words / (3 * boot_tiles(n)) / BOOT_GROUP * BOOT_GROUP;
    if (fit < BOOT_GROUP) fit = BOOT_GROUP;
    return (int)(fit < all ? fit : all);
}

size_t boot_workspace_bytes(int64_t n, int n_rep, int64_t part_words) { return boot_layout(n, n_rep, part_words).bytes; }

void launch_boot(const BootArgs& a, hipStream_t s) {
    ExactSortArgs sort;
    sort.pred = a.pred;
    sort.label = a.label;
    sort.n = a.n;
    sort.rows = 1;
    sort.sorted_out = nullptr;
    sort.ws = a.ws;
    BootPass p;
    p.sorted = launch_exact_sort(sort, s);
    p.unit = a.unit;
    p.n = a.n;
    p.n_tiles = boot_tiles(a.n);
    p.seed = a.seed;
    const BootLayout l = boot_layout(a.n, a.n_rep, a.part_words);
    const int chunk = l.chunk;
    p.part_n = reinterpret_cast<uint32_t*>(a.ws + l.part_n);
    p.part_p = reinterpret_cast<uint32_t*>(a.ws + l.part_p);
    p.part_h = reinterpret_cast<uint32_t*>(a.ws + l.part_h);
    p.T = a.T;
    p.P = a.P;
    p.N = a.N;
    for (int first = 0; first <= a.n_rep; first += chunk) {
        p.first = first;
        p.slots = a.n_rep + 1 - first < chunk ? a.n_rep + 1 - first : chunk;
        const dim3 grid((unsigned)p.n_tiles, (unsigned)((p.slots + BOOT_GROUP - 1) / BOOT_GROUP));
        MAMDR_LAUNCH(k_boot_parts, grid, dim3(THREADS), 0, s, p);
        MAMDR_LAUNCH(k_boot_carry, dim3((unsigned)((p.slots + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, p);
        MAMDR_LAUNCH(k_boot_T, grid, dim3(THREADS), 0, s, p);
    }
}

}  // namespace mamdr
