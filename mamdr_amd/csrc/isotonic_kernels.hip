// Isotonic regression (pool adjacent violators) of one split's (prediction, label) pairs, its application to other
// predictions, and the Brier / log-loss sums of a split (mamdr_isotonic_fit(_bounded), mamdr_isotonic_apply,
// mamdr_score_sums: include/mamdr_hip.h, which carries the definitions in full; the host definition is
// mamdr_amd/isotonic.py).  No reference counterpart: the reference's pipeline ends at one 500-threshold AUC per domain.
//
// Definition, in short.  key = GAUC's order-preserving 32-bit key (score_key: NaN lowest and equal to NaN, -0 == +0),
// positive = label != 0.  Sorted by key, a run is a maximal set of rows of one key; run j has r_j rows and s_j positives.
// Points Q_0 = (0, 0), Q_{j+1} = Q_j + (r_j, s_j).  The blocks of the fit are the groups of runs between consecutive STRICT
// vertices of the lower convex hull of Q_0 .. Q_R: with A, B, C consecutive candidates, B is dropped exactly when
// (B.x - A.x) * (C.y - B.y) - (B.y - A.y) * (C.x - B.x) <= 0 in int64 (coordinates are below 2^31: the products are below
// 2^62).  That is PAV pooling the last two blocks while mean_left >= mean_right.
//
// The chain, one launch per phase; the kernel boundary is the ONLY hand-off between workgroups, every count that a later
// kernel needs stays on the device, nothing is read back:
//   sort      launch_exact_sort (exact_kernels.hip): the composites key << 1 | positive, ascending
//   points    k_iso_run_sums   per tile of 1,024 sorted positions (run heads << 32 | positives)
//             scan             exclusive, over the tiles (eval_device.h's scan_exclusive<AddU64, ISO_SCAN_TILE>: 64-bit sums)
//             k_iso_points     the scan inside the tile from its carry; the head of run j at sorted position i writes
//                              point j = (i, positives below i); the last position writes point R = (n, P), n_runs, P and
//                              the number of points; n_nan is the length of the run of key 0
//   hull      a strict vertex of the global hull is a strict vertex of the hull of any contiguous subset that contains it,
//             and the hull is the hull of its strict vertices: dropping, inside a tile, what the tile's own chain drops
//             never loses a vertex, whatever the tiling.  Per level:
//             k_iso_tile_chain one THREAD per tile of tile_points consecutive points: the monotone chain over them, the
//                              stack in the tile's own slots of the other buffer
//             scan             exclusive, over the tiles' survivor counts
//             k_iso_compact    the survivors, packed, back into the first buffer; their number
//             The host fixes the number of levels from n and tile_points alone, as if every level shrank by the most it
//             can (a tile keeps its first and last point: tile_points / 2), until one tile would hold the rest.  The
//             GRIDS are sized for a diagram that never shrinks -- a strictly convex one keeps every point at every
//             level -- and the tiles past the live count leave at once.
//             k_iso_final      one workgroup: the chain over whatever is left, 256 points at a time through LDS, walked
//                              by thread 0 -> the hull's vertices and n_blocks.  O(points left) on one lane: that is
//                              the whole cost when nothing shrank.
//   blocks    k_iso_blocks     block b from vertices b and b + 1: first_key, rows, positives
// Integers only; no floating point and no atomics anywhere in the fit: the outputs are unique, the same bits under any
// tile_points and any order of the rows.
//
//   apply     k_iso_apply      per row the key, a binary search over first_key (staged in LDS up to 4,096 blocks), one
//                              fp64 division rounded once to fp32, one store
//   sums      k_score_parts / k_score_finish   fp64, ONE order per n: thread t of tile b adds rows 1024 b + 4 t + j for
//                              j = 0 .. 3 in turn, then block_sum's tree (eval_device.h); thread t of the finish adds
//                              tiles t + 256 i in turn and the same tree.  No floating-point atomics.
//                              Compiled with -ffp-contract=off.
#include "eval_device.h"
#include "host_common.h"

namespace mamdr {
namespace {

constexpr int POINT_ITEMS = ISO_POINT_TILE / THREADS;
constexpr int APPLY_ITEMS = ISO_APPLY_TILE / THREADS;
constexpr int SCORE_ITEMS = ISO_SCORE_TILE / THREADS;

// -------------------------------------------------------------------------------------------------------------- points
struct PointPass {
    const u64* sorted;           // [n] composites, ascending
    u64* tile_sum;               // [n_tiles] heads << 32 | positives of every tile, then (scanned in place) their carries
    u64* pts;                    // [n + 1] point j = x << 32 | y
    int64_t n;
    long long* counts;           // n_blocks, n_runs, n_nan, P
    long long* m0;               // the number of points, R + 1
};

// (heads << 32 | positives) of sorted position i: both sums stay below 2^31, the halves never meet
__device__ __forceinline__ u64 run_elem(int64_t i, u64 c, u64 prev) {
    return ((i == 0 || (c >> 1) != (prev >> 1)) ? (1ull << 32) : 0ull) | (c & 1ull);
}

__global__ __launch_bounds__(THREADS) void k_iso_run_sums(const PointPass p) {
    __shared__ u64 lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * ISO_POINT_TILE + threadIdx.x * POINT_ITEMS;
    u64 prev = (first > 0 && first < p.n) ? p.sorted[first - 1] : 0ull;
    u64 v = 0ull;
#pragma unroll
    for (int j = 0; j < POINT_ITEMS; ++j) {
        const int64_t i = first + j;
        if (i >= p.n) continue;
        const u64 c = p.sorted[i];
        v += run_elem(i, c, prev);
        prev = c;
    }
    u64 total;
    block_scan<AddU64>(v, lds, total);
    if (threadIdx.x == 0) p.tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(THREADS) void k_iso_points(const PointPass p) {
    __shared__ u64 lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * ISO_POINT_TILE + threadIdx.x * POINT_ITEMS;
    u64 item[POINT_ITEMS];
    u64 prev = (first > 0 && first < p.n) ? p.sorted[first - 1] : 0ull;
    u64 v = 0ull;
#pragma unroll
    for (int j = 0; j < POINT_ITEMS; ++j) {
        const int64_t i = first + j;
        item[j] = 0ull;
        if (i >= p.n) continue;
        const u64 c = p.sorted[i];
        item[j] = run_elem(i, c, prev);
        v += item[j];
        prev = c;
    }
    u64 total;
    u64 running = p.tile_sum[blockIdx.x] + block_scan<AddU64>(v, lds, total);       // heads and positives below position `first`
    const bool nan_first = (p.sorted[0] >> 1) == 0ull;                      // (n > 0) NaN predictions are the lowest run
#pragma unroll
    for (int j = 0; j < POINT_ITEMS; ++j) {
        const int64_t i = first + j;
        if (i >= p.n) continue;
        if (item[j] >> 32) {                                                // i starts run `running >> 32`
            const int64_t run = (int64_t)(running >> 32);
            if (run <= p.n) p.pts[run] = ((u64)i << 32) | (running & 0xffffffffull);       // (run < n by construction)
            if (run == 1 && nan_first) p.counts[2] = i;
        }
        running += item[j];
        if (i == p.n - 1) {
            const int64_t R = (int64_t)(running >> 32), P = (int64_t)(running & 0xffffffffull);
            if (R <= p.n) p.pts[R] = ((u64)p.n << 32) | (u64)P;
            p.counts[1] = R;
            p.counts[3] = P;
            if (R == 1 && nan_first) p.counts[2] = p.n;
            *p.m0 = R + 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- hull
// B leaves the chain A, B, C: it lies on or above the segment A C
__device__ __forceinline__ bool drops(u64 a, u64 b, u64 c) {
    const int64_t ax = (int64_t)(a >> 32), ay = (int64_t)(a & 0xffffffffull);
    const int64_t bx = (int64_t)(b >> 32), by = (int64_t)(b & 0xffffffffull);
    const int64_t cx = (int64_t)(c >> 32), cy = (int64_t)(c & 0xffffffffull);
    return (bx - ax) * (cy - by) - (by - ay) * (cx - bx) <= 0;
}

// one step of the monotone chain: the stack is out[0 .. top), its two topmost entries are kept in a and b
__device__ __forceinline__ void chain_push(u64* out, int64_t& top, u64& a, u64& b, u64 c) {
    while (top >= 2 && drops(a, b, c)) {
        --top;
        b = a;
        if (top >= 2) a = out[top - 2];
    }
    out[top++] = c;
    a = b;
    b = c;
}

struct HullPass {
    u64* src;                    // [cap] the level's points
    u64* dst;                    // [cap] tile g's survivors from dst[g * tile] on
    u64* cnt;                    // [tiles + 1] survivors per tile (entry `tiles` is 0), then (scanned in place) their offsets
    const long long* m_in;       // the level's number of points
    long long* m_out;            // the next level's
    int64_t cap, tiles;          // n + 1; ceil(cap / tile)
    int tile;
};

__device__ __forceinline__ int64_t live_points(const long long* m, int64_t cap) {
    const int64_t v = *m;
    return v < 0 ? 0 : (v > cap ? cap : v);          // (never beyond the buffers, whatever the word holds)
}

__global__ __launch_bounds__(THREADS) void k_iso_tile_chain(const HullPass h) {
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g > h.tiles) return;
    const int64_t m = live_points(h.m_in, h.cap);
    const int64_t first = g * h.tile;
    if (g == h.tiles || first >= m) {
        h.cnt[g] = 0ull;
        return;
    }
    const int64_t count = m - first < h.tile ? m - first : h.tile;
    u64* out = h.dst + first;
    int64_t top = 0;
    u64 a = 0ull, b = 0ull;
    for (int64_t k = 0; k < count; ++k) chain_push(out, top, a, b, h.src[first + k]);
    h.cnt[g] = (u64)top;
}

__global__ __launch_bounds__(THREADS) void k_iso_compact(const HullPass h) {
    const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (p == 0) *h.m_out = (long long)h.cnt[h.tiles];
    if (p >= live_points(h.m_in, h.cap)) return;
    const int64_t g = p / h.tile, k = p - g * h.tile;
    const int64_t off = (int64_t)h.cnt[g], count = (int64_t)h.cnt[g + 1] - off;
    if (k < count && off + k < h.cap) h.src[off + k] = h.dst[p];
}

__global__ __launch_bounds__(THREADS) void k_iso_final(const HullPass h, long long* counts) {
    __shared__ u64 buf[THREADS];
    const int64_t m = live_points(h.m_in, h.cap);
    int64_t top = 0;             // (thread 0's)
    u64 a = 0ull, b = 0ull;
    for (int64_t base = 0; base < m; base += THREADS) {
        if (base + threadIdx.x < m) buf[threadIdx.x] = h.src[base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int count = m - base < THREADS ? (int)(m - base) : THREADS;
            for (int k = 0; k < count; ++k) chain_push(h.dst, top, a, b, buf[k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[0] = top > 0 ? top - 1 : 0;
}

struct BlockPass {
    const u64* hull;             // [n_blocks + 1] vertices
    const u64* sorted;
    const long long* counts;
    int64_t n;
    uint32_t* first_key;
    long long* rows;
    long long* positives;
};

__global__ __launch_bounds__(THREADS) void k_iso_blocks(const BlockPass q) {
    const int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    int64_t n_blocks = q.counts[0];
    if (n_blocks > q.n) n_blocks = q.n;
    if (b >= n_blocks) return;
    const u64 v = q.hull[b], w = q.hull[b + 1];
    const int64_t x = (int64_t)(v >> 32);
    q.first_key[b] = x < q.n ? (uint32_t)(q.sorted[x] >> 1) : 0u;
    q.rows[b] = (int64_t)(w >> 32) - x;
    q.positives[b] = (int64_t)(w & 0xffffffffull) - (int64_t)(v & 0xffffffffull);
}

// the call's workspace behind the sort's: the tiles' run sums, two point buffers, the tiles' survivor counts, the scans'
// upper levels, the levels' point counts
struct IsoLayout {
    int64_t point_tiles, cap, hull_tiles;
    size_t tile_sum, tile_work, pts_a, pts_b, cnt, cnt_work, m, bytes;
};
IsoLayout iso_layout(int64_t n, int tile) {
    IsoLayout l;
    l.point_tiles = (n + ISO_POINT_TILE - 1) / ISO_POINT_TILE;
    l.cap = n + 1;
    l.hull_tiles = (l.cap + tile - 1) / tile;
    WsCursor ws;
    ws.take(exact_sort_workspace_bytes(n));          // the sort's part leads
    l.tile_sum = ws.take((size_t)l.point_tiles * sizeof(u64));
    l.tile_work = ws.take((size_t)scan_work(l.point_tiles, ISO_SCAN_TILE) * sizeof(u64));
    l.pts_a = ws.take((size_t)l.cap * sizeof(u64));
    l.pts_b = ws.take((size_t)l.cap * sizeof(u64));
    l.cnt = ws.take((size_t)(l.hull_tiles + 1) * sizeof(u64));
    l.cnt_work = ws.take((size_t)scan_work(l.hull_tiles + 1, ISO_SCAN_TILE) * sizeof(u64));
    l.m = ws.take((size_t)(ISO_MAX_LEVELS + 1) * sizeof(long long));
    l.bytes = ws.at;
    return l;
}

// --------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(THREADS) void k_iso_apply(const IsoApplyArgs a) {
    __shared__ uint32_t keys[ISO_APPLY_LDS];
    const bool staged = a.n_blocks <= ISO_APPLY_LDS;
    if (staged) {
        for (int s = threadIdx.x; s < (int)a.n_blocks; s += THREADS) keys[s] = a.first_key[s];
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < APPLY_ITEMS; ++r) {
        const int64_t i = (int64_t)blockIdx.x * ISO_APPLY_TILE + r * THREADS + threadIdx.x;
        if (i >= a.n) continue;
        const uint32_t k = score_key(a.pred[i]);
        int64_t lo = 0, hi = a.n_blocks;             // -> the number of blocks with first_key <= k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            const uint32_t at = staged ? keys[mid] : a.first_key[mid];
            if (at <= k) lo = mid + 1;
            else hi = mid;
        }
        const int64_t b = lo > 0 ? lo - 1 : 0;
        a.out[i] = (float)((double)a.positives[b] / (double)a.rows[b]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- sums
struct ScoreSum {                // (block_sum, eval_device.h)
    double brier, logloss;
    __device__ __forceinline__ void add(const ScoreSum& o) {
        brier += o.brier;
        logloss += o.logloss;
    }
    __device__ __forceinline__ ScoreSum down(int o) const { return ScoreSum{__shfl_down(brier, o), __shfl_down(logloss, o)}; }
};

__global__ __launch_bounds__(THREADS) void k_score_parts(const ScoreArgs a) {
    __shared__ ScoreSum lds[WAVES];
    const int64_t first = (int64_t)blockIdx.x * ISO_SCORE_TILE + threadIdx.x * SCORE_ITEMS;
    ScoreSum v = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SCORE_ITEMS; ++j) {
        const int64_t i = first + j;
        if (i >= a.n) continue;
        const double p = (double)a.pred[i];
        const bool positive = a.label[i] != 0.f;
        const double d = p - (positive ? 1.0 : 0.0);
        v.brier += d * d;
        const double q = p < 1e-7 ? 1e-7 : (p > 1.0 - 1e-7 ? 1.0 - 1e-7 : p);       // (a NaN stays a NaN)
        v.logloss += -log(positive ? q : 1.0 - q);
    }
    const ScoreSum s = block_sum(v, lds);
    if (threadIdx.x == 0) {
        a.part[2 * (int64_t)blockIdx.x] = s.brier;
        a.part[2 * (int64_t)blockIdx.x + 1] = s.logloss;
    }
}

__global__ __launch_bounds__(THREADS) void k_score_finish(const ScoreArgs a, int64_t n_tiles) {
    __shared__ ScoreSum lds[WAVES];
    ScoreSum v = {0.0, 0.0};
    for (int64_t b = threadIdx.x; b < n_tiles; b += THREADS) {
        v.brier += a.part[2 * b];
        v.logloss += a.part[2 * b + 1];
    }
    const ScoreSum s = block_sum(v, lds);
    if (threadIdx.x == 0) {
        a.out[0] = s.brier;
        a.out[1] = s.logloss;
    }
}

}  // namespace

int iso_levels(int64_t n, int tile) {
    int levels = 0;
    int64_t most = n + 1;        // the points left if every level so far shrank by tile / 2
    while (most > tile && levels < ISO_MAX_LEVELS) {
        most = 2 * ((most + tile - 1) / tile);
        ++levels;
    }
    return levels;
}

size_t iso_fit_workspace_bytes(int64_t n, int tile) { return iso_layout(n, tile).bytes; }

void launch_iso_fit(const IsoFitArgs& f, hipStream_t s) {
    const IsoLayout l = iso_layout(f.n, f.tile);
    ExactSortArgs sort;
    sort.pred = f.pred;
    sort.label = f.label;
    sort.n = f.n;
    sort.rows = 0;
    sort.sorted_out = nullptr;
    sort.ws = f.ws;
    const u64* sorted = launch_exact_sort(sort, s);
    long long* m = reinterpret_cast<long long*>(f.ws + l.m);
    PointPass p;
    p.sorted = sorted;
    p.tile_sum = reinterpret_cast<u64*>(f.ws + l.tile_sum);
    p.pts = reinterpret_cast<u64*>(f.ws + l.pts_a);
    p.n = f.n;
    p.counts = f.counts;
    p.m0 = m;
    MAMDR_LAUNCH(k_iso_run_sums, dim3((unsigned)l.point_tiles), dim3(THREADS), 0, s, p);
    scan_exclusive<AddU64, ISO_SCAN_TILE>(p.tile_sum, l.point_tiles, reinterpret_cast<u64*>(f.ws + l.tile_work), s);
    MAMDR_LAUNCH(k_iso_points, dim3((unsigned)l.point_tiles), dim3(THREADS), 0, s, p);
    HullPass h;
    h.src = p.pts;
    h.dst = reinterpret_cast<u64*>(f.ws + l.pts_b);
    h.cnt = reinterpret_cast<u64*>(f.ws + l.cnt);
    h.cap = l.cap;
    h.tiles = l.hull_tiles;
    h.tile = f.tile;
    const int levels = iso_levels(f.n, f.tile);
    for (int level = 0; level < levels; ++level) {
        h.m_in = m + level;
        h.m_out = m + level + 1;
        MAMDR_LAUNCH(k_iso_tile_chain, dim3((unsigned)((l.hull_tiles + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, h);
        scan_exclusive<AddU64, ISO_SCAN_TILE>(h.cnt, l.hull_tiles + 1, reinterpret_cast<u64*>(f.ws + l.cnt_work), s);
        MAMDR_LAUNCH(k_iso_compact, dim3((unsigned)((l.cap + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, h);
    }
    h.m_in = m + levels;
    h.m_out = nullptr;
    MAMDR_LAUNCH(k_iso_final, dim3(1), dim3(THREADS), 0, s, h, f.counts);
    BlockPass q;
    q.hull = h.dst;
    q.sorted = sorted;
    q.counts = f.counts;
    q.n = f.n;
    q.first_key = f.first_key;
    q.rows = f.rows;
    q.positives = f.positives;
    MAMDR_LAUNCH(k_iso_blocks, dim3((unsigned)((f.n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, q);
}

void launch_iso_apply(const IsoApplyArgs& a, hipStream_t s) {
    MAMDR_LAUNCH(k_iso_apply, dim3((unsigned)((a.n + ISO_APPLY_TILE - 1) / ISO_APPLY_TILE)), dim3(THREADS), 0, s, a);
}

size_t score_workspace_bytes(int64_t n) { return (size_t)((n + ISO_SCORE_TILE - 1) / ISO_SCORE_TILE) * 2 * sizeof(double); }

void launch_score_sums(const ScoreArgs& a, hipStream_t s) {
    const int64_t tiles = (a.n + ISO_SCORE_TILE - 1) / ISO_SCORE_TILE;
    MAMDR_LAUNCH(k_score_parts, dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
    MAMDR_LAUNCH(k_score_finish, dim3(1), dim3(THREADS), 0, s, a, tiles);
}

}  // namespace mamdr
