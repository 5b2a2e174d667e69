// Checks the dealing arithmetic of k_wgrad_adam (mamdr_amd/csrc/wgrad_adam_deal.h): the S workgroups' column blocks are a
// bijection that stays inside the half of dz1 their residue's tiles read, every tile of every weight matrix is dealt exactly
// once with 26 tiles per residue, and the line model -- the distinct 128-B lines per batch row of xpre / acts / dz that the
// workgroups of one residue mod 8 (one XCD) read -- gives 12 lines from the tiles, none more from the S workgroups under
// the XCD-aware placement and two more on every residue under blk = b.  Built and run by
// tests/test_wgrad_adam_deal_host.py with the host compiler's address and undefined-behaviour sanitizers.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "wgrad_adam_deal.h"

using namespace mamdr;

static int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (fails++ < 20) {                           \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// the rows of the three operand buffers (mamdr_device.h): xpre [user | item], acts [x | h1 | h2 | h3], dz [dz1 | dz2 | dz3];
// every row starts on a line boundary (256, 832 and 448 floats are multiples of 32)
constexpr int EMB = FZ_DEAL_EMB, H1 = FZ_DEAL_H1, H2 = FZ_DEAL_H2, H3 = FZ_DEAL_H3, XDIM = 3 * EMB;
constexpr int LINE = 32;      // floats per 128-B line
static_assert((2 * EMB) % LINE == 0 && (XDIM + H1 + H2 + H3) % LINE == 0 && (H1 + H2 + H3) % LINE == 0, "rows are whole lines");
enum Buf { XPRE = 0, ACTS = 1, DZ = 2 };
typedef std::set<std::pair<int, int>> Lines;      // (buffer, line of the row)

static void touch(Lines& l, int buf, int col0, int ncols) {
    for (int c = col0; c < col0 + ncols; ++c) l.insert(std::make_pair(buf, c / LINE));
}

static void tile_lines(Lines& l, const FzTile& f) {
    if (f.gemm == 0) {
        touch(l, XPRE, 16 * f.ablk, 16);
        touch(l, DZ, 32 * f.bblk, 32);
    } else if (f.gemm == 1) {
        touch(l, ACTS, XDIM + 16 * f.ablk, 16);
        touch(l, DZ, H1 + 32 * f.bblk, 32);
    } else {
        touch(l, ACTS, XDIM + H1 + 16 * f.ablk, 16);
        touch(l, DZ, H1 + H2 + 32 * f.bblk, 32);
    }
}

int main() {
    // ---- S workgroups: a bijection of [0, 32) inside the residue's half of dz1
    for (int in_order = 0; in_order < 2; ++in_order) {
        std::vector<int> seen(FZ_SBLK, 0);
        for (int b = 0; b < FZ_SBLK; ++b) {
            const int blk = fz_s_block(b, in_order != 0);
            CHECK(blk >= 0 && blk < FZ_SBLK, "b %d -> block %d (in_order %d)", b, blk, in_order);
            if (blk >= 0 && blk < FZ_SBLK) seen[blk] += 1;
            if (in_order) CHECK(blk == b, "in order: b %d -> %d", b, blk);
            else CHECK((blk >> 4) == ((b & 7) >> 2), "b %d -> block %d lies in the other half of dz1", b, blk);
        }
        for (int k = 0; k < FZ_SBLK; ++k) CHECK(seen[k] == 1, "block %d dealt %d times (in_order %d)", k, seen[k], in_order);
    }
    // ---- tiles: every (gemm, ablk, bblk) exactly once, 26 per residue
    const int na[3] = {2 * EMB / 16, H1 / 16, H2 / 16}, nb[3] = {H1 / 32, H2 / 32, H3 / 32};
    std::set<std::vector<int>> tiles;
    int per_res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < FZ_TILES; ++t) {
        const FzTile f = fz_tile(t);
        CHECK(f.gemm >= 0 && f.gemm < 3, "tile %d: gemm %d", t, f.gemm);
        if (f.gemm < 0 || f.gemm > 2) continue;
        CHECK(f.ablk >= 0 && f.ablk < na[f.gemm] && f.bblk >= 0 && f.bblk < nb[f.gemm], "tile %d: gemm %d block (%d, %d)", t, f.gemm,
              f.ablk, f.bblk);
        CHECK(tiles.insert(std::vector<int>{f.gemm, f.ablk, f.bblk}).second, "tile %d: (%d, %d, %d) dealt twice", t, f.gemm, f.ablk,
              f.bblk);
        per_res[t & 7] += 1;
    }
    CHECK((int)tiles.size() == na[0] * nb[0] + na[1] * nb[1] + na[2] * nb[2] && (int)tiles.size() == FZ_TILES, "%d distinct tiles",
          (int)tiles.size());
    for (int x = 0; x < 8; ++x) CHECK(per_res[x] == 26, "residue %d holds %d tiles", x, per_res[x]);
    // ---- line model per residue: tile t is workgroup FZ_SBLK + t (the same residue: FZ_SBLK % 8 == 0), S workgroup b is b
    int extra_new = 0, extra_old = 0;
    for (int x = 0; x < 8; ++x) {
        Lines tl;
        for (int t = x; t < FZ_TILES; t += 8) tile_lines(tl, fz_tile(t));
        CHECK((int)tl.size() == 12, "residue %d: the tiles read %d lines per row", x, (int)tl.size());
        for (int in_order = 0; in_order < 2; ++in_order) {
            Lines all = tl;
            for (int b = x; b < FZ_SBLK; b += 8) touch(all, DZ, FZ_SC * fz_s_block(b, in_order != 0), FZ_SC);
            const int extra = (int)all.size() - (int)tl.size();
            if (in_order) {
                CHECK(extra == 2, "residue %d: blk = b adds %d lines per row", x, extra);
                extra_old += extra;
            } else {
                CHECK(extra == 0, "residue %d: the S workgroups add %d lines per row", x, extra);
                extra_new += extra;
            }
        }
    }
    std::printf("%d S blocks, %d tiles, 12 lines per row and residue; S workgroups' extra lines over 8 residues: %d dealt, %d in order; %d failures\n",
                FZ_SBLK, (int)tiles.size(), extra_new, extra_old, fails);
    return fails ? 1 : 0;
}
