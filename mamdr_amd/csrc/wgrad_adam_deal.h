// The dealing arithmetic of k_wgrad_adam (fused_kernels.hip): which own workgroup of the launch takes which 8-column block of
// dz1 (S workgroup), which 16 x 32 tile of which weight matrix (tile workgroup), or which half of the output unit.  No HIP
// dependencies (tests/test_wgrad_adam_deal_host.py and tests/test_wgrad_adam_deal2_host.py build it with the host compiler
// alone).
//
// Workgroups b and b + 8 k share an XCD (round-robin dispatch; the residue b & 7 is a label of the group, not the XCD's
// id) and the 8 L2s share no data, so the launch is as long as the number of cold 128-B operand lines one XCD pulls
// across the fabric.  Two dealings, the same blocks, the same values (no value depends on the dealing: a speed assumption
// only).  Lines are counted per batch row: 8 of x, 8 + 4 + 2 of h1 | h2 | h3, 8 + 4 + 2 of dz1 | dz2 | dz3, 36 distinct.
//
// * The residue dealing (fz_s_block, fz_tile, the output units at 240 / 241; MAMDR_FZ_DEAL_RESIDUE=1): every residue holds
//   the same mix, 4 S workgroups + 16 tiles of dW0 + 8 of dW1 + 2 of dW2.  Residue x = (xa = x & 3, xb = x >> 2) reads a
//   quarter of the activation columns (xa) and a half of the gradient columns (xb) of every matrix: 2 + 2 + 1 lines of A
//   (x | h1 | h2) and 4 + 2 + 1 lines of dz (dz1 | dz2 | dz3), 12 lines in all -- and the S workgroups of the residue take
//   column blocks of dz1 inside the half its tiles read anyway.  With the h3 line of the output unit on residues 0 and 1:
//   13 13 12 12 12 12 12 12, worst 13, 98 over the chip.
// * The dealing by matrix (FZ_DEAL2, the default): three small rectangles per XCD cost more lines than one large one
//   (la + lb lines for 2 la lb tiles), so the XCDs specialise.  Worst residue 10 lines, 69 over the chip:
//     residue 0   dW1[0:128, :] less one tile                                   31 tiles             8 lines
//     residue 1   dW1[128:256, :] less two tiles, and the tile residue 0 lacks  31 tiles             9 lines
//     residue 2   all of dW2; dz1 lines 5 - 7's S blocks; 2 tiles of dW0        12 S + 18 tiles     10 lines
//     residue 3   dW0[0:128, 0:96]    and 6 S blocks of dz1 lines 0 - 2          6 S + 24 tiles      7 lines
//     residue 4   dW0[128:256, 0:96]  and the other 6                            6 S + 24 tiles      7 lines
//     residue 5   dW0[0:128, 96:192],   dz1 line 3's S blocks, the output unit   4 S + 24 tiles + 2  9 lines
//     residue 6   dW0[128:256, 96:192], dz1 line 4's S blocks, 2 tiles of dW1    4 S + 26 tiles      9 lines
//     residue 7   dW0[0:256, 192:256] less the 2 tiles of residue 2             30 tiles            10 lines
//   Every residue holds 30 own workgroups (0 and 1: 31, as the grid has it), S first, then tiles, then output units.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAMDR_DEAL_FN __host__ __device__ constexpr
#else
#define MAMDR_DEAL_FN constexpr
#endif

namespace mamdr {

constexpr int FZ_DEAL_EMB = 128, FZ_DEAL_H1 = 256, FZ_DEAL_H2 = 128, FZ_DEAL_H3 = 64;     // (mamdr_device.h; checked there)
constexpr int FZ_SBLK = 32;                           // S workgroups = 8-column blocks of dz1 (DM_PARTS)
constexpr int FZ_SC = 8;                              // columns per S workgroup
constexpr int FZ_T0 = (2 * FZ_DEAL_EMB / 16) * (FZ_DEAL_H1 / 32);     // 128 tiles of dW0[0:256, :]
constexpr int FZ_T1 = (FZ_DEAL_H1 / 16) * (FZ_DEAL_H2 / 32);          // 64 tiles of dW1
constexpr int FZ_T2 = (FZ_DEAL_H2 / 16) * (FZ_DEAL_H3 / 32);          // 16 tiles of dW2
constexpr int FZ_TILES = FZ_T0 + FZ_T1 + FZ_T2;                       // 208
constexpr int FZ_OUTB = FZ_DEAL_H3 / 32;              // output-unit workgroups = 32-column blocks of h3
constexpr int FZ_OWN = FZ_SBLK + FZ_TILES + FZ_OUTB;  // 242 dealt workgroups (the loss workgroup and the riders sit behind them)

// the S workgroups sit first in the grid: tile t is workgroup FZ_SBLK + t, and its residue t & 7 must be the workgroup's
static_assert(FZ_SBLK % 8 == 0, "tile t and workgroup FZ_SBLK + t must share the residue mod 8");
static_assert(FZ_SBLK * FZ_SC == FZ_DEAL_H1 && FZ_SBLK == 32, "fz_s_block deals 32 blocks of 8 columns");
static_assert(FZ_TILES % 8 == 0, "the same number of tiles on every residue");

// S workgroup b -> its column block of dz1 (columns 8 blk .. 8 blk + 7, in 128-B line blk >> 2 of a dz1 row).  The tiles
// of residue b & 7 read the lines 4 xb .. 4 xb + 3, xb = (b & 7) >> 2: blk >> 4 == xb for every b (a bijection of
// [0, 32): the four S workgroups of a residue take the same quarter of each of the four lines of their half).
// in_order: blk = b (MAMDR_FZ_S_INORDER=1, the placement before: 16 of the 32 blocks sit in the other half, and their
// workgroup is the only reader of 1,024 lines on its XCD)
MAMDR_DEAL_FN int fz_s_block(int b, bool in_order) {
    return in_order ? b : 16 * ((b & 7) >> 2) + 4 * (b >> 3) + (b & 3);
}

struct FzTile {
    int gemm;      // 0: dW0[0:256, :]   1: dW1   2: dW2
    int ablk;      // 16-column block of the A operand (x / h1 / h2) = 16-row block of the weight matrix
    int bblk;      // 32-column block of the gradient (dz1 / dz2 / dz3) = 32-column block of the weight matrix
};
// tile t in [0, 208) -> its matrix and blocks: residue x = t & 7 = (xa, xb) holds 16 + 8 + 2 tiles, li = t >> 3 of them:
// 4 x 4 blocks of dW0 (A blocks 4 xa .. + 3, gradient blocks 4 xb .. + 3), 4 x 2 of dW1, 2 x 1 of dW2
MAMDR_DEAL_FN FzTile fz_tile(int t) {
    const int x = t & 7, xa = x & 3, xb = x >> 2, li = t >> 3;
    if (li < 16) return FzTile{0, 4 * xa + (li & 3), 4 * xb + (li >> 2)};
    if (li < 24) return FzTile{1, 4 * xa + ((li - 16) & 3), 2 * xb + ((li - 16) >> 2)};
    return FzTile{2, 2 * xa + (li - 24), xb};
}

// ---- a workgroup's role as one word (both dealings): role | x << 3 | y << 8
//   role 0 .. 2  tile of dW0 / dW1 / dW2 (FzTile::gemm), x = ablk, y = bblk
//   FZ_ROLE_S    S workgroup, x = its column block of dz1
//   FZ_ROLE_OUT  output unit, x = its 32-column block of h3
constexpr int FZ_ROLE_S = 3, FZ_ROLE_OUT = 4;
MAMDR_DEAL_FN int fz_code(int role, int x, int y) { return role | (x << 3) | (y << 8); }
MAMDR_DEAL_FN int fz_code_role(int code) { return code & 7; }
MAMDR_DEAL_FN int fz_code_x(int code) { return (code >> 3) & 31; }
MAMDR_DEAL_FN int fz_code_y(int code) { return code >> 8; }

// the residue dealing: own workgroup b in [0, FZ_OWN) -> its role ([0, 32) S, [32, 240) tiles, 240 / 241 output unit)
MAMDR_DEAL_FN int fz_residue_code(int b, bool in_order) {
    if (b < FZ_SBLK) return fz_code(FZ_ROLE_S, fz_s_block(b, in_order), 0);
    if (b < FZ_SBLK + FZ_TILES) {
        const FzTile f = fz_tile(b - FZ_SBLK);
        return fz_code(f.gemm, f.ablk, f.bblk);
    }
    return fz_code(FZ_ROLE_OUT, b - FZ_SBLK - FZ_TILES, 0);
}

// ---- the dealing by matrix: a table, built at compile time from the rectangles of the header comment.  Workgroup
// 8 k + x is item k of residue x's list (S blocks first: they are the longest chains and keep the lowest grid indices).
struct FzDeal2 {
    int code[FZ_OWN];      // own workgroup b -> fz_code
    int n[8];              // own workgroups per residue
};
MAMDR_DEAL_FN void fz_deal2_put(FzDeal2& d, int x, int code) {
    d.code[8 * d.n[x] + x] = code;         // (past FZ_OWN: not a constant expression, the build stops)
    d.n[x] += 1;
}
// the tiles [a0, a1) x [b0, b1) of one matrix to residue x, less the tiles [sa0, sa1) of gradient block sb
MAMDR_DEAL_FN void fz_deal2_rect(FzDeal2& d, int x, int gemm, int a0, int a1, int b0, int b1, int sa0 = 0, int sa1 = 0, int sb = -1) {
    for (int bb = b0; bb < b1; ++bb)
        for (int ab = a0; ab < a1; ++ab)
            if (!(bb == sb && ab >= sa0 && ab < sa1)) fz_deal2_put(d, x, fz_code(gemm, ab, bb));
}
MAMDR_DEAL_FN void fz_deal2_s(FzDeal2& d, int x, int blk0, int blk1) {
    for (int blk = blk0; blk < blk1; ++blk) fz_deal2_put(d, x, fz_code(FZ_ROLE_S, blk, 0));
}
MAMDR_DEAL_FN FzDeal2 fz_deal2_make() {
    FzDeal2 d{};
    // residue 0: dW1, h1 lines 0 - 3 x dz2 lines 0 - 3, less tile (7, 3)
    fz_deal2_rect(d, 0, 1, 0, 8, 0, 4, 7, 8, 3);
    // residue 1: dW1, h1 lines 4 - 7 x dz2 lines 0 - 3, less tiles (14, 3) and (15, 3); and tile (7, 3)
    fz_deal2_rect(d, 1, 1, 8, 16, 0, 4, 14, 16, 3);
    fz_deal2_put(d, 1, fz_code(1, 7, 3));
    // residue 2: the S blocks of dz1 lines 5 - 7, all of dW2, dW0 tiles (14, 7) and (15, 7) (x line 7, dz1 line 7)
    fz_deal2_s(d, 2, 20, 32);
    fz_deal2_rect(d, 2, 2, 0, 8, 0, 2);
    fz_deal2_rect(d, 2, 0, 14, 16, 7, 8);
    // residues 3, 4: dW0, x lines 0 - 3 / 4 - 7 x dz1 lines 0 - 2, and six S blocks of those lines each
    fz_deal2_s(d, 3, 0, 6);
    fz_deal2_rect(d, 3, 0, 0, 8, 0, 3);
    fz_deal2_s(d, 4, 6, 12);
    fz_deal2_rect(d, 4, 0, 8, 16, 0, 3);
    // residue 5: dW0, x lines 0 - 3 x dz1 lines 3 - 5, the S blocks of dz1 line 3, both output units
    fz_deal2_s(d, 5, 12, 16);
    fz_deal2_rect(d, 5, 0, 0, 8, 3, 6);
    for (int ob = 0; ob < FZ_OUTB; ++ob) fz_deal2_put(d, 5, fz_code(FZ_ROLE_OUT, ob, 0));
    // residue 6: dW0, x lines 4 - 7 x dz1 lines 3 - 5, the S blocks of dz1 line 4, dW1 tiles (14, 3) and (15, 3)
    fz_deal2_s(d, 6, 16, 20);
    fz_deal2_rect(d, 6, 0, 8, 16, 3, 6);
    fz_deal2_rect(d, 6, 1, 14, 16, 3, 4);
    // residue 7: dW0, x lines 0 - 7 x dz1 lines 6 - 7, less tiles (14, 7) and (15, 7)
    fz_deal2_rect(d, 7, 0, 0, 16, 6, 8, 14, 16, 7);
    return d;
}
constexpr FzDeal2 FZ_DEAL2 = fz_deal2_make();
// every residue is full: 8 k + x < FZ_OWN for exactly the k below (a second round on a CU would cost more than any line)
MAMDR_DEAL_FN bool fz_deal2_full(const FzDeal2& d) {
    for (int x = 0; x < 8; ++x)
        if (d.n[x] != (FZ_OWN - x + 7) / 8) return false;
    return true;
}
static_assert(fz_deal2_full(FZ_DEAL2), "the dealing by matrix must fill every residue's 30 / 31 own workgroups");

// what k_wgrad_adam reads, one 8-byte entry per own workgroup: {its role dealt by matrix, its role under the residue dealing}.
// Both words arrive with one scalar load whose address depends on the workgroup id alone, so the load goes out with the
// kernel's first argument loads and the flag word only selects between two registers.  (Under MAMDR_FZ_S_INORDER=1 an S
// workgroup of the residue dealing takes block b instead of the entry's: fz_residue_code(b, true).)
struct FzDealTable {
    int code[FZ_OWN][2];
};
MAMDR_DEAL_FN FzDealTable fz_deal_table_make() {
    FzDealTable t{};
    for (int b = 0; b < FZ_OWN; ++b) {
        t.code[b][0] = FZ_DEAL2.code[b];
        t.code[b][1] = fz_residue_code(b, false);
    }
    return t;
}

}  // namespace mamdr
