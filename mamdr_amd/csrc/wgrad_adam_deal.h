// The dealing arithmetic of k_wgrad_adam (fused_kernels.hip): which S workgroup takes which 8-column block of dz1, and
// which tile workgroup takes which 16 x 32 tile of which weight matrix.  No HIP dependencies
// (tests/test_wgrad_adam_deal_host.py builds it with the host compiler alone).
//
// Workgroups b and b + 8 k share an XCD (round-robin dispatch; the residue b & 7 is a label of the group, not the XCD's
// id) and the 8 L2s share no data, so the launch is as long as the number of cold 128-B operand lines one XCD pulls
// across the fabric.  Residue x = (xa = x & 3, xb = x >> 2) reads a quarter of the activation columns (xa) and a half of
// the gradient columns (xb) of every matrix: per batch row 2 + 2 + 1 lines of A (x | h1 | h2) and 4 + 2 + 1 lines of dz
// (dz1 | dz2 | dz3), 12 lines in all -- and the S workgroups of the residue take column blocks of dz1 inside the half its
// tiles read anyway.  All of this is a speed assumption only: no value depends on it.
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

}  // namespace mamdr
