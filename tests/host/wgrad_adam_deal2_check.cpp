// Checks both dealings of k_wgrad_adam (mamdr_amd/csrc/wgrad_adam_deal.h) as maps of the own workgroups [0, 242) to roles:
// each is a bijection onto the 32 S blocks, the 208 tiles and the 2 output-unit workgroups; every residue mod 8 (one XCD)
// holds 30 or 31 own workgroups, its S workgroups below its tiles and output units; and the line model -- the distinct 128-B
// lines per batch row of xpre / acts / dz that the workgroups of one residue read, the output units' h3 lines included --
// gives 12 lines per residue (13 where an output unit sits) under the residue dealing and the counts the header states
// under the dealing by matrix, whose worst residue must stay at or below 10 lines and whose total at or below 74.  Built
// and run by tests/test_wgrad_adam_deal2_host.py with the host compiler's address and undefined-behaviour sanitizers.
#include <cstdio>
#include <set>
#include <string>
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

// the operand lines of one role (fz_tile_body, fz_s_body, fz_out_body of fused_kernels.hip)
static void role_lines(Lines& l, int code) {
    const int role = fz_code_role(code), x = fz_code_x(code), y = fz_code_y(code);
    if (role == 0) {
        touch(l, XPRE, 16 * x, 16);
        touch(l, DZ, 32 * y, 32);
    } else if (role == 1) {
        touch(l, ACTS, XDIM + 16 * x, 16);
        touch(l, DZ, H1 + 32 * y, 32);
    } else if (role == 2) {
        touch(l, ACTS, XDIM + H1 + 16 * x, 16);
        touch(l, DZ, H1 + H2 + 32 * y, 32);
    } else if (role == FZ_ROLE_S) {
        touch(l, DZ, FZ_SC * x, FZ_SC);
    } else {
        touch(l, ACTS, XDIM + H1 + H2 + 32 * x, 32);
    }
}

struct Count {
    int lines[8], worst, total;
};

// one dealing, given as its 242 codes: bijection, residues, order inside a residue, line model
static Count check_dealing(const char* name, const std::vector<int>& code, bool s_first) {
    const int na[3] = {2 * EMB / 16, H1 / 16, H2 / 16}, nb[3] = {H1 / 32, H2 / 32, H3 / 32};
    std::set<std::vector<int>> seen;
    int n_s = 0, n_tile = 0, n_out = 0;
    CHECK((int)code.size() == FZ_OWN && FZ_OWN == 242, "%s: %d codes", name, (int)code.size());
    for (int b = 0; b < (int)code.size(); ++b) {
        const int role = fz_code_role(code[b]), x = fz_code_x(code[b]), y = fz_code_y(code[b]);
        CHECK(code[b] == fz_code(role, x, y), "%s: workgroup %d: code %d does not decode to itself", name, b, code[b]);
        if (role >= 0 && role < 3) {
            CHECK(x >= 0 && x < na[role] && y >= 0 && y < nb[role], "%s: workgroup %d: gemm %d block (%d, %d)", name, b, role, x, y);
            n_tile += 1;
        } else if (role == FZ_ROLE_S) {
            CHECK(x >= 0 && x < FZ_SBLK && y == 0, "%s: workgroup %d: S block %d (%d)", name, b, x, y);
            n_s += 1;
        } else if (role == FZ_ROLE_OUT) {
            CHECK(x >= 0 && x < FZ_OUTB && y == 0, "%s: workgroup %d: output block %d (%d)", name, b, x, y);
            n_out += 1;
        } else {
            CHECK(false, "%s: workgroup %d: role %d", name, b, role);
        }
        CHECK(seen.insert(std::vector<int>{role, x, y}).second, "%s: workgroup %d: role (%d, %d, %d) dealt twice", name, b, role, x, y);
    }
    CHECK(n_s == FZ_SBLK && n_tile == FZ_TILES && n_tile == 208 && n_out == FZ_OUTB && (int)seen.size() == FZ_OWN,
          "%s: %d S blocks, %d tiles, %d output blocks, %d distinct", name, n_s, n_tile, n_out, (int)seen.size());
    Count c = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, 0};
    for (int x = 0; x < 8; ++x) {
        int own = 0, last_s = -1, first_other = FZ_OWN;
        Lines l;
        for (int b = x; b < (int)code.size(); b += 8) {
            own += 1;
            if (fz_code_role(code[b]) == FZ_ROLE_S) last_s = b;
            else if (b < first_other) first_other = b;
            role_lines(l, code[b]);
        }
        CHECK(own == 30 || own == 31, "%s: residue %d holds %d own workgroups", name, x, own);
        if (s_first) CHECK(last_s < first_other, "%s: residue %d: S workgroup %d sits behind workgroup %d", name, x, last_s, first_other);
        c.lines[x] = (int)l.size();
        c.total += c.lines[x];
        if (c.lines[x] > c.worst) c.worst = c.lines[x];
    }
    return c;
}

static std::string show(const Count& c) {
    std::string s;
    for (int x = 0; x < 8; ++x) s += std::to_string(c.lines[x]) + " ";
    return s + "worst " + std::to_string(c.worst) + " total " + std::to_string(c.total);
}

int main() {
    std::vector<int> residue, in_order, matrix;
    for (int b = 0; b < FZ_OWN; ++b) {
        residue.push_back(fz_residue_code(b, false));
        in_order.push_back(fz_residue_code(b, true));
        matrix.push_back(FZ_DEAL2.code[b]);
    }
    // the table the kernel reads holds both
    constexpr FzDealTable table = fz_deal_table_make();
    static_assert(sizeof(table.code) == sizeof(int) * 2 * FZ_OWN, "one 8-byte entry per own workgroup");
    for (int b = 0; b < FZ_OWN; ++b)
        CHECK(table.code[b][0] == matrix[b] && table.code[b][1] == residue[b], "the kernel's table, workgroup %d: %d %d", b, table.code[b][0],
              table.code[b][1]);
    // the residue dealing in codes is what fz_s_block / fz_tile say (tests/host/wgrad_adam_deal_check.cpp pins those)
    for (int b = 0; b < FZ_OWN; ++b) {
        const int c = residue[b];
        if (b < FZ_SBLK) {
            CHECK(fz_code_role(c) == FZ_ROLE_S && fz_code_x(c) == fz_s_block(b, false), "residue dealing: S workgroup %d", b);
            CHECK(fz_code_x(in_order[b]) == b, "residue dealing in order: S workgroup %d", b);
        } else if (b < FZ_SBLK + FZ_TILES) {
            const FzTile f = fz_tile(b - FZ_SBLK);
            CHECK(fz_code_role(c) == f.gemm && fz_code_x(c) == f.ablk && fz_code_y(c) == f.bblk && in_order[b] == c, "residue dealing: tile workgroup %d", b);
        } else {
            CHECK(fz_code_role(c) == FZ_ROLE_OUT && fz_code_x(c) == b - FZ_SBLK - FZ_TILES && in_order[b] == c, "residue dealing: output workgroup %d", b);
        }
    }
    const Count cr = check_dealing("residue dealing", residue, true);
    const Count ci = check_dealing("residue dealing in order", in_order, true);
    const Count cm = check_dealing("dealing by matrix", matrix, true);
    for (int x = 0; x < 8; ++x) {
        CHECK(cr.lines[x] == (x < 2 ? 13 : 12), "residue dealing: residue %d reads %d lines per row", x, cr.lines[x]);
        CHECK(ci.lines[x] == cr.lines[x] + 2, "residue dealing in order: residue %d reads %d lines per row", x, ci.lines[x]);
        CHECK(FZ_DEAL2.n[x] == (x < 2 ? 31 : 30), "dealing by matrix: residue %d holds %d", x, FZ_DEAL2.n[x]);
    }
    const int stated[8] = {8, 9, 10, 7, 7, 9, 9, 10};      // the header's comment
    for (int x = 0; x < 8; ++x) CHECK(cm.lines[x] == stated[x], "dealing by matrix: residue %d reads %d lines per row, stated %d", x, cm.lines[x], stated[x]);
    CHECK(cm.worst <= 10, "dealing by matrix: worst residue %d lines", cm.worst);
    CHECK(cm.total <= 74, "dealing by matrix: %d lines over the chip", cm.total);
    std::printf("lines per row and residue: residue dealing %s; in order %s; by matrix %s; %d failures\n", show(cr).c_str(), show(ci).c_str(),
                show(cm).c_str(), fails);
    return fails ? 1 : 0;
}
