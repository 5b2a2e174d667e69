"""Diagnostic: per-phase cycles of k_wgrad_adam's workgroups from s_memtime stamps (build -DMAMDR_STAMPS, never shipped).
usage: python tools/stamp_fused.py <libstamps.so> [shape] [batch]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np, torch
from mamdr_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from mamdr_amd import engine, synthetic
shape = sys.argv[2] if len(sys.argv) > 2 else "taobao10"
bs = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
g = synthetic.generate(shape, batch_size=bs, seed=123)
eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], bs, dropout=0.5)
eng.bind_table("user_emb", g["tables"]["user_emb"]); eng.bind_table("item_emb", g["tables"]["item_emb"])
d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
c = g["data"]["train"][d]; eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
rs = np.random.RandomState(0)
eng.set_weights(torch.from_numpy((rs.standard_normal(eng.n_params) * 0.05).astype(np.float32)).to(eng.device))
n = eng.n_rows(d, "train")
stamps = torch.zeros(65536 + 8192, dtype=torch.int64, device=eng.device)
eng.lib.mamdr_debug_set_stamps.argtypes = [C.c_void_p, C.c_void_p]
eng.lib.mamdr_debug_set_stamps(eng.ctx, C.c_void_p(stamps.data_ptr()))
perm = torch.from_numpy(engine.shuffle_perm(n, 10000, 1)).to(eng.device)
for _ in range(5):
    eng.train_steps(d, perm=perm, first_step=0, n_steps=3)
torch.cuda.synchronize()
raw = stamps.cpu().numpy()[65536:65536 + 8 * 242].reshape(242, 8).astype(np.float64)


def role_map(residue):
    """own workgroup b -> role (0 - 2: tile of dW0 / dW1 / dW2, 3: S, 4: output unit), from the table the kernel itself reads
    (mamdr_amd/csrc/wgrad_adam_deal.h, printed by a host program built here: one source for the map)"""
    import subprocess, tempfile
    src = ('#include <cstdio>\n#include "wgrad_adam_deal.h"\nint main() { constexpr mamdr::FzDealTable t = mamdr::fz_deal_table_make();\n'
           'for (int b = 0; b < mamdr::FZ_OWN; ++b) std::printf("%d %d\\n", t.code[b][0], t.code[b][1]); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "deal.cpp"), os.path.join(tmp, "deal")
        open(cpp, "w").write(src)
        subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"), cpp, "-o", exe])
        codes = np.array([[int(v) for v in l.split()] for l in subprocess.check_output([exe], text=True).splitlines()])
    return codes[:, 1 if residue else 0] & 7


in_order = os.environ.get("MAMDR_FZ_S_INORDER", "0") not in ("", "0")
residue = in_order or os.environ.get("MAMDR_FZ_DEAL_RESIDUE", "0") not in ("", "0")
role = role_map(residue)
b_all = np.arange(242)
ws = raw[:, :5]
r0 = raw[:, 5].min()
print("k_wgrad_adam stamps, %s (cycles relative to the first workgroup's start): start | contraction begins | ends | barrier passed | done" %
      ("residue dealing" if residue else "dealing by matrix"))
for name, idx in (("S workgroups", b_all[role == 3]), ("tiles", b_all[role < 3]), ("output unit", b_all[role == 4])):
    w = np.diff(ws[idx], axis=1)
    print("  %-13s n=%3d  phase cycles: median %s   max %s   lifetime median %d max %d" % (
        name, len(w), np.round(np.median(w, axis=0)).astype(int).tolist(), np.round(w.max(axis=0)).astype(int).tolist(),
        np.median(ws[idx][:, 4] - ws[idx][:, 0]), (ws[idx][:, 4] - ws[idx][:, 0]).max()))
print("  (phases: prologue | contraction | wait at the barrier | reduce + optimiser step)")
# Lifetimes in the CU's own cycles; ends on the device-wide 100 MHz clock, relative to the launch's first workgroup.
print("by residue mod 8 (one XCD each): workgroups S / tiles / output | lifetime cycles median / max | end on the device-wide clock, 10 ns, median / max")
for x in range(8):
    idx = b_all[(b_all & 7) == x]
    life = raw[idx, 4] - raw[idx, 0]
    end = raw[idx, 6] - r0
    print("  residue %d  %2d / %2d / %d  lifetime %6d / %6d | end %4d / %4d" % (
        x, (role[idx] == 3).sum(), (role[idx] < 3).sum(), (role[idx] == 4).sum(), np.median(life), life.max(), np.median(end), end.max()))
for name, idx in (("S workgroups", b_all[role == 3]), ("tiles", b_all[role < 3]), ("output unit", b_all[role == 4])):
    end = raw[idx, 6] - r0
    print("  %-13s end %4d / %4d   the latest: b=%d" % (name, np.median(end), end.max(), idx[np.argmax(end)]))
if residue:
    # The S workgroups in two classes: workgroup b's column block under blk = b lies in the half of dz1 that the tiles of its
    # residue b & 7 (its XCD) read -- b >> 4 == (b & 7) >> 2 -- or in the other half, where b is its XCD's only reader of those
    # lines.  (The classes are sets of workgroups: without MAMDR_FZ_S_INORDER every block is in the right half.)
    b_ = np.arange(32)
    home = (b_ >> 4) == ((b_ & 7) >> 2)
    print("placement (MAMDR_FZ_S_INORDER=%d): lifetime cycles median / max | end on the device-wide clock, 10 ns, median / max" % in_order)
    for name, idx in (("S, block b on the reading XCD", b_[home]), ("S, block b on another XCD", b_[~home]), ("tiles", np.arange(32, 240))):
        life = raw[idx, 4] - raw[idx, 0]
        end = raw[idx, 6] - r0
        print("  %-30s n=%3d  lifetime %6d / %6d | end %4d / %4d" % (name, len(idx), np.median(life), life.max(), np.median(end), end.max()))
    late = np.argsort(raw[:32, 6])[::-1][:8]
    print("  the 8 S workgroups that end last: %s" % ", ".join("b=%d%s" % (b, "" if home[b] else "*") for b in late), "(*: block b on another XCD)")
