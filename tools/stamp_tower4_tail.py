"""Diagnostic: k_tower4's phases behind layer 0, and when each workgroup ends within its launch (headline workload: Taobao-10,
1,024 rows, frozen tables, the domain-table step pending).  Reads the stamps of a -DMAMDR_STAMPS library
(tools/build_variant.sh <name> -DMAMDR_STAMPS); every read is the last two steps of a three-step call, one per parity.
usage: python tools/stamp_tower4_tail.py <libstamps.so> phases     medians over 16 launches x 256 workgroups: the phase table,
                                                                   the domain-table duty inside layer 0, and the cycle at
                                                                   which wave 0 has the first operands of layer 1 / of
                                                                   backward 1 in registers (T4STAMP_X)
       python tools/stamp_tower4_tail.py <libstamps.so> rank       >= 200 launches: end of every workgroup (s_memrealtime)
                                                                   against the launch's median, by tile index and XCD residue"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np, torch
from mamdr_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
mode = sys.argv[2]
from mamdr_amd import engine, synthetic
bs = 1024
g = synthetic.generate("taobao10", batch_size=bs, seed=123)
eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], bs, dropout=0.5)
eng.bind_table("user_emb", g["tables"]["user_emb"]); eng.bind_table("item_emb", g["tables"]["item_emb"])
d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
c = g["data"]["train"][d]; eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
rs = np.random.RandomState(0)
eng.set_weights(torch.from_numpy((rs.standard_normal(eng.n_params) * 0.05).astype(np.float32)).to(eng.device))
n = eng.n_rows(d, "train")
tiles = bs // 4
stamps = torch.zeros(65536 + 8192 + 4096, dtype=torch.int64, device=eng.device)
eng.lib.mamdr_debug_set_stamps.argtypes = [C.c_void_p, C.c_void_p]
eng.lib.mamdr_debug_set_stamps(eng.ctx, C.c_void_p(stamps.data_ptr()))
perm = torch.from_numpy(engine.shuffle_perm(n, 10000, 1)).to(eng.device)
n_domain = g["n_domain"]

if mode == "phases":
    # medians over the stamped launches of several calls (each read: the last two steps of a 3-step call, by parity)
    rows = []
    for it in range(12):
        stamps.zero_()
        eng.train_steps(d, perm=perm, first_step=0, n_steps=3)
        torch.cuda.synchronize()
        if it < 4:
            continue
        st = stamps.cpu().numpy()
        for par in (0, 1):
            w0 = st[par * 16384:par * 16384 + tiles * 16].reshape(tiles, 16).astype(np.float64)
            w4 = st[par * 16384 + 256 * 16:par * 16384 + (256 + tiles) * 16].reshape(tiles, 16).astype(np.float64)
            if w0[:, 0].min() > 0 and w0[:, 13].min() > 0:      # a launch with the domain-table step pending (midseg stamped)
                rows.append((w0, w4))
    print("stamped launches with a pending domain-table step: %d (x %d workgroups)" % (len(rows), tiles))
    if not rows:
        sys.exit("no stamps: %s is not a -DMAMDR_STAMPS build" % sys.argv[1])
    W0 = np.concatenate([r[0] for r in rows]); W4 = np.concatenate([r[1] for r in rows])
    t0 = W0[:, 0]
    names = ["prefetch+gather", "L0 contract", "L0 exchange+epilogue", "L1 contract", "L1 exchange+epilogue", "L2 contract",
             "L2 epi+out/loss/dz3", "bwd2 contract+epilogue", "bwd1 contract+epilogue"]
    dif = np.diff(W0[:, :10], axis=1)
    tot = W0[:, 9] - W0[:, 0]
    print("total cycles median %.0f (min %.0f max %.0f)" % (np.median(tot), tot.min(), tot.max()))
    for i, nme in enumerate(names):
        print("  %-26s %8.0f" % (nme, np.median(dif[:, i])))
    print("  tail behind layer 0 (stamps 2 -> 9) median %.0f" % np.median(W0[:, 9] - W0[:, 2]))
    print("  gather detail (after kernel start, median): midseg entered %.0f | domain columns finished %.0f | domain rows written back %.0f | layer 0 begins %.0f | layer 0 ends %.0f" %
          tuple(np.median(W0[:, k] - t0) for k in (13, 14, 15, 1, 2)))
    wr = np.arange(len(W0)) % tiles < n_domain
    print("  write-back duty (stamp 14 -> 15): tiles < n_domain median %.0f | other tiles median %.0f" %
          (np.median((W0[:, 15] - W0[:, 14])[wr]), np.median((W0[:, 15] - W0[:, 14])[~wr])))
    x = W4[:, 8:10]
    if x.min() > 0:
        print("  first layer-1 operands in registers (wave 0): %.0f after kernel start, %.0f after the epilogue barrier (stamp 3)" %
              (np.median(x[:, 0] - t0), np.median(x[:, 0] - W0[:, 3])))
        print("  first backward-1 operands in registers (wave 0): %.0f after kernel start, %.0f after the epilogue barrier (stamp 8)" %
              (np.median(x[:, 1] - t0), np.median(x[:, 1] - W0[:, 8])))
else:
    # Part C's ranking: when does each workgroup END within its launch (s_memrealtime, 10 ns ticks)?
    ends, starts = [], []
    for it in range(120):
        stamps.zero_()
        eng.train_steps(d, perm=perm, first_step=0, n_steps=3)
        torch.cuda.synchronize()
        if it < 10:
            continue
        st = stamps.cpu().numpy()
        for par in (0, 1):
            w0 = st[par * 16384:par * 16384 + tiles * 16].reshape(tiles, 16).astype(np.float64)
            if w0[:, 10].min() > 0 and w0[:, 13].min() > 0:
                starts.append(w0[:, 10] * 10.0); ends.append(w0[:, 11] * 10.0)
    E, S = np.array(ends), np.array(starts)           # [launch][tile] ns
    print("launches ranked: %d (pending domain-table step, 1,024 rows, %d workgroups)" % (len(E), tiles))
    first = S.min(axis=1, keepdims=True)
    rel = E - np.median(E, axis=1, keepdims=True)     # end relative to the launch's median workgroup
    span = E.max(axis=1) - first[:, 0]
    print("launch span (first start -> last end) median %.0f ns; last end - median end: median %.0f ns" % (np.median(span), np.median(E.max(axis=1) - np.median(E, axis=1))))
    rank = E.argsort(axis=1).argsort(axis=1)           # 0 = first to end, 255 = last
    t = np.arange(tiles)
    print("by tile group: end - median end [ns] (median over launches and tiles; mean) | rank of the end (median) | share of launches in which the group holds the LAST finisher")
    last = E.argmax(axis=1)
    groups = [("tiles < n_domain (%d)" % n_domain, t < n_domain), ("tiles >= n_domain", t >= n_domain)]
    for r in range(8):
        groups.append(("residue %d, tiles >= n_domain" % r, (t % 8 == r) & (t >= n_domain)))
    for r in range(8):
        groups.append(("residue %d, tiles < n_domain" % r, (t % 8 == r) & (t < n_domain)))
    for name, m in groups:
        if not m.any():
            continue
        print("  %-32s n=%3d  end-median %7.0f (mean %7.0f)  start-first %6.0f  lifetime %7.0f  rank %5.1f  last finisher in %5.1f %% of launches" % (
            name, m.sum(), np.median(rel[:, m]), rel[:, m].mean(), np.median((S - first)[:, m]), np.median((E - S)[:, m]), np.median(rank[:, m]), 100.0 * np.isin(last, t[m]).mean()))
    print("  per tile < n_domain: " + " ".join("t%d:%+.0f/r%.0f" % (k, np.median(rel[:, k]), np.median(rank[:, k])) for k in range(n_domain)))
    print("  the ten latest tiles by median end-median: " + " ".join("t%d:%+.0f" % (k, np.median(rel[:, k])) for k in np.argsort(-np.median(rel, axis=0))[:10]))
eng.close()
