"""Device time of mamdr_rank_slates (per-query candidate slates) and the share of its phases, beside the only route without
it: mamdr_recommend_domain with the dense score matrix over the UNION of the slates.  Taobao-10-shaped synthetic data
(23,778 users, 6,932 items, 10 domains), frozen tables, the mlp tower by default, every query in domain 0.

    python tools/slate_bench.py [--tower mlp|wdl|deepfm|star] [--reps 5] [--out profiles/slate_bench.txt]

Two shapes: 4,096 slates x 100 entries (the sampled-negatives protocol; 100 > 64, so k_slate_order's long form: one 256-thread
workgroup per slate, one LDS stage) and 256 slates x 4,096 entries (a re-ranking stage's long slates: 16 workgroups per slate,
four LDS stages each).  Neither shape runs the wave form (slates of up to 64 entries).  Slates are drawn without
replacement from the whole item table, so the union is (nearly) the whole table.

Method: each (shape, leg) runs in a child process of its own under `timeout -k 10`.  Leg `slates`: two warm-up calls, then
`reps` calls between two HIP events on the engine's stream (the call's read-back of the offsets included, uploads and the
outputs' read-back not); then, in a run of their own, `reps` calls with the library's profile slots on: the entries' item
term (k_rec_item_proj: MAMDR_KERNEL_GATHER), the pair tiles (k_rec_pair: MAMDR_KERNEL_EVAL) and k_slate_order
(MAMDR_KERNEL_AUX); the query term is not timed.  Leg `union`: recommend_domain(k = 1, d_scores_all) over the union of the
slates, the same two HIP events.  No threshold: the figures are what this file writes down.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"4096x100": (4096, 100), "256x4096": (256, 4096)}


def leg(args):
    import torch
    from mamdr_amd import _lib as L
    from recommend_bench import build, timed
    eng, n_user, n_item, _ = build(args.tower, 1024)
    n_query, length = SHAPES[args.shape]
    rs = np.random.RandomState(3)
    uids = rs.choice(n_user, n_query, replace=False).astype(np.int32)
    ids = np.argsort(rs.random_sample((n_query, n_item)), axis=1)[:, :length].astype(np.int32)      # distinct per slate
    off = np.arange(n_query + 1, dtype=np.int64) * length
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    res = {"leg": args.leg, "shape": args.shape, "tower": args.tower, "queries": n_query, "length": length,
           "entries": int(off[-1]), "device": torch.cuda.get_device_name(eng.device), "reps": args.reps}
    d_uid = torch.from_numpy(uids).to(eng.device)
    if args.leg == "slates":
        d_off, d_ids = torch.from_numpy(off).to(eng.device), torch.from_numpy(ids.ravel()).to(eng.device)
        scores = torch.empty(int(off[-1]), dtype=torch.float32, device=eng.device)
        pos = torch.empty(int(off[-1]), dtype=torch.int32, device=eng.device)
        order = torch.empty(int(off[-1]), dtype=torch.int32, device=eng.device)

        def call():
            L.check(eng.lib.mamdr_rank_slates(eng.ctx, 0, n_query, p(d_uid), p(d_off), p(d_ids), p(scores), p(pos), p(order)))
        res["ms"] = timed(eng, call, args.reps)
        got = pos.cpu().numpy().reshape(n_query, length)
        assert (np.sort(got, axis=1) == np.arange(length)).all()
        sc = scores.cpu().numpy().reshape(n_query, length)
        assert (np.diff(np.take_along_axis(sc, order.cpu().numpy().reshape(n_query, length), 1), axis=1) <= 0).all()
        eng.profile(True)
        eng.profile_reset()
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize(eng.device)
        for name, slot in (("item_ms", L.KERNEL_GATHER), ("pair_ms", L.KERNEL_EVAL), ("order_ms", L.KERNEL_AUX)):
            ms, cnt = eng.profile_read(slot)
            res[name], res[name.replace("_ms", "_launches")] = ms / args.reps, cnt // args.reps
        eng.profile(False)
    else:
        union = np.unique(ids)
        d_cand = torch.from_numpy(union.astype(np.int32)).to(eng.device)
        out_i = torch.empty((n_query, 1), dtype=torch.int32, device=eng.device)
        out_s = torch.empty((n_query, 1), dtype=torch.float32, device=eng.device)
        dense = torch.empty((n_query, union.size), dtype=torch.float32, device=eng.device)

        def call():
            L.check(eng.lib.mamdr_recommend_domain(eng.ctx, 0, n_query, p(d_uid), p(d_cand), union.size, None, None, 1,
                                                   p(out_i), p(out_s), p(dense)))
        res["ms"] = timed(eng, call, args.reps)
        res["union"], res["pairs"] = int(union.size), int(union.size) * n_query
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tower", default="mlp", choices=["mlp", "wdl", "deepfm", "star"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", default=None, choices=["slates", "union"])
    ap.add_argument("--shape", default=None, choices=sorted(SHAPES))
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slate_bench.txt"))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    text = ""
    # one child per (shape, leg), each under its own time limit; a failed leg ends the run
    for shape in ("4096x100", "256x4096"):
        got = {}
        for name in ("slates", "union"):
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                   "--shape", shape, "--tower", args.tower, "--reps", str(args.reps)]
            run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                raise SystemExit("leg %s of %s failed (exit %d): nothing further is started" % (name, shape, run.returncode))
            got[name] = json.loads(lines[-1][7:])
        a, b = got["slates"], got["union"]
        timed_sum = a["item_ms"] + a["pair_ms"] + a["order_ms"]
        text += ("%s  %s  tower %s  %d slates x %d entries = %d pairs, domain 0, %d reps (HIP events, 2 warm-up calls, a process "
                 "per leg)\n"
                 "  mamdr_rank_slates (scores, pos, order)            %9.3f ms / call  %8.1f M pairs/s\n"
                 "    profile slots, a run of their own:  item term %8.3f ms (%4.1f %%, %d launches)  pair tiles %8.3f ms (%4.1f %%, "
                 "%d)  k_slate_order %8.3f ms (%4.1f %%, %d)   [shares of their sum %.3f ms]\n"
                 "  mamdr_recommend_domain(k = 1, dense scores) over the union of %d items = %d pairs  %9.3f ms / call   "
                 "union / slates = %.1fx\n" % (
                     time.strftime("%Y-%m-%d"), a["device"], args.tower, a["queries"], a["length"], a["entries"], a["reps"],
                     a["ms"], a["entries"] / (a["ms"] * 1e-3) / 1e6,
                     a["item_ms"], 100 * a["item_ms"] / timed_sum, a["item_launches"],
                     a["pair_ms"], 100 * a["pair_ms"] / timed_sum, a["pair_launches"],
                     a["order_ms"], 100 * a["order_ms"] / timed_sum, a["order_launches"], timed_sum,
                     b["union"], b["pairs"], b["ms"], b["ms"] / a["ms"]))
    print(text)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
