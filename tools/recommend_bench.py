"""pairs/s of mamdr_recommend beside the only way to score the same (user, item, domain) pairs without it:
mamdr_eval_domain with d_pred_out over a bound split that holds those triples (one full 384 -> 256 -> 128 -> 64 -> 1
forward per row).  Taobao-10-shaped synthetic data (23,778 users, 6,932 items, 10 domains), frozen tables, the mlp tower
by default.  --tower star: every query in domain 0 through mamdr_recommend_domain (the Star tower retrieves one domain per
call), the eval leg over the same triples as domain 0's split.

    python tools/recommend_bench.py [--tower mlp|wdl|deepfm|star] [--queries 512] [--k 10] [--reps 5] [--out profiles/recommend_bench.txt]
    python tools/recommend_bench.py --rank [--tower mlp|star] [--targets 3] [--out profiles/rank_bench.txt]

--rank: mamdr_rank_domain (exact ranks of `targets` random items per query among the whole item table, every query in domain
0) beside (b) mamdr_recommend_domain(k) over the same queries and (c) what a caller without it must do: recommend_domain with
the dense [queries, items] score matrix, its read-back and a numpy ranking per target -- (a) and (b) in device time by the
method below, (c) in wall time (two warm-up rounds, `reps` rounds).  The rank leg also checks the link to top-K on 8 queries;
the host leg counts the (query, target, tile) triples whose count is not zero -- the integer atomics of a call.

Method (device time): each leg runs in a child process of its own under `timeout -k 10`; inside it two warm-up calls, then
`reps` calls between two HIP events recorded on the engine's stream; the figure is elapsed / reps.  The recommend leg's
time covers all of its launches (query term, item term, scoring, merge); the eval leg's covers k_tower<eval> and its
loss / regulariser tail, as a caller of mamdr_eval_domain pays them.  Neither covers uploads or read-backs.  The recommend
leg also checks, for 8 of the queries, that both paths score the same pairs alike.  Nothing is tuned per leg: default
chunk, default tile sizes, the same queries and the whole item table as candidates.
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


def build(tower, batch):
    import torch  # noqa: F401
    from mamdr_amd import synthetic
    from mamdr_amd.engine import TowerEngine
    spec = synthetic.SHAPES["taobao10"]
    rs = np.random.RandomState(7)
    n_user, n_item, n_domain = spec["n_user"], spec["n_item"], spec["n_domain"]
    eng = TowerEngine(n_user, n_item, n_domain, batch, dropout=0.0, emb_trainable=False, tower=tower)
    eng.bind_table("user_emb", (rs.standard_normal((n_user, 128)) * 0.1).astype(np.float32))
    eng.bind_table("item_emb", (rs.standard_normal((n_item, 128)) * 0.1).astype(np.float32))
    scale = {"domain_emb": 0.05, "W0": 0.06, "W1": 0.07, "W2": 0.1, "wo": 0.17, "gb": 0.0}
    scale.update({"Ws0": 0.06, "Ws1": 0.07, "Ws2": 0.1})
    named = {n: (rs.standard_normal(cnt) * scale.get(n, 0.05)).astype(np.float32) for n, (off, cnt) in eng.segments.items()}
    for n in named:             # Star: PartitionedNorm's gammas and the per-domain kernel factors around one
        if n.startswith("pn_gamma") or n.startswith("Wd"):
            named[n] = (1.0 + 0.2 * rs.standard_normal(named[n].shape)).astype(np.float32)
    eng.set_weights(eng.pack(named))
    return eng, n_user, n_item, n_domain


def timed(eng, call, reps):
    import torch
    for _ in range(2):
        call()
    torch.cuda.synchronize(eng.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(eng.stream)
    for _ in range(reps):
        call()
    b.record(eng.stream)
    torch.cuda.synchronize(eng.device)
    return a.elapsed_time(b) / reps


def eval_preds(eng, uid, pid, dom, reps=0):
    """mamdr_eval_domain with d_pred_out over a split holding the triples -> (preds, ms per call or None)."""
    import torch
    from mamdr_amd import _lib as L
    eng.bind_domain_data(0, "test", uid, pid, dom, np.zeros(uid.shape[0], np.float32))
    preds = torch.empty(uid.shape[0], dtype=torch.float32, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def call():
        L.check(eng.lib.mamdr_eval_domain(eng.ctx, 0, L.SPLIT_TEST, eng.eval_batch, p(eng._loss1), p(eng._hist), p(preds)))
    ms = timed(eng, call, reps) if reps else (call(), None)[1]
    torch.cuda.synchronize(eng.device)
    return preds.cpu().numpy(), ms


def leg(args):
    import torch
    from mamdr_amd import _lib as L
    eng, n_user, n_item, n_domain = build(args.tower, 1024)
    rs = np.random.RandomState(3)
    uids = rs.choice(n_user, args.queries, replace=False).astype(np.int32)
    star = args.tower == "star" or args.rank          # (--rank: every leg in domain 0 through the single-domain calls)
    doms = np.zeros_like(uids) if star else (uids % n_domain).astype(np.int32)
    pairs = int(args.queries) * n_item
    res = {"leg": args.leg, "tower": args.tower, "queries": int(args.queries), "items": n_item, "pairs": pairs, "k": args.k,
           "device": torch.cuda.get_device_name(eng.device), "reps": args.reps}
    if args.leg in ("rank", "host"):
        targets = [rs.choice(n_item, args.targets, replace=False) for _ in range(args.queries)]
        res["targets"] = args.targets
    if args.leg == "rank":
        from mamdr_amd.recommend import exclusion_csr
        t_off, t_ids = exclusion_csr(targets, args.queries, "targets")
        d_uid, d_off, d_ids = (torch.from_numpy(x).to(eng.device) for x in (uids, t_off, t_ids))
        ranks = torch.empty(t_ids.size, dtype=torch.int32, device=eng.device)
        live = torch.empty(args.queries, dtype=torch.int32, device=eng.device)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def call():
            L.check(eng.lib.mamdr_rank_domain(eng.ctx, 0, args.queries, p(d_uid), None, 0, None, None, p(d_off), p(d_ids),
                                              p(ranks), None, p(live)))
        res["ms"] = timed(eng, call, args.reps)
        # the link to top-K (8 queries): a target of rank r < 128 is the r-th id of recommend_domain's list
        top = eng.recommend_domain(uids[:8], 0, 128)[0]
        got = ranks.cpu().numpy()
        for q in range(8):
            for j in range(t_off[q], t_off[q + 1]):
                assert (top[q, got[j]] == t_ids[j]) if got[j] < 128 else (t_ids[j] not in top[q]), (q, j)
        assert live.cpu().numpy().tolist() == [n_item] * args.queries
        res["mean_rank"] = float(got.mean())
    elif args.leg == "host":
        tiles = -(-n_item // 64)
        ids = np.arange(n_item)

        def round_trip():
            dense = eng.recommend_domain(uids, 0, args.k, want_scores=True)[2]
            out, atomics = [], 0
            for q in range(args.queries):
                row = dense[q]
                for t in np.unique(targets[q]):
                    before = (row > row[t]) | ((row == row[t]) & (ids < t))
                    out.append(int(before.sum()))
                    atomics += int(np.add.reduceat(before, np.arange(0, n_item, 64)).astype(bool).sum())
            return out, atomics
        for _ in range(2):
            round_trip()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            _, atomics = round_trip()
        res["ms"] = (time.perf_counter() - t0) / args.reps * 1e3
        res["rank_atomics"], res["rank_atomics_bound"] = atomics, args.queries * args.targets * tiles
        res["live_atomics"] = args.queries * tiles
    elif args.leg == "recommend":
        d_uid, d_dom = torch.from_numpy(uids).to(eng.device), torch.from_numpy(doms).to(eng.device)
        out_i = torch.empty((args.queries, args.k), dtype=torch.int32, device=eng.device)
        out_s = torch.empty((args.queries, args.k), dtype=torch.float32, device=eng.device)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

        def call():
            if star:
                L.check(eng.lib.mamdr_recommend_domain(eng.ctx, 0, args.queries, p(d_uid), None, 0, None, None, args.k,
                                                       p(out_i), p(out_s), None))
            else:
                L.check(eng.lib.mamdr_recommend(eng.ctx, args.queries, p(d_uid), p(d_dom), None, 0, None, None, args.k,
                                                p(out_i), p(out_s), None))
        res["ms"] = timed(eng, call, args.reps)
        # both paths score the same pairs alike (8 queries)
        if star:
            _, _, dense = eng.recommend_domain(uids[:8], 0, args.k, want_scores=True)
        else:
            _, _, dense = eng.recommend(uids[:8], doms[:8], args.k, want_scores=True)
        preds, _ = eval_preds(eng, np.repeat(uids[:8], n_item), np.tile(np.arange(n_item, dtype=np.int32), 8), np.repeat(doms[:8], n_item))
        res["max_abs_diff_vs_eval"] = float(np.abs(dense.ravel() - preds).max())
    else:
        _, res["ms"] = eval_preds(eng, np.repeat(uids, n_item), np.tile(np.arange(n_item, dtype=np.int32), args.queries),
                                  np.repeat(doms, n_item), reps=args.reps)
    res["pairs_per_s"] = pairs / (res["ms"] * 1e-3)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tower", default="mlp", choices=["mlp", "wdl", "deepfm", "star"])
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", default=None, choices=["recommend", "eval", "rank", "host"])
    ap.add_argument("--rank", action="store_true", help="the mamdr_rank_domain comparison (module docstring)")
    ap.add_argument("--targets", type=int, default=3)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rank_bench.txt" if args.rank else "recommend_bench.txt")
    if args.leg:
        return leg(args)
    got = {}
    # one child per leg, each under its own time limit; a failed leg ends the run
    for name in (("rank", "recommend", "host") if args.rank else ("recommend", "eval")):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--tower", args.tower, "--queries", str(args.queries), "--k", str(args.k), "--reps", str(args.reps),
               "--targets", str(args.targets)] + (["--rank"] if args.rank else [])
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not lines:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            raise SystemExit("leg %s failed (exit %d): nothing further is started" % (name, run.returncode))
        got[name] = json.loads(lines[-1][7:])
    if args.rank:
        a, b, c = got["rank"], got["recommend"], got["host"]
        tiles = -(-a["items"] // 64)
        text = ("%s  %s  tower %s  %d queries x %d items, %d targets per query, domain 0, %d reps (a, b: HIP events, 2 warm-up "
                "calls; c: wall time, 2 warm-up rounds; a process per leg)\n"
                "  a  mamdr_rank_domain                              %9.3f ms / call  (mean rank %.1f; link to top-128 checked on 8 queries)\n"
                "  b  mamdr_recommend_domain(k = %d)                 %9.3f ms / call   a / b = %.3f\n"
                "  c  recommend_domain(want_scores) + read-back + numpy ranks  %9.3f ms / round (wall)\n"
                "  tiles: pre-pass %d pair tiles, grid %d x %d = %d scoring tiles (pre-pass share %.4f)\n"
                "  integer atomics per call: ranks %d of at most %d (queries x targets x tiles, zero counts skipped; counted on "
                "the host from the score matrix), live counts %d\n" % (
                    time.strftime("%Y-%m-%d"), a["device"], args.tower, a["queries"], a["items"], a["targets"], a["reps"],
                    a["ms"], a["mean_rank"], b["k"], b["ms"], a["ms"] / b["ms"], c["ms"],
                    -(-a["queries"] * a["targets"] // 64), tiles, a["queries"], tiles * a["queries"],
                    -(-a["queries"] * a["targets"] // 64) / float(tiles * a["queries"]),
                    c["rank_atomics"], c["rank_atomics_bound"], c["live_atomics"]))
        print(text)
        with open(args.out, "a") as f:
            f.write(text)
        return
    r, e = got["recommend"], got["eval"]
    ratio = r["pairs_per_s"] / e["pairs_per_s"]
    text = ("%s  %s  tower %s  %d queries x %d items = %d pairs, K %d, %d reps (HIP events, 2 warm-up calls, a process per leg)\n"
            "  %-30s  %9.3f ms / call  %8.1f M pairs/s  (max |score - eval path's| over 8 queries: %.2e)\n"
            "  mamdr_eval_domain + d_pred_out  %9.3f ms / call  %8.1f M pairs/s\n"
            "  recommend / eval throughput     %.2fx  (flop per pair: 82,048 / 360,576 = 0.23)\n" % (
                time.strftime("%Y-%m-%d"), r["device"], args.tower, r["queries"], r["items"], r["pairs"], r["k"], r["reps"],
                "mamdr_recommend_domain (d = 0)" if args.tower == "star" else "mamdr_recommend",
                r["ms"], r["pairs_per_s"] / 1e6, r["max_abs_diff_vs_eval"], e["ms"], e["pairs_per_s"] / 1e6, ratio))
    print(text)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
