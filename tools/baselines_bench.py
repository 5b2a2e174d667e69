"""The baselines' four device calls and the report behind `run.py --rank-eval --baselines`, timed on the GPU:

    python tools/baselines_bench.py [--out profiles/baselines_bench.txt]          every leg, one process each
    python tools/baselines_bench.py --leg scores:taobao                           one leg: <cooc|scores|select|report>:<taobao|dense>

Problems.  "taobao": the largest domain (by test users) of the full-size Taobao-10 data of config/Taobao-10/deepctr_DN+DR.json
under the rank-eval protocol -- its catalogue, its train histories, its test users, their exclusions and targets.  "dense":
a synthetic catalogue of 6,932 items (C = 192 MB: beyond the L2, inside the Infinity Cache) with 4,096 users of 64 random
items each, which gives mamdr_history_scores enough rows of C to stream for a rate to mean something (the shipped histories
hold 1.9 items on average).
Legs.  cooc: mamdr_item_cooc with its sum of L^2.  scores: mamdr_history_scores over one block of 256 queries and over all
queries, with the requested bytes of C rows (sum of L_q * m * 4) over the time.  select: mamdr_rank_scores and
mamdr_topk_scores (k = 10) on the ItemKNN score matrix and on the one MostPopular row.  report (taobao only): wall time of
recommend.rank_report and of baselines.report behind it on the same freshly built model (untrained weights: the cost does not
depend on their values), device synchronised on both sides.
Method: two warm-up calls, then five calls, each between two HIP events of its own on the current stream; the median is
reported, with min and max.  One process per leg.  No time is reported unless the device's outputs equal the host
definitions' (baselines.cooc_host, history_scores_host's fp32 replay byte for byte, rank_scores_host, topk_scores_host) on the
leg's own problem -- on its first 64 queries where the host loop would take minutes.
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
LEGS = ["cooc:taobao", "scores:taobao", "select:taobao", "cooc:dense", "scores:dense", "select:dense", "report:taobao"]
CONFIG = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
CHECKED = 64            # queries held to the host definitions before a time is reported
SHRINK = 10.0


def timed(fn):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def config():
    with open(CONFIG) as f:
        cfg = json.load(f)
    os.chdir(ROOT)          # (the dataset paths of the shipped configs are relative to the repository)
    return cfg


def problem(which):
    """-> {"m", "off", "pos", "query" (user indices into the CSR, -1: no history), "cand", "excl" CSR, "tgt" CSR, "pop" fp32 [m], "name"}."""
    from mamdr_amd import baselines as bl
    from mamdr_amd import recommend as rec
    if which == "dense":
        rs = np.random.RandomState(7)
        m, n_user, L = 6932, 4096, 64
        rows = np.sort(np.argsort(rs.random_sample((n_user, m)), axis=1)[:, :L], axis=1)
        off, pos = np.arange(n_user + 1, dtype=np.int64) * L, rows.ravel().astype(np.int32)
        cand = np.arange(m, dtype=np.int32)
        excl = rec.exclusion_csr([rows[u] for u in range(n_user)], n_user)
        tgt = rec.exclusion_csr([rs.choice(m, 3, replace=False) for _ in range(n_user)], n_user, "targets")
        return {"m": m, "off": off, "pos": pos, "query": np.arange(n_user, dtype=np.int32), "cand": cand, "excl": excl, "tgt": tgt,
                "pop": np.bincount(pos, minlength=m).astype(np.float32), "name": "dense (m 6,932, 4,096 users x 64 items)"}
    from mamdr_amd.model_zoo.base_model import BaseModel
    from mamdr_amd.utils import MultiDomainDataset
    ds = MultiDomainDataset(config()["dataset"])
    d = max(ds.test_dataset, key=lambda x: np.unique(ds.test_dataset[x]["data"]["uid"]).size)

    class Protocol(object):             # _retrieval_problem reads the dataset only
        dataset = ds
    catalogue, users, exclude = BaseModel._retrieval_problem(Protocol(), d, None, True)
    h = bl.histories(ds, d, catalogue)
    at = np.minimum(np.searchsorted(h["users"], users), h["users"].size - 1)
    off, pos = bl.check_csr(h["off"], h["pos"], catalogue.size)
    return {"m": int(catalogue.size), "off": off, "pos": pos, "query": np.where(h["users"][at] == users, at, -1).astype(np.int32),
            "cand": catalogue.astype(np.int32), "excl": rec.exclusion_csr(exclude, users.size),
            "tgt": rec.exclusion_csr(rec.split_positives(ds, d, users), users.size, "targets"),
            "pop": h["popularity"].astype(np.float32),
            "name": "Taobao-10 domain %d (m %d, %d users with a history, %d test users)" % (d, catalogue.size, h["users"].size, users.size)}


def leg(what, which):
    import torch
    from mamdr_amd import _lib
    from mamdr_amd import baselines as bl
    if not torch.cuda.is_available():
        sys.exit("baselines_bench: no HIP device (a CPU run gives no time)")
    if what == "report":
        return report_leg()
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    pr = problem(which)
    m, off, pos, query = pr["m"], pr["off"], pr["pos"], pr["query"]
    n_user, nnz, nq = off.size - 1, pos.size, query.size
    d_off, d_pos, d_q = up(off), up(pos), up(query)
    cooc = torch.empty((m, m), dtype=torch.int32, device="cuda")
    run_cooc = lambda: _lib.check(lib.mamdr_item_cooc(p(d_off), p(d_pos), nnz, n_user, m, p(cooc), s))      # noqa: E731
    run_cooc()
    host_c = bl.cooc_host(off, pos, m)
    assert np.array_equal(cooc.cpu().numpy().view(np.uint32), host_c), "mamdr_item_cooc differs from cooc_host"
    head = "%-7s %s" % (what, pr["name"])
    if what == "cooc":
        med, lo, hi = timed(run_cooc)
        pairs = bl.pair_counts(off)
        print("%s: mamdr_item_cooc (memset of %.0f MB + %d adds = sum L^2; dense form: n_user m^2 = %.2e)   median %8.3f ms  "
              "(min %8.3f  max %8.3f)" % (head, 4e-6 * m * m, pairs, float(n_user) * m * m, med, lo, hi), flush=True)
        return
    lengths = np.where(query >= 0, np.diff(off)[np.maximum(query, 0)], 0)
    scores = torch.empty((nq, m), dtype=torch.float32, device="cuda")

    def run_scores(n):
        _lib.check(lib.mamdr_history_scores(p(cooc), m, p(d_off), p(d_pos), nnz, n_user, p(d_q), n, SHRINK, p(scores), s))
    run_scores(nq)
    want = bl.history_scores_host(host_c, off, pos, query[:CHECKED], SHRINK)
    assert scores[:CHECKED].cpu().numpy().tobytes() == want.tobytes(), "mamdr_history_scores differs from the fp32 replay"
    if what == "scores":
        for n in (min(256, nq), nq):
            med, lo, hi = timed(lambda: run_scores(n))
            req = float(lengths[:n].sum()) * m * 4
            print("%s: mamdr_history_scores %5d queries (sum L_q %d, %.1f MB of C rows requested, %.1f MB of scores written)   "
                  "median %8.3f ms  (min %8.3f  max %8.3f)   %7.1f GB/s of C rows" % (
                      head, n, int(lengths[:n].sum()), req / 1e6, 4e-6 * n * m, med, lo, hi, req / (med * 1e-3) / 1e9), flush=True)
        return
    d_cand, (e_off, e_ids), (t_off, t_ids) = up(pr["cand"]), pr["excl"], pr["tgt"]
    d_eo, d_ei, d_to, d_ti = up(e_off), up(e_ids if e_ids.size else np.zeros(1, np.int32)), up(t_off), up(t_ids)
    n_tgt, k = int(t_ids.size), 10
    ranks = torch.empty(n_tgt, dtype=torch.int32, device="cuda")
    live = torch.empty(nq, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    top = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    row = up(pr["pop"])
    for who, src, stride in (("ItemKNN matrix", scores, m), ("MostPopular row", row, 0)):
        run_rank = lambda: _lib.check(lib.mamdr_rank_scores(p(src), stride, nq, p(d_cand), m, p(d_eo), p(d_ei), p(d_to), p(d_ti),     # noqa: E731
                                                            n_tgt, p(ranks), None, p(live), s))
        run_topk = lambda: _lib.check(lib.mamdr_topk_scores(p(src), stride, nq, p(d_cand), m, p(d_eo), p(d_ei), k, p(ids), p(top), s))   # noqa: E731
        run_rank()
        run_topk()
        n = CHECKED
        host_s = src[:n].cpu().numpy() if stride else src.cpu().numpy()
        w_r, w_l, _ = bl.rank_scores_host(host_s, n, t_off[:n + 1], t_ids[:t_off[n]], pr["cand"], e_off[:n + 1], e_ids[:e_off[n]])
        w_i, w_s = bl.topk_scores_host(host_s, n, k, pr["cand"], e_off[:n + 1], e_ids[:e_off[n]])
        assert np.array_equal(ranks[:t_off[n]].cpu().numpy(), w_r) and np.array_equal(live[:n].cpu().numpy(), w_l), "mamdr_rank_scores differs"
        assert np.array_equal(ids[:n].cpu().numpy(), w_i) and top[:n].cpu().numpy().tobytes() == w_s.tobytes(), "mamdr_topk_scores differs"
        for name, fn in (("mamdr_rank_scores", run_rank), ("mamdr_topk_scores k = 10", run_topk)):
            med, lo, hi = timed(fn)
            print("%s: %-24s %-15s %5d queries x %d candidates, %d targets   median %8.3f ms  (min %8.3f  max %8.3f)" % (
                head, name, who, nq, m, n_tgt, med, lo, hi), flush=True)


def report_leg():
    import io
    import contextlib
    import tempfile
    import torch
    from mamdr_amd import baselines as bl
    from mamdr_amd import cli
    from mamdr_amd import recommend as rec
    from mamdr_amd.utils import MultiDomainDataset
    cfg = config()
    cfg["model"]["name"] = "mlp"
    tmp = tempfile.mkdtemp()
    cfg["train"].update(result_save_path=os.path.join(tmp, "result"), checkpoint_path=os.path.join(tmp, "ckpt"))
    model = cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    ks = [10, 50]

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()) as text:
            out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out, text.getvalue()
    wall(lambda: rec.rank_report(model, ks))                # (warm-up of both: workspaces, code objects, the allocator)
    wall(lambda: bl.report(model, ks, 10, shrink=SHRINK))
    t_rank, (_, tower), _ = wall(lambda: rec.rank_report(model, ks))
    t_rec, _, _ = wall(lambda: [model.recommend(d, 10) for d in sorted(model.dataset.test_dataset)])
    t_base, _, text = wall(lambda: bl.report(model, ks, 10, shrink=SHRINK, tower=tower))
    d = 5
    assert np.array_equal(bl.rank(model, d, "pop")["ranks"], bl.rank_host(model, d, "pop")["ranks"]), "MostPopular differs from the host"
    print("report  Taobao-10, all 10 domains, mlp tower: recommend.rank_report %7.3f s wall; baselines.report behind it %7.3f s wall "
          "(of which the tower's own top-10 lists for the overlap: %.3f s)" % (t_rank, t_base, t_rec), flush=True)
    print("        (the quality table of the UNTRAINED tower is no finding; a trained run's table: DESIGN section 22)")
    print("\n".join("        " + line for line in text.splitlines() if line[:1].isdigit() and int(line.split(":")[0]) == d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        what, which = args.leg.split(":")
        return leg(what, which)
    lines = ["baselines: co-occurrence counts, ItemKNN scores, ranks and top-K lists from scores; 5 calls after 2 warm-up calls, one "
             "process per leg; every leg's device outputs equal the host definitions'"]
    for name in LEGS:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], stdout=subprocess.PIPE,
                             universal_newlines=True, timeout=400)
        if res.returncode != 0:
            sys.exit("baselines_bench: leg %s ended with %d" % (name, res.returncode))
        keep = [ln for ln in res.stdout.splitlines() if ln.startswith((name.split(":")[0], "        "))]
        lines += ["  " + ln for ln in keep]
        print("\n".join("  " + ln for ln in keep), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
