"""Throughput of the generic-layer engine's retrieval calls (mamdr_graph_recommend_domain, mamdr_graph_rank_domain) beside
its own evaluation (mamdr_graph_eval_domain: the same forward, the yardstick) and, for mlp at [256, 128, 64] / E 128, beside
the step engine's mamdr_recommend_domain on the same problem.

Problem: full-size synthetic taobao10, batch 1024; one domain's test users x its catalogue (the distinct pids of its three
splits) through recommend_domain(k = 10) and, with every user's test items as targets, through rank_domain; evaluation over
the explicit triples of the first 256 of those users x the catalogue, bound as a split.  Random weights:
throughput does not depend on them.  Device events around whole calls (host marshalling and the copies of the arguments
included), the three calls alternating, after one warm-up round.

usage: python tools/graph_retrieval_bench.py [kind,kind,...|all [repeats [domain [max_users]]]]
kinds: ccpm autoint nfm pnn mlp64 (mlp at E 64, hidden [128, 64]) mlp (+ the step engine's mlp beside it); one JSON line per kind
(one process for every kind: a profiler may wrap the whole run)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mamdr_amd import engine, graph_engine, synthetic  # noqa: E402

KINDS = {"ccpm": ("ccpm", 128, (256, 128, 64)), "autoint": ("autoint", 128, (256, 128, 64)), "nfm": ("nfm", 128, (256, 128, 64)),
         "pnn": ("pnn", 128, (256, 128, 64)), "mlp64": ("mlp", 64, (128, 64)), "mlp": ("mlp", 128, (256, 128, 64))}
ONLY = sys.argv[1].split(",") if len(sys.argv) > 1 and sys.argv[1] != "all" else list(KINDS)
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
DOMAIN = int(sys.argv[3]) if len(sys.argv) > 3 else 0
MAX_USERS = int(sys.argv[4]) if len(sys.argv) > 4 else 0
BATCH = 1024


def bind(eng, g, rs):
    eng.bind_table("user_emb", g["tables"]["user_emb"])
    eng.bind_table("item_emb", g["tables"]["item_emb"])
    for split in ("train", "val", "test"):
        c = g["data"][split][DOMAIN]
        eng.bind_domain_data(DOMAIN, split, c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(torch.from_numpy((rs.standard_normal(eng.n_params) * 0.05).astype(np.float32)).to(eng.device))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def measure(name):
    kind, emb_dim, hidden = KINDS[name]
    g = synthetic.generate("taobao10", batch_size=BATCH, seed=7, scale=1.0, emb_dim=emb_dim)
    rs = np.random.RandomState(1)
    lib = engine.L.load()
    eng = graph_engine.GraphEngine(kind, g["n_user"], g["n_item"], g["n_domain"], BATCH, hidden, (), emb_dim=emb_dim)
    eng.enable_retrieval()              # (mlp: a bare engine of this kind serves the calls once asked to)
    bind(eng, g, rs)
    test = g["data"]["test"][DOMAIN]
    users = np.unique(test["uid"])
    if MAX_USERS:
        users = users[:MAX_USERS]
    cat = np.unique(np.concatenate([g["data"][s][DOMAIN]["pid"] for s in ("train", "val", "test")])).astype(np.int32)
    targets = [test["pid"][test["uid"] == u] for u in users]
    n_pairs = users.size * cat.size
    n_tgt = int(sum(np.unique(t).size for t in targets))
    # the yardstick's split: explicit triples, the first 256 users x the catalogue (full batches but the last), bound as "val"
    e_uid = np.repeat(users[:256], cat.size).astype(np.int32)
    e_pid = np.tile(cat, min(256, users.size)).astype(np.int32)
    n_rows = int(e_uid.shape[0])
    eng.bind_domain_data(DOMAIN, "val", e_uid, e_pid, np.full(n_rows, DOMAIN, np.int32), np.zeros(n_rows, np.float32))
    calls = {"eval": lambda: eng.evaluate(DOMAIN, "val"),
             "recommend": lambda: eng.recommend_domain(users, DOMAIN, 10, candidates=cat),
             "rank": lambda: eng.rank_domain(users, DOMAIN, targets, candidates=cat)}
    step = None
    if name == "mlp":                   # the step engine on the same problem: the first layer separated by field
        step = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], BATCH, tower="mlp")
        bind(step, g, rs)
        calls["step_recommend"] = lambda: step.recommend_domain(users, DOMAIN, 10, candidates=cat)
    for fn in calls.values():           # warm-up: workspaces grown, kernels loaded
        fn()
    n0 = int(lib.mamdr_graph_launch_count())
    calls["recommend"]()
    launches = int(lib.mamdr_graph_launch_count()) - n0
    chunk_pad = (min(cat.size, 16384) + 63) // 64 * 64
    batches = sum(-(-(min(256, users.size - q) * chunk_pad) // BATCH) for q in range(0, users.size, 256))
    times = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, fn in calls.items():
            times[k].append(timed(fn))
    out = {"kind": name, "emb_dim": emb_dim, "hidden": list(hidden), "domain": DOMAIN, "users": int(users.size),
           "candidates": int(cat.size), "pairs": int(n_pairs), "targets": n_tgt, "eval_rows": n_rows, "max_batch": BATCH,
           "repeats": REPEATS, "forward_batches_per_recommend": int(batches),
           "launches_per_forward_batch": round(launches / float(batches), 3),
           "eval_rows_per_s": spread([n_rows / t for t in times["eval"]]),
           "recommend_pairs_per_s": spread([n_pairs / t for t in times["recommend"]]),
           "rank_pairs_per_s": spread([(n_pairs + n_tgt) / t for t in times["rank"]]),
           "seconds": {k: spread(v) for k, v in times.items()}}
    if step is not None:
        out["step_recommend_pairs_per_s"] = spread([n_pairs / t for t in times["step_recommend"]])
        step.close()
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device"
    for kind in ONLY:
        measure(kind)
