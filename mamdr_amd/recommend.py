"""Host side of top-K retrieval (`mamdr_recommend`, include/mamdr_hip.h): the exclusion lists' CSR form, ranking metrics,
and the per-domain report behind `run.py --recommend K`.  Pure numpy.  The reference has no counterpart: its pipeline
ends at per-domain loss and AUC (base_model.py:111-144).
"""
import os

import numpy as np


def exclusion_csr(exclude, n_query):
    """`exclude` -- one array of item ids per query (None or empty: nothing excluded), in any order, duplicates allowed --
    as the CSR `mamdr_recommend` takes: (offsets int64 [n_query + 1], ids int32, ascending and distinct per query)."""
    if len(exclude) != n_query:
        raise ValueError("exclude lists %d queries, the call has %d" % (len(exclude), n_query))
    rows = [np.unique(np.asarray(e if e is not None else (), np.int64).ravel()) for e in exclude]
    off = np.zeros(n_query + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    ids = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if ids.size and (ids.min() < 0 or ids.max() > np.iinfo(np.int32).max):
        raise ValueError("exclude: item id out of range")
    return off, ids.astype(np.int32)


def ranking_metrics(ids, positives):
    """HitRate@K, Recall@K and NDCG@K of ranked lists `ids` [Q, K] (-1 = padding behind a short list) against each query's
    set of positive items `positives` (Q arrays), averaged over the queries that HAVE a positive (the others say nothing
    about a ranking): {"hit_rate", "recall", "ndcg", "n_eval"}; all three are 0 when no query has one.
    NDCG with binary gains: DCG = sum over hits at 0-based rank r of 1 / log2(r + 2), IDCG = the same sum over the first
    min(K, |positives|) ranks."""
    ids = np.asarray(ids)
    if ids.ndim != 2 or len(positives) != ids.shape[0]:
        raise ValueError("ids must be [Q, K] with one positive set per query")
    K = ids.shape[1]
    discount = 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)
    hit = recall = ndcg = 0.0
    n = 0
    for row, pos in zip(ids, positives):
        pos = np.unique(np.asarray(pos, np.int64).ravel())
        if pos.size == 0:
            continue
        n += 1
        rel = np.isin(row, pos) & (row >= 0)
        hit += float(rel.any())
        recall += rel.sum() / float(pos.size)
        ndcg += float((rel * discount).sum() / discount[:min(K, pos.size)].sum()) if K else 0.0
    if n == 0:
        return {"hit_rate": 0.0, "recall": 0.0, "ndcg": 0.0, "n_eval": 0}
    return {"hit_rate": hit / n, "recall": recall / n, "ndcg": ndcg / n, "n_eval": n}


def split_positives(dataset, domain, users):
    """the items each of `users` has with label 1 in the domain's test split."""
    c = dataset.test_dataset[domain]["data"]
    uid, pid = np.asarray(c["uid"]), np.asarray(c["pid"])
    keep = np.asarray(c["label"]) > 0
    by_user = {}
    for u, p in zip(uid[keep].tolist(), pid[keep].tolist()):
        by_user.setdefault(u, []).append(p)
    return [np.asarray(by_user.get(int(u), ()), np.int64) for u in users]


def report(model, k, out_path=None):
    """`run.py --recommend K`: for every domain the top K of its catalogue for the users of its test split (items seen in
    train / val left out), written to ONE .npz -- domains, and per domain d users_d [Q], ids_d [Q, K], scores_d [Q, K];
    hit_rate / recall / ndcg [n domains] against the test split's positives -- and printed.  -> (path, {domain: metrics})."""
    domains = sorted(model.dataset.test_dataset)
    arrays, metrics = {"domains": np.asarray(domains, np.int64), "k": np.asarray(k, np.int64)}, {}
    print("Recommend top-{}: ".format(k))
    for d in domains:
        r = model.recommend(d, k)
        m = ranking_metrics(r["ids"], split_positives(model.dataset, d, r["users"]))
        m["catalogue"] = int(r["catalogue"])
        metrics[d] = m
        arrays["users_%d" % d], arrays["ids_%d" % d], arrays["scores_%d" % d] = r["users"], r["ids"], r["scores"]
        print("{}: HitRate@{} {:.4f} Recall@{} {:.4f} NDCG@{} {:.4f} ({} users, {} items; random ranking: HitRate {:.4f})".format(
            d, k, m["hit_rate"], k, m["recall"], k, m["ndcg"], m["n_eval"], m["catalogue"],
            min(1.0, float(k) / max(1, m["catalogue"]))))
    for name in ("hit_rate", "recall", "ndcg"):
        arrays[name] = np.asarray([metrics[d][name] for d in domains], np.float64)
    if out_path is None:
        out_path = os.path.join(model.result_path, "recommend_top%d.npz" % k)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Recommendations written to {}".format(out_path))
    return out_path, metrics
