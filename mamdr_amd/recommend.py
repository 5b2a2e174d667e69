"""Host side of top-K retrieval (`mamdr_recommend`, include/mamdr_hip.h) and of the exact full-catalogue ranks
(`mamdr_rank_domain`): the exclusion and target lists' CSR form, ranking metrics from top-K lists (`ranking_metrics`) and from
ranks (`rank_metrics`), and the per-domain reports behind `run.py --recommend K` and `run.py --rank-eval KS`.  Pure numpy.  The reference has no counterpart: its pipeline
ends at per-domain loss and AUC (base_model.py:111-144).
"""
import os

import numpy as np


def exclusion_csr(exclude, n_query, what="exclude"):
    """`exclude` -- one array of item ids per query (None or empty: nothing excluded), in any order, duplicates allowed --
    as the CSR `mamdr_recommend` takes: (offsets int64 [n_query + 1], ids int32, ascending and distinct per query).
    `mamdr_rank_domain`'s target lists take the same form (`what` names the list in the errors)."""
    if len(exclude) != n_query:
        raise ValueError("%s lists %d queries, the call has %d" % (what, len(exclude), n_query))
    rows = [np.unique(np.asarray(e if e is not None else (), np.int64).ravel()) for e in exclude]
    off = np.zeros(n_query + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    ids = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if ids.size and (ids.min() < 0 or ids.max() > np.iinfo(np.int32).max):
        raise ValueError("%s: item id out of range" % what)
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


def rank_metrics(offsets, ranks, listed, live, n_positives, ks):
    """MRR, mean percentile rank and HitRate / Recall / NDCG at every K of `ks` from exact ranks (`mamdr_rank_domain`):
    offsets [Q + 1] and ranks / listed [T] are the targets' CSR, their 0-based ranks and whether each is among the live
    candidates of its query (an unlisted target is a miss at every K); live [Q] the queries' live candidates; n_positives [Q]
    the number of positives each query is held against.  fp64.  Only queries with n_positives > 0 count (`n_eval` of them):
      hit_rate[K] = any listed rank < K;  recall[K] = #(listed ranks < K) / n_positives[q];
      ndcg[K]     = sum over listed r < K of 1 / log2(r + 2), divided by the same sum over the first min(K, n_positives[q])
                    ranks -- `ranking_metrics`' definitions, so for K <= 128 both routes agree;
      mrr         = mean over those queries of 1 / (1 + the smallest listed rank), 0 where nothing is listed;
      mean_percentile = mean over their listed targets of rank / max(1, live[q] - 1)  (0 = first, 1 = last).
    -> {"ks", "hit_rate" [len(ks)], "recall", "ndcg", "mrr", "mean_percentile", "n_eval"}; everything 0 without a positive."""
    offsets, ranks = np.asarray(offsets, np.int64), np.asarray(ranks, np.int64)
    listed, live, n_pos = np.asarray(listed, bool), np.asarray(live, np.int64), np.asarray(n_positives, np.int64)
    ks = [int(k) for k in ks]
    nq = offsets.shape[0] - 1
    if ranks.shape != listed.shape or ranks.ndim != 1 or live.shape != (nq,) or n_pos.shape != (nq,) or \
            (nq >= 0 and offsets[-1] != ranks.shape[0]):
        raise ValueError("rank_metrics: offsets [Q + 1], ranks / listed [T], live / n_positives [Q] do not fit together")
    hit, recall, ndcg = np.zeros(len(ks)), np.zeros(len(ks)), np.zeros(len(ks))
    mrr = pct_sum = 0.0
    n = n_pct = 0
    for q in range(nq):
        if n_pos[q] <= 0:
            continue
        n += 1
        sl = slice(offsets[q], offsets[q + 1])
        r = np.sort(ranks[sl][listed[sl]])
        if r.size:
            mrr += 1.0 / (1.0 + float(r[0]))
            pct_sum += float((r / float(max(1, live[q] - 1))).sum())
            n_pct += r.size
        for i, k in enumerate(ks):
            in_k = r[r < k]
            hit[i] += float(in_k.size > 0)
            recall[i] += in_k.size / float(n_pos[q])
            ideal = (1.0 / np.log2(np.arange(min(k, int(n_pos[q])), dtype=np.float64) + 2.0)).sum()
            ndcg[i] += float((1.0 / np.log2(in_k.astype(np.float64) + 2.0)).sum() / ideal) if ideal > 0 else 0.0
    d = float(max(n, 1))
    return {"ks": ks, "hit_rate": hit / d, "recall": recall / d, "ndcg": ndcg / d, "mrr": mrr / d,
            "mean_percentile": pct_sum / n_pct if n_pct else 0.0, "n_eval": n}


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


def rank_report(model, ks, out_path=None):
    """`run.py --rank-eval KS`: for every domain the exact rank of each test user's held-out positives in the domain's whole
    catalogue (model.rank_eval: items seen in train / val left out; under the wrappers that keep a phi_d per domain, the
    best theta (+|*) phi_d of THAT domain), written to ONE .npz -- domains, ks, per domain d users_d [Q], offsets_d [Q + 1],
    ids_d / ranks_d / listed_d [T], live_d [Q]; mrr / mean_percentile [n domains], hit_rate / recall / ndcg [n domains, len(ks)]
    -- and printed, one line per domain.  -> (path, {domain: metrics})."""
    ks = [int(k) for k in ks]
    domains = sorted(model.dataset.test_dataset)
    arrays, metrics = {"domains": np.asarray(domains, np.int64), "ks": np.asarray(ks, np.int64)}, {}
    print("Rank eval (exact ranks in the whole catalogue): ")
    for d in domains:
        r = model.rank_eval(d)
        m = rank_metrics(r["offsets"], r["ranks"], r["listed"], r["live"], r["n_positives"], ks)
        m["catalogue"] = int(r["catalogue"].shape[0])
        metrics[d] = m
        for name in ("users", "offsets", "ids", "ranks", "listed", "live"):
            arrays["%s_%d" % (name, d)] = r[name]
        print("{}: MRR {:.4f} MeanPercentile {:.4f} {} ({} users, {} items)".format(
            d, m["mrr"], m["mean_percentile"],
            " ".join("HitRate@{k} {:.4f} Recall@{k} {:.4f} NDCG@{k} {:.4f}".format(m["hit_rate"][i], m["recall"][i], m["ndcg"][i], k=k)
                     for i, k in enumerate(ks)), m["n_eval"], m["catalogue"]))
    for name in ("mrr", "mean_percentile", "hit_rate", "recall", "ndcg"):
        arrays[name] = np.asarray([metrics[d][name] for d in domains], np.float64)
    if out_path is None:
        out_path = os.path.join(model.result_path, "rank_eval.npz")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Ranks written to {}".format(out_path))
    return out_path, metrics
