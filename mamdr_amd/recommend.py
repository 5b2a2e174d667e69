"""Host side of top-K retrieval (`mamdr_recommend`, include/mamdr_hip.h), of the exact full-catalogue ranks
(`mamdr_rank_domain`) and of per-query slates (`mamdr_rank_slates`: `slates_csr`, `sample_negatives`, `sampled_report` behind
`run.py --sampled-eval N`): the exclusion and target lists' CSR form, ranking metrics from top-K lists (`ranking_metrics`) and from
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


def slates_csr(slates, n_query):
    """`slates` -- one array of item ids per query, DISTINCT inside a slate, a slate may be empty or None -- as the CSR
    `mamdr_rank_slates` takes: (offsets int64 [n_query + 1], ids int32), every slate in the caller's order."""
    if len(slates) != n_query:
        raise ValueError("slates lists %d queries, the call has %d" % (len(slates), n_query))
    rows = [np.asarray(e if e is not None else (), np.int64).ravel() for e in slates]
    off = np.zeros(n_query + 1, np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    ids = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if ids.size and (ids.min() < 0 or ids.max() > np.iinfo(np.int32).max):
        raise ValueError("slates: item id out of range")
    if ids.size:
        q = np.repeat(np.arange(n_query), np.diff(off))
        o = np.lexsort((ids, q))
        same = (ids[o][1:] == ids[o][:-1]) & (q[o][1:] == q[o][:-1])
        if same.any():
            raise ValueError("slates: item %d is listed twice in the slate of query %d" % (
                ids[o][1:][same][0], q[o][1:][same][0]))
    return off, ids.astype(np.int32)


SAMPLE_ROUNDS = 16      # vectorised rejection rounds of sample_negatives before the per-slate completion
SAMPLE_SCAN_MAX = 8     # forbidden lists up to this length are compared entry by entry, longer ones searched (the same answer)


def sample_negatives(catalogue, forbid_off, forbid_ids, n_neg, seed):
    """`n_neg` items per slate, drawn uniformly without replacement from `catalogue` (item ids; taken as a set) minus the
    slate's forbidden ids forbid_ids[forbid_off[s] : forbid_off[s + 1]] (any order, duplicates and ids outside the catalogue
    allowed).  A slate with fewer free items than n_neg gets all of them.  -> (offsets int64 [S + 1], ids int64): slate s's
    draws at ids[offsets[s] : offsets[s + 1]], min(n_neg, free) of them.  A function of its arguments only: the stream is
    numpy's RandomState(seed), whose values are frozen.
    Vectorised rejection over all slates at once: every open position draws a catalogue index; a draw that is forbidden or
    equals another position of its slate is drawn again in the next round (of two equal positions the first stays).  The
    procedure never looks at an item's value except to compare it, so every free item is as likely as any other and every
    set of the right size equally likely.  Slates still open after SAMPLE_ROUNDS rounds -- those that take nearly all of
    their free items -- are completed one by one from their explicit free set."""
    cat = np.unique(np.asarray(catalogue, np.int64).ravel())
    off = np.asarray(forbid_off, np.int64).ravel()
    fid = np.asarray(forbid_ids, np.int64).ravel()
    n_slate, n_cat, n_neg = off.size - 1, int(cat.size), int(n_neg)
    if n_slate < 0 or n_neg < 0 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != fid.size:
        raise ValueError("sample_negatives: forbid_off [S + 1] ascending from 0 to len(forbid_ids), n_neg >= 0")
    # the forbidden (slate, catalogue index) pairs as sorted distinct keys slate * n_cat + index
    keys = np.zeros(0, np.int64)
    if fid.size and n_cat:
        idx = np.minimum(np.searchsorted(cat, fid), n_cat - 1)
        hit = cat[idx] == fid
        keys = np.unique(np.repeat(np.arange(n_slate, dtype=np.int64), np.diff(off))[hit] * n_cat + idx[hit])
    n_forbid = np.bincount(keys // max(n_cat, 1), minlength=n_slate)[:n_slate] if n_slate else np.zeros(0, np.int64)
    want = np.minimum(n_neg, n_cat - n_forbid).astype(np.int64)
    # short forbidden lists as a table [slate][SAMPLE_SCAN_MAX or fewer] of catalogue indices (-1: none): a few whole-array
    # comparisons per round instead of one binary search per draw
    f_max = int(n_forbid.max()) if n_slate else 0
    forbid = None
    if keys.size and f_max <= SAMPLE_SCAN_MAX:
        ks = keys // n_cat
        forbid = np.full((n_slate, f_max), -1, np.int32)
        forbid[ks, np.arange(keys.size) - (np.cumsum(n_forbid) - n_forbid)[ks]] = keys - ks * n_cat
    rs = np.random.RandomState(int(seed))
    draws = np.zeros((n_slate, n_neg), np.int32)          # (catalogue indices; the sentinels below reach n_cat + n_neg)
    col = np.arange(n_neg, dtype=np.int32)[None, :]
    todo = np.flatnonzero(want > 0)
    redraw = col < want[todo][:, None]
    # (value, position) packed into one integer per draw: a plain sort of distinct keys is the stable sort by value
    shift = max(int(max(n_neg, 1) - 1).bit_length(), 1)
    packed = np.int32 if ((n_cat + n_neg) << shift) < 2 ** 31 else np.int64
    for _ in range(SAMPLE_ROUNDS):
        if not todo.size:
            break
        active = col < want[todo][:, None]
        d = draws[todo]
        new = rs.randint(0, n_cat, size=int(redraw.sum()))
        d[redraw] = new
        bad = np.zeros_like(active)
        if forbid is not None:
            f = forbid[todo]
            for j in range(f_max):
                bad |= d == f[:, j:j + 1]
        elif keys.size:     # (only the positions drawn in this round can be forbidden: the others passed when they were drawn)
            k = np.repeat(todo * n_cat, redraw.sum(1)) + new
            bad[redraw] = keys[np.minimum(np.searchsorted(keys, k), keys.size - 1)] == k
        # equal positions of a slate: sorted per row (positions behind the slate's end under distinct sentinels) they come
        # together in position order; all but the first are drawn again
        v = np.where(active, d, np.int32(n_cat) + col).astype(packed)
        v <<= shift
        v |= col
        v.sort(axis=1)
        pos = v & ((1 << shift) - 1)
        v >>= shift
        dup_sorted = np.zeros_like(active)
        dup_sorted[:, 1:] = v[:, 1:] == v[:, :-1]
        dup = np.zeros_like(active)
        np.put_along_axis(dup, pos.astype(np.intp), dup_sorted, 1)
        redraw = (bad | dup) & active
        draws[todo] = d
        open_ = redraw.any(1)
        todo, redraw = todo[open_], redraw[open_]
    for s in todo.tolist():                       # (ascending: the stream's order is part of the function)
        lo, hi = np.searchsorted(keys, [s * n_cat, (s + 1) * n_cat])
        free = np.setdiff1d(np.arange(n_cat, dtype=np.int64), keys[lo:hi] - s * n_cat, assume_unique=True)
        draws[s, :want[s]] = rs.choice(free, int(want[s]), replace=False)
    out_off = np.zeros(n_slate + 1, np.int64)
    np.cumsum(want, out=out_off[1:])
    return out_off, cat[draws[col < want[:, None]]] if n_cat else np.zeros(0, np.int64)


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


def sampled_report(model, n_neg, ks, seed=0, out_path=None):
    """`run.py --sampled-eval N`: the sampled-negatives protocol -- for every domain, each (user, positive) pair of its test
    split ranked among N items the user never interacted with (model.sampled_eval; under the wrappers that keep a phi_d per
    domain, the best theta (+|*) phi_d of THAT domain) --, with MRR and HitRate / NDCG at every K of `ks` averaged over
    the pairs (rank_metrics with one slate per query), written to ONE .npz -- domains, ks, n_neg, seed, per domain d users_d /
    positives_d / rank_d [S], offsets_d [S + 1], ids_d / scores_d / pos_d [E]; n_short [n domains], mrr / mean_percentile
    [n domains], hit_rate / recall / ndcg [n domains, len(ks)] -- and printed, one line per domain.
    -> (path, {domain: metrics})."""
    ks, n_neg, seed = [int(k) for k in ks], int(n_neg), int(seed)
    domains = sorted(model.dataset.test_dataset)
    arrays = {"domains": np.asarray(domains, np.int64), "ks": np.asarray(ks, np.int64), "n_neg": np.asarray(n_neg, np.int64),
              "seed": np.asarray(seed, np.int64)}
    metrics = {}
    print("Sampled eval ({} negatives per positive, seed {}): ".format(n_neg, seed))
    for d in domains:
        r = model.sampled_eval(d, n_neg, seed=seed)
        n_slate = r["rank"].shape[0]
        m = rank_metrics(np.arange(n_slate + 1), r["rank"], np.ones(n_slate, bool), r["slate_len"], np.ones(n_slate, np.int64), ks)
        m["n_short"] = int(r["n_short"])
        metrics[d] = m
        for name in ("users", "positives", "offsets", "ids", "scores", "pos", "rank"):
            arrays["%s_%d" % (name, d)] = r[name]
        print("{}: MRR {:.4f} {} ({} pairs, {} short slates; random ranking: {})".format(
            d, m["mrr"],
            " ".join("HitRate@{k} {:.4f} NDCG@{k} {:.4f}".format(m["hit_rate"][i], m["ndcg"][i], k=k) for i, k in enumerate(ks)),
            m["n_eval"], m["n_short"],
            " ".join("HitRate@{} {:.4f}".format(k, min(1.0, float(k) / (n_neg + 1))) for k in ks)))
    for name in ("mrr", "mean_percentile", "hit_rate", "recall", "ndcg"):
        arrays[name] = np.asarray([metrics[d][name] for d in domains], np.float64)
    arrays["n_short"] = np.asarray([metrics[d]["n_short"] for d in domains], np.int64)
    if out_path is None:
        out_path = os.path.join(model.result_path, "sampled_eval_neg%d.npz" % n_neg)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Sampled evaluation written to {}".format(out_path))
    return out_path, metrics
