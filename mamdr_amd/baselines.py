"""Baselines under the rank-eval protocol (`run.py --rank-eval [KS] --baselines [SHRINK]`): MostPopular and ItemKNN ranked
with the candidates, exclusions, held-out positives and tie rule of `BaseModel.rank_eval`, so that a tower's figures have
something to stand against.  The documented host definitions of `mamdr_item_cooc`, `mamdr_history_scores`,
`mamdr_rank_scores` and `mamdr_topk_scores` (include/mamdr_hip.h) and the report built on the device calls.  No reference
counterpart.

Histories (`histories`).  The label-1 rows of a domain's train split as distinct (user, catalogue position) pairs, a CSR
over the sorted distinct users; `popularity` [m] counts the label-1 ROWS per position (duplicates included: what
`mamdr_id_counts` over the split's pid and label columns gives).  A pid outside the catalogue is dropped.

MostPopular.  Every user is scored with the one row float32(popularity); ties -- and there are many -- go by ascending id.

ItemKNN (cosine over co-occurrence, with shrinkage).  C[a][b] = the users whose history holds both items, n_a = C[a][a];
  sim(c, j) = float32(C[c][j]) / (sqrt(n_c) * sqrt(n_j) + shrink)   for c != j and C[c][j] > 0, else +0.0
  score(u, c) = the fp32 sum of sim(c, j) over j in H(u), in ascending j, from +0.0, one add per entry
each operation rounded to fp32 on its own (`history_scores_host`; dtype=np.float64 is the same formula in float64: the
fp32 form is within (L_u + 8) * 2^-24 relative of it -- 5 roundings per similarity, L_u - 1 adds of non-negative terms).
A test user with no train history in the domain (`n_cold`) gets an all-zero row and is ranked by the tie rule: counted,
not patched.

Ranking from scores.  key = (order-preserving bits of the score << 32) | ~id with -0 taken as +0 and NaN behind every
number (list_metrics.rank_keys on the canonical score); a position is live for a query when its id is not excluded;
rank(target) = the live positions whose key is greater than the key of the position that holds the target's id, -1 when
no position holds it; the top-K list is the first K live positions of that ordering.  A live candidate sits at position
r < K of the list exactly when its rank is r.

Memory.  ItemKNN holds C: m^2 * 4 bytes (192 MB at 6,932 items); the scores are formed in blocks of queries sized so that
[block][m] fp32 stays within SCORE_BLOCK_BYTES.  The block count leaves no trace in any output byte.
"""
import os

import numpy as np

from . import list_metrics
from . import recommend as rec

MAX_K = 128                         # MAMDR_SCORES_MAX_K
MAX_ITEMS = 65535                   # the largest m mamdr_item_cooc takes
DEFAULT_SHRINK = 10.0               # run.py --baselines without a number
DEFAULT_MAX_ITEMS = 16384           # train.baselines_max_items: C of 1 GiB
DEFAULT_K = 10                      # the ItemKNN lists saved when --recommend is not given
MAX_SHRINK = 2.0 ** 20
SCORE_BLOCK_BYTES = 64 << 20        # of fp32 scores per block of queries
WHICH = ("pop", "itemknn")


def check_shrink(shrink):
    shrink = float(shrink)
    if not 0.0 <= shrink <= MAX_SHRINK:          # (NaN fails both comparisons)
        raise ValueError("baselines: shrink %r outside [0, 2^20]" % (shrink,))
    return shrink


def error_bound(n_history):
    """|fp32 score - float64 score| <= (L + 8) * 2^-24 * float64 score for a history of L entries."""
    return (int(n_history) + 8) * 2.0 ** -24


# ------------------------------------------------------------------ histories
def check_csr(off, pos, m):
    """a histories CSR as the device calls want it: off int64 [n_user + 1] ascending from 0 to len(pos), pos inside [0, m),
    ascending and distinct within a user -> (off int64, pos int32)."""
    off, pos = np.ascontiguousarray(off, np.int64).ravel(), np.ascontiguousarray(pos, np.int64).ravel()
    if off.size < 1 or off[0] != 0 or off[-1] != pos.size or (np.diff(off) < 0).any():
        raise ValueError("baselines: history offsets must ascend from 0 to len(pos) = %d" % pos.size)
    if pos.size and (pos.min() < 0 or pos.max() >= int(m)):
        raise ValueError("baselines: a history position outside [0, %d)" % int(m))
    if pos.size > 1:
        inner = np.ones(pos.size - 1, bool)
        inner[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < pos.size)] - 1] = False        # (pairs that straddle two users)
        if (np.diff(pos)[inner] <= 0).any():
            raise ValueError("baselines: history positions must be ascending and distinct within a user")
    return off, pos.astype(np.int32)


def histories(dataset, domain, catalogue):
    """the label-1 rows of `domain`'s train split over `catalogue` (ascending distinct item ids) -> {"users": sorted distinct
    uids that have one, "off" int64 [n_user + 1], "pos" int32 [nnz]: the CSR of their distinct catalogue positions, ascending
    per user, "popularity" int64 [m]: label-1 rows per position}.  A pid outside the catalogue is dropped; a domain without
    a train split has nobody."""
    cat = np.asarray(catalogue, np.int64).ravel()
    m = int(cat.size)
    if m > 1 and (np.diff(cat) <= 0).any():
        raise ValueError("baselines: the catalogue must be ascending and distinct")
    uid = pid = np.zeros(0, np.int64)
    if domain in dataset.train_dataset:
        c = dataset.train_dataset[domain]["data"]
        keep = np.asarray(c["label"]) > 0
        uid, pid = np.asarray(c["uid"], np.int64)[keep], np.asarray(c["pid"], np.int64)[keep]
    if m and pid.size:
        at = np.minimum(np.searchsorted(cat, pid), m - 1)
        hit = cat[at] == pid
        uid, at = uid[hit], at[hit]
    else:
        uid, at = np.zeros(0, np.int64), np.zeros(0, np.int64)
    popularity = np.bincount(at, minlength=m).astype(np.int64)[:m] if m else np.zeros(0, np.int64)
    users, row = np.unique(uid, return_inverse=True)
    pairs = np.unique(row.astype(np.int64) * max(m, 1) + at)           # ascending: by user, then by position
    off = np.zeros(users.size + 1, np.int64)
    np.cumsum(np.bincount(pairs // max(m, 1), minlength=users.size), out=off[1:])
    return {"users": users, "off": off, "pos": (pairs % max(m, 1)).astype(np.int32), "popularity": popularity}


def pair_counts(off):
    """the sparse co-occurrence count's adds: the sum over users of L_u^2."""
    n = np.diff(np.asarray(off, np.int64))
    return int((n * n).sum())


# ------------------------------------------------------------------ host definitions of the device calls
def _ranges(off, nnz):
    """every user's [lo, hi) inside [0, nnz], an end below its start an empty range: what the kernels read."""
    off = np.asarray(off, np.int64).ravel()
    lo = np.clip(off[:-1], 0, nnz)
    return lo, np.maximum(lo, np.minimum(off[1:], nnz))


def cooc_host(off, pos, m):
    """mamdr_item_cooc on the host -> uint32 [m, m]: C[a][b] = the users whose history holds both a and b (every ORDERED
    pair of a history's entries adds one: with distinct positions that is the definition; the diagonal is the item's user
    count).  A position outside [0, m) counts nowhere."""
    m = int(m)
    pos = np.asarray(pos, np.int64).ravel()
    C = np.zeros((m, m), np.int64)
    for lo, hi in zip(*_ranges(off, pos.size)):
        h = pos[lo:hi]
        h = h[(h >= 0) & (h < m)]
        if h.size and np.unique(h).size == h.size:
            C[np.ix_(h, h)] += 1
        elif h.size:                                     # (a broken history: every ordered pair of ENTRIES, as the kernel adds)
            np.add.at(C, (h[:, None], h[None, :]), 1)
    return C.astype(np.uint32)


def history_scores_host(cooc, off, pos, queries, shrink, dtype=np.float32):
    """mamdr_history_scores on the host -> dtype [Q, m].  dtype=np.float32 is the device's arithmetic replayed operation by
    operation (numpy rounds every fp32 operation on its own; its square root and division are IEEE); dtype=np.float64 the
    same formula in float64.  Row j of C is what entry j brings (C is symmetric)."""
    C = np.asarray(cooc)
    m = int(C.shape[0])
    pos = np.asarray(pos, np.int64).ravel()
    lo_all, hi_all = _ranges(off, pos.size)
    q = np.asarray(queries, np.int64).ravel()
    shrink = dtype(check_shrink(shrink))
    root = np.sqrt(np.diagonal(C).astype(dtype))
    cols = np.arange(m)
    out = np.zeros((q.size, m), dtype)
    for i, u in enumerate(q.tolist()):
        if not 0 <= u < lo_all.size:
            continue
        acc = np.zeros(m, dtype)
        for j in pos[lo_all[u]:hi_all[u]].tolist():
            if not 0 <= j < m:
                continue
            cnt = C[j]
            with np.errstate(divide="ignore", invalid="ignore"):
                sim = cnt.astype(dtype) / (root * root[j] + shrink)
            acc = acc + np.where((cnt > 0) & (cols != j), sim, dtype(0))
        out[i] = acc
    return out


def _score_problem(scores, n_query, cand, excl_off, excl_ids):
    s = np.asarray(scores, np.float32)
    n_query = int(n_query)
    if s.ndim == 1:
        s = np.broadcast_to(s, (n_query, s.shape[0]))
    if s.ndim != 2 or s.shape[0] != n_query:
        raise ValueError("baselines: scores must be [Q, n_cand] or [n_cand]")
    ids = np.arange(s.shape[1], dtype=np.int64) if cand is None else np.asarray(cand, np.int64).ravel()
    if ids.shape[0] != s.shape[1]:
        raise ValueError("baselines: %d candidate ids for %d score columns" % (ids.shape[0], s.shape[1]))
    canon = np.where(s == 0, np.float32(0), s)                           # -0 counts as +0; NaN stays
    keys = list_metrics.rank_keys(canon, np.broadcast_to(ids, s.shape))
    live = np.ones(s.shape, bool)
    if excl_off is not None:
        excl_off, excl_ids = np.asarray(excl_off, np.int64), np.asarray(excl_ids, np.int64)
        for qi in range(n_query):
            live[qi] = ~np.isin(ids, excl_ids[excl_off[qi]:excl_off[qi + 1]])
    return s, canon, ids, keys, live


def rank_scores_host(scores, n_query, tgt_off, tgt_ids, cand=None, excl_off=None, excl_ids=None):
    """mamdr_rank_scores on the host -> (ranks int32 [T], live int32 [Q], scores float32 [T]: the targets' raw scores, 0 for
    one that is no candidate)."""
    s, _, ids, keys, live = _score_problem(scores, n_query, cand, excl_off, excl_ids)
    tgt_off, tgt_ids = np.asarray(tgt_off, np.int64), np.asarray(tgt_ids, np.int64)
    ranks, out = np.zeros(tgt_ids.size, np.int32), np.zeros(tgt_ids.size, np.float32)
    for qi in range(int(n_query)):
        for t in range(int(tgt_off[qi]), int(tgt_off[qi + 1])):
            at = np.flatnonzero(ids == tgt_ids[t])
            if not at.size:
                ranks[t] = -1
                continue
            ranks[t] = int((keys[qi][live[qi]] > keys[qi][at[0]]).sum())
            out[t] = s[qi][at[0]]
    return ranks, live.sum(1).astype(np.int32), out


def topk_scores_host(scores, n_query, k, cand=None, excl_off=None, excl_ids=None):
    """mamdr_topk_scores on the host -> (ids int32 [Q, k], scores float32 [Q, k]): the first k live positions by key
    descending; -1 / 0 behind a short list; a NaN leaves as the quiet NaN, a -0.0 as +0.0."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("baselines: k %d outside 1..%d" % (k, MAX_K))
    _, canon, ids, keys, live = _score_problem(scores, n_query, cand, excl_off, excl_ids)
    shown = np.where(np.isnan(canon), np.float32(np.nan), canon)
    ids_out, out = np.full((int(n_query), k), -1, np.int32), np.zeros((int(n_query), k), np.float32)
    for qi in range(int(n_query)):
        at = np.flatnonzero(live[qi])
        order = at[np.argsort(keys[qi][at], kind="stable")[::-1]][:k]
        ids_out[qi, :order.size] = ids[order]
        out[qi, :order.size] = shown[qi][order]
    return ids_out, out


# ------------------------------------------------------------------ one domain under the rank-eval protocol
def block_queries(m, n_query):
    """queries per block of ItemKNN scores: [block][m] fp32 within SCORE_BLOCK_BYTES, at least one."""
    return max(1, min(int(n_query), SCORE_BLOCK_BYTES // (4 * max(1, int(m)))))


def _csr_block(off, ids, b0, b1):
    """queries [b0, b1) of a CSR as a CSR of their own (a one-element ids array under an empty one: a non-null pointer)."""
    part = ids[off[b0]:off[b1]]
    return (off[b0:b1 + 1] - off[b0]).astype(np.int64), part if part.size else np.zeros(1, np.int32)


def rank(model, domain, which, shrink=DEFAULT_SHRINK, k=None, block=None):
    """`BaseModel.rank_eval`'s problem for `domain` -- its catalogue, the test split's users, their train / val items
    excluded, their label-1 test items as targets -- ranked by a baseline instead of the tower: which = "pop" (MostPopular:
    the train split's label-1 counts from mamdr_id_counts, one fp32 row for every user) or "itemknn" (mamdr_item_cooc over
    `histories`, mamdr_history_scores in blocks of `block` queries, default block_queries(m, Q)), through
    mamdr_rank_scores.  -> the keys of the engine's rank_domain ("offsets", "ids", "ranks", "listed", "live") plus "users",
    "catalogue", "n_positives" and "n_cold" (the users without a train history in the domain); with k also "top_ids" /
    "top_scores" [Q, k] (mamdr_topk_scores).  No output byte depends on `block`."""
    import torch
    if which not in WHICH:
        raise ValueError("baselines: which %r is neither 'pop' nor 'itemknn'" % (which,))
    shrink = check_shrink(shrink)
    eng = model.model
    catalogue, users, exclude = model._retrieval_problem(domain, None, True)
    nq, m = int(users.size), int(catalogue.size)
    if m > np.iinfo(np.int32).max or (catalogue.size and (catalogue.min() < 0 or catalogue.max() > np.iinfo(np.int32).max)):
        raise ValueError("baselines: catalogue ids must fit int32")
    e_off, e_ids = rec.exclusion_csr(exclude, nq)
    t_off, t_ids = rec.exclusion_csr(rec.split_positives(model.dataset, domain, users), nq, "targets")
    listed = np.isin(t_ids, catalogue)
    for q in range(nq):
        sl = slice(t_off[q], t_off[q + 1])
        listed[sl] &= ~np.isin(t_ids[sl], e_ids[e_off[q]:e_off[q + 1]])
    h = histories(model.dataset, domain, catalogue)
    at = np.minimum(np.searchsorted(h["users"], users), max(h["users"].size - 1, 0))
    known = h["users"][at] == users if h["users"].size else np.zeros(nq, bool)
    res = {"offsets": t_off, "ids": t_ids, "listed": listed, "users": users, "catalogue": catalogue,
           "n_positives": np.diff(t_off).astype(np.int64), "n_cold": int((~known).sum())}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)      # noqa: E731
    ranks, live = np.zeros(t_ids.size, np.int32), np.zeros(nq, np.int32)
    top_ids = np.full((nq, int(k or 1)), -1, np.int32)
    top_scores = np.zeros((nq, int(k or 1)), np.float32)
    if nq and m:
        d_cand = dev(catalogue.astype(np.int32))
        if which == "pop":
            row = torch.zeros(m, dtype=torch.float32, device=eng.device)
            if domain in model.dataset.train_dataset:
                cols = eng.data[(domain, "train")]
                row = eng.id_counts(cols["pid"], int(eng.n_item), cols["label"])[d_cand.long()].to(torch.float32).contiguous()
            blocks, step = [(0, nq)], nq
        else:
            if m > MAX_ITEMS:
                raise ValueError("baselines: ItemKNN over %d items (at most %d)" % (m, MAX_ITEMS))
            off, pos = check_csr(h["off"], h["pos"], m)
            n_user = off.size - 1
            if n_user < 1:                                              # nobody has a history: one empty user
                off, n_user = np.zeros(2, np.int64), 1
            d_off, d_pos = dev(off), dev(pos if pos.size else np.zeros(1, np.int32))[:pos.size]
            cooc = eng.item_cooc(d_off, d_pos, m)
            query = np.where(known, at, -1).astype(np.int32)
            step = block_queries(m, nq) if block is None else max(1, int(block))
            blocks = [(b0, min(nq, b0 + step)) for b0 in range(0, nq, step)]
        for b0, b1 in blocks:
            scores = row if which == "pop" else eng.history_scores(cooc, d_off, d_pos, dev(query[b0:b1]), shrink)
            bt_off, bt_ids = _csr_block(t_off, t_ids, b0, b1)
            be_off, be_ids = _csr_block(e_off, e_ids, b0, b1)
            d_eoff, d_eids = dev(be_off), dev(be_ids)
            n_t = int(t_off[b1] - t_off[b0])
            r, lv = eng.rank_scores(scores, b1 - b0, dev(bt_off), dev(bt_ids)[:n_t], candidates=d_cand, excl_off=d_eoff,
                                    excl_ids=d_eids)
            ranks[t_off[b0]:t_off[b1]], live[b0:b1] = list_metrics.to_host(r), list_metrics.to_host(lv)
            if k:
                ti, ts = eng.topk_scores(scores, b1 - b0, int(k), candidates=d_cand, excl_off=d_eoff, excl_ids=d_eids)
                top_ids[b0:b1], top_scores[b0:b1] = list_metrics.to_host(ti), list_metrics.to_host(ts)
    elif t_ids.size:
        ranks[:] = -1
    res.update(ranks=ranks, live=live)
    if k:
        res.update(top_ids=top_ids, top_scores=top_scores)
    return res


def rank_host(model, domain, which, shrink=DEFAULT_SHRINK, k=None):
    """`rank` by the host definitions alone (numpy; no engine call): what the device route is held to."""
    shrink = check_shrink(shrink)
    catalogue, users, exclude = model._retrieval_problem(domain, None, True)
    nq, m = int(users.size), int(catalogue.size)
    e_off, e_ids = rec.exclusion_csr(exclude, nq)
    t_off, t_ids = rec.exclusion_csr(rec.split_positives(model.dataset, domain, users), nq, "targets")
    h = histories(model.dataset, domain, catalogue)
    if which == "pop":
        scores = h["popularity"].astype(np.float32)
    else:
        at = np.minimum(np.searchsorted(h["users"], users), max(h["users"].size - 1, 0))
        known = h["users"][at] == users if h["users"].size else np.zeros(nq, bool)
        scores = history_scores_host(cooc_host(h["off"], h["pos"], m), h["off"], h["pos"], np.where(known, at, -1), shrink)
    ranks, live, _ = rank_scores_host(scores, nq, t_off, t_ids, catalogue, e_off, e_ids)
    res = {"offsets": t_off, "ids": t_ids, "ranks": ranks, "live": live}
    if k:
        res["top_ids"], res["top_scores"] = topk_scores_host(scores, nq, k, catalogue, e_off, e_ids)
    return res


# ------------------------------------------------------------------ run.py --rank-eval [KS] --baselines [SHRINK]
def jaccard(a, b):
    """the mean over the rows of |A n B| / |A u B| of two id lists [Q, K] (-1: padding), over the rows whose union is not
    empty; 0.0 without one."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("baselines: two [Q, K] id lists of the same users")
    total, n = 0.0, 0
    for x, y in zip(a, b):
        x, y = np.unique(x[x >= 0]), np.unique(y[y >= 0])
        union = np.union1d(x, y).size
        if union:
            total += np.intersect1d(x, y).size / float(union)
            n += 1
    return total / n if n else 0.0


def figures(ks):
    """the names of a metrics dict's scalars, in the order they are printed and saved."""
    return ["mrr", "mean_percentile"] + ["%s_at_%d" % (name, int(k)) for k in ks for name in ("hit_rate", "recall", "ndcg")]


def _flat(m):
    """recommend.rank_metrics' dict -> {figure: value}."""
    out = {"mrr": float(m["mrr"]), "mean_percentile": float(m["mean_percentile"])}
    for i, k in enumerate(m["ks"]):
        for name in ("hit_rate", "recall", "ndcg"):
            out["%s_at_%d" % (name, int(k))] = float(m[name][i])
    return out


def _line(d, who, m, ks, tail=""):
    return "{}: {:<8} MRR {:.4f} MeanPercentile {:.4f} {}{}".format(
        d, who, m["mrr"], m["mean_percentile"],
        " ".join("HitRate@{k} {:.4f} Recall@{k} {:.4f} NDCG@{k} {:.4f}".format(
            m["hit_rate_at_%d" % k], m["recall_at_%d" % k], m["ndcg_at_%d" % k], k=k) for k in ks), tail)


def report(model, ks, k_lists=None, out_path=None, shrink=DEFAULT_SHRINK, max_items=DEFAULT_MAX_ITEMS, tower=None):
    """`run.py --rank-eval KS --baselines [SHRINK]`: for every domain MRR, mean percentile and HitRate / Recall / NDCG at
    every K of `ks` (recommend.rank_metrics) of MostPopular and ItemKNN beside the tower's own -- `tower`: rank_report's
    {domain: metrics}, computed here (model.rank_eval) when not given --; with k_lists (run.py --recommend K) also the mean
    per-user Jaccard overlap of the tower's top-K with each baseline's.  A domain whose catalogue exceeds `max_items` gets
    MostPopular only and is named.  Written to ONE .npz -- domains, ks, shrink, k_lists, m / n_cold / skipped [n domains],
    per domain d users_d, offsets_d, ids_d, listed_d, live_d, ranks_pop_d, ranks_itemknn_d, itemknn_ids_d /
    itemknn_scores_d [Q, K]; one [n domains] array per figure and baseline (<figure>_pop, <figure>_itemknn; NaN where
    skipped), overlap_pop / overlap_itemknn -- and printed.  -> (path, {domain: report})."""
    ks = [int(k) for k in ks]
    shrink, max_items = check_shrink(shrink), int(max_items)
    k_top = int(k_lists) if k_lists else DEFAULT_K
    if not 1 <= k_top <= MAX_K:
        raise ValueError("baselines: lists of %d items (1..%d)" % (k_top, MAX_K))
    domains = sorted(model.dataset.test_dataset)
    names = figures(ks)
    arrays = {"domains": np.asarray(domains, np.int64), "ks": np.asarray(ks, np.int64), "shrink": np.asarray(shrink, np.float64),
              "k_lists": np.asarray(k_top, np.int64)}
    reports = {}
    print("Baselines under the rank-eval protocol (MostPopular; ItemKNN, shrink {:g}): ".format(shrink))
    for d in domains:
        if tower is not None and d in tower:
            tm = _flat(tower[d])
        else:
            r = model.rank_eval(d)
            tm = _flat(rec.rank_metrics(r["offsets"], r["ranks"], r["listed"], r["live"], r["n_positives"], ks))
        pop = rank(model, d, "pop", shrink, k=k_top)
        m = int(pop["catalogue"].shape[0])
        skipped = m > max_items
        knn = None if skipped else rank(model, d, "itemknn", shrink, k=k_top)
        rep = reports[d] = {"m": m, "n_cold": pop["n_cold"], "skipped": skipped, "tower": tm, "itemknn": None,
                            "overlap_pop": None, "overlap_itemknn": None}
        rep["pop"] = _flat(rec.rank_metrics(pop["offsets"], pop["ranks"], pop["listed"], pop["live"], pop["n_positives"], ks))
        if knn is not None:
            rep["itemknn"] = _flat(rec.rank_metrics(knn["offsets"], knn["ranks"], knn["listed"], knn["live"],
                                                    knn["n_positives"], ks))
        for name in ("users", "offsets", "ids", "listed", "live"):
            arrays["%s_%d" % (name, d)] = pop[name]
        arrays["ranks_pop_%d" % d] = pop["ranks"]
        arrays["ranks_itemknn_%d" % d] = knn["ranks"] if knn is not None else np.zeros(0, np.int32)
        arrays["itemknn_ids_%d" % d] = knn["top_ids"] if knn is not None else np.zeros((0, k_top), np.int32)
        arrays["itemknn_scores_%d" % d] = knn["top_scores"] if knn is not None else np.zeros((0, k_top), np.float32)
        print(_line(d, "tower", tm, ks, " ({} users, {} items)".format(pop["users"].size, m)))
        print(_line(d, "pop", rep["pop"], ks))
        if knn is not None:
            print(_line(d, "itemknn", rep["itemknn"], ks, " ({} cold users: no train history, ranked by the tie rule)".format(
                pop["n_cold"])))
        else:
            print("{}: itemknn  skipped: {} items exceed train.baselines_max_items = {} (the co-occurrence matrix would take "
                  "{:.2f} GiB); MostPopular only".format(d, m, max_items, 4.0 * m * m / 2.0 ** 30))
        if k_lists:
            mine = np.asarray(model.recommend(d, k_top)["ids"])
            rep["overlap_pop"] = jaccard(mine, pop["top_ids"])
            if knn is not None:
                rep["overlap_itemknn"] = jaccard(mine, knn["top_ids"])
            print("{}: overlap  Jaccard@{} of the tower's lists with MostPopular {:.4f}{}".format(
                d, k_top, rep["overlap_pop"],
                " with ItemKNN {:.4f}".format(rep["overlap_itemknn"]) if knn is not None else ""))
    nan = float("nan")
    for who in WHICH:
        for name in names:
            arrays["%s_%s" % (name, who)] = np.asarray([reports[d][who][name] if reports[d][who] is not None else nan
                                                        for d in domains], np.float64)
        arrays["overlap_" + who] = np.asarray([nan if reports[d]["overlap_" + who] is None else reports[d]["overlap_" + who]
                                               for d in domains], np.float64)
    arrays["m"] = np.asarray([reports[d]["m"] for d in domains], np.int64)
    arrays["n_cold"] = np.asarray([reports[d]["n_cold"] for d in domains], np.int64)
    arrays["skipped"] = np.asarray([reports[d]["skipped"] for d in domains], bool)
    if out_path is None:
        out_path = os.path.join(model.result_path, "baselines.npz")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Baselines written to {}".format(out_path))
    return out_path, reports


def headline(reports, shrink=DEFAULT_SHRINK):
    """what result.json gains: baselines_shrink; domain_<figure>_pop / domain_<figure>_itemknn = {domain: value} and their
    plain means over the domains that have the baseline avg_<figure>_pop / avg_<figure>_itemknn (no keys without one);
    domain_overlap_pop / domain_overlap_itemknn (when the overlap was measured); domain_cold_users; baselines_skipped: the
    domains whose catalogue exceeded train.baselines_max_items (MostPopular only)."""
    out = {"baselines_shrink": float(shrink)}
    for who in WHICH:
        have = {d: r[who] for d, r in reports.items() if r.get(who) is not None}
        for name in (next(iter(have.values())) if have else {}):
            out["domain_%s_%s" % (name, who)] = {str(d): m[name] for d, m in have.items()}
            out["avg_%s_%s" % (name, who)] = float(np.mean([m[name] for m in have.values()]))
        over = {str(d): r["overlap_" + who] for d, r in reports.items() if r.get("overlap_" + who) is not None}
        if over:
            out["domain_overlap_" + who] = over
    out["domain_cold_users"] = {str(d): int(r["n_cold"]) for d, r in reports.items()}
    out["baselines_skipped"] = [int(d) for d, r in reports.items() if r["skipped"]]
    return out
