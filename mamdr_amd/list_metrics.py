"""Beyond-accuracy report of top-K lists, host side: what the lists are MADE OF -- how much of a domain's catalogue is ever
shown (coverage), how concentrated exposure is (Gini, entropy), how far the lists lean on popular items (novelty, average
popularity, tail share), how different two users' lists are (personalisation) and how similar the K items inside one list
are to each other (intra-list diversity).  The documented host definitions of `mamdr_id_counts` and `mamdr_list_similarity`
(include/mamdr_hip.h), the figures of one domain (`summarise`), the per-domain report behind `run.py --list-metrics [K]` and
its result.json keys.  Pure numpy except for the engine calls.  The reference has no counterpart: it never builds a list.

The device counts and contracts, the host defines.  Per domain the device gives four things (BaseModel.list_eval):

- `exposure` [n_item]: how often each item occurs in the lists (`mamdr_id_counts` over the flattened [Q][K] ids; the -1
  padding of a short list counts nowhere);
- `popularity` [n_item]: each item's label-1 rows in the domain's train split (`mamdr_id_counts` over its pid and label
  columns);
- `sim_sum` [Q], `pairs` [Q]: per list the sum of the cosines between its valid entries' item-embedding rows and the number
  of such pairs (`mamdr_list_similarity` on the item table of the weights that produced the lists).

Figures (`summarise`), float64.  c and p are exposure and popularity restricted to the domain's catalogue of n items,
C = sum c_i, P = sum p_i, Q' the number of non-empty lists:

- coverage        #{c_i > 0} / n
- gini            Gini coefficient of c over the catalogue from the ascending order c_(1) <= ... <= c_(n):
                  sum_j (2 j - n - 1) c_(j) / (n C); 0 when C = 0
- entropy         Shannon entropy in bits of c / C; 0 when C = 0
- novelty         sum c_i * (-log2((p_i + 1) / (P + n))) / C: the mean self-information of a shown item under the add-one
                  smoothed train popularity (a never-clicked item stays finite); 0 when C = 0
- avg_popularity  sum c_i p_i / C; 0 when C = 0
- tail_share      the share of C that falls on tail items.  The head is the shortest prefix of the items, ordered by
                  descending p_i and then ascending id, whose popularity sum reaches 0.8 P, in integers: 5 * sum_head >= 4 P
                  (P = 0: the empty prefix, every item is tail).  0 when C = 0
- personalisation 1 - [sum_i c_i (c_i - 1) / 2] / [Q' (Q' - 1) / 2 * k]: for lists of distinct ids the numerator counts, over
                  all pairs of lists, the items they share, so this is one minus the mean overlap of two users' lists --
                  exact from integers, no pairwise pass over users.  0 when Q' < 2
- ild, n_ild      the mean of 1 - sim_sum / pairs over the lists with pairs > 0, and how many lists that is; 0 without one

Diversified re-ranking (`run.py --diversify [LAMBDA]`).  `mamdr_list_diversify` picks K of every user's top-N pool by greedy
Maximal Marginal Relevance (Carbonell & Goldstein 1998): the next pick maximises lambda * relevance - (1 - lambda) * (the
largest cosine with a pick so far).  `diversify_host` is its float64 definition, `diversify_replay` the same loop in
separately rounded fp32 on cosines the caller supplies (the device's own: then the outputs agree to the bit),
`minmax_relevance` the relevance `BaseModel.diversify` feeds it by default, `diversify_report` / `diversify_headline` the
report of both sides -- the base top-K and the re-ranked lists -- and its result.json keys.

Determinism.  The counts are integers.  `mamdr_list_similarity` fixes every order from the list's own valid entries: a
list's (sim_sum, pairs) are the same bits from run to run and wherever the list sits.  Everything else is numpy on the host.
"""
import os

import numpy as np

MAX_K = 128                         # MAMDR_LIST_MAX_K: the longest list mamdr_list_similarity takes
EMB_DIMS = (32, 64, 128, 256)       # the table widths it takes
DEFAULT_K = 10                      # run.py --list-metrics without a number and without --recommend
FIGURES = ("coverage", "gini", "entropy", "novelty", "avg_popularity", "tail_share", "personalisation", "ild")
AVERAGED = ("coverage", "gini", "novelty", "personalisation", "ild")      # headline's avg_<figure>
DEFAULT_LAMBDA = 0.7                # run.py --diversify without a number
ACCURACY = ("hit_rate", "recall", "ndcg")       # recommend.ranking_metrics' figures, reported beside FIGURES by diversify_report


def to_host(x):
    """device tensor or array -> numpy."""
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def check_k(k, what="list metrics"):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("%s: k %d outside 1..%d" % (what, k, MAX_K))
    return k


def error_bound(emb_dim):
    """per pair: |device cosine - fp64 cosine of the same fp32 rows| <= (2 E + 8) * 2^-24 -- with u = 2^-24 the fp32 fma
    chain of E terms is within E u |a| |b| of the dot product, each norm within (E / 2 + 1) u relative (the chain of its
    square, halved by the IEEE square root, plus the root's rounding), the two IEEE divisions one u each: 2 E + 4, rounded
    up to 2 E + 8.  The fp64 additions add nothing visible."""
    return (2 * int(emb_dim) + 8) * 2.0 ** -24


# ------------------------------------------------------------------ host definitions of the two device calls
def id_counts_host(ids, n_bins, label=None):
    """mamdr_id_counts on the host -> int64 [n_bins]: counts[i] = #{j : ids[j] == i}, with a label column only the
    positions with label[j] != 0 (fp32: -0.0 is 0, NaN is not).  An id outside [0, n_bins) counts nowhere."""
    ids = np.asarray(ids).ravel().astype(np.int64)
    n_bins = int(n_bins)
    if n_bins <= 0:
        raise ValueError("id counts: n_bins %d is not positive" % n_bins)
    keep = (ids >= 0) & (ids < n_bins)
    if label is not None:
        label = np.asarray(label, np.float32).ravel()
        if label.shape != ids.shape:
            raise ValueError("id counts: ids and label differ in length")
        keep &= label != 0
    return np.bincount(ids[keep], minlength=n_bins).astype(np.int64)


def list_similarity_host(ids, rows):
    """mamdr_list_similarity on the host, in float64 on the given fp32 rows -> (sim_sum float64 [Q], pairs int32 [Q]).
    ids [Q, K]; an entry is valid when its id lies inside [0, n_rows), every other id is padding wherever it sits.  With L
    valid entries pairs = L (L - 1) / 2 and sim_sum = sum over the valid entries a < b of cos(x_a, x_b) =
    (x_a . x_b) / (|x_a| |x_b|), exactly 0 when either norm is 0."""
    ids = np.asarray(ids)
    rows = np.asarray(rows, np.float32)
    if ids.ndim != 2 or rows.ndim != 2:
        raise ValueError("list similarity: ids must be [Q, K], rows [n_rows, emb_dim]")
    n_rows = rows.shape[0]
    sim_sum = np.zeros(ids.shape[0], np.float64)
    pairs = np.zeros(ids.shape[0], np.int32)
    for q, row in enumerate(ids.astype(np.int64)):
        x = rows[row[(row >= 0) & (row < n_rows)]].astype(np.float64)
        L = x.shape[0]
        pairs[q] = L * (L - 1) // 2
        if L < 2:
            continue
        norm = np.sqrt((x * x).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = (x @ x.T) / (norm[:, None] * norm[None, :])
        cos[(norm == 0)[:, None] | (norm == 0)[None, :]] = 0.0
        sim_sum[q] = cos[np.triu_indices(L, k=1)].sum()
    return sim_sum, pairs


# ------------------------------------------------------------------ greedy MMR: the host definitions of mamdr_list_diversify
def diversify_tol(emb_dim, lam):
    """how far, in float64 value, a device pick may stand below its step's best, for rel in [0, 1]:
    ((1 - lambda) (2 E + 8) + 8) * 2^-24 -- the cosine's error_bound(E) scaled by its weight, plus 8 units for the rounding of
    1 - lambda, of the two products, of the difference and of a |cos| slightly above 1.  Two entries can each be off by it:
    a device pick is within 2 tol of the float64 best."""
    return ((1.0 - float(lam)) * (2 * int(emb_dim) + 8) + 8.0) * 2.0 ** -24


def _valid_entries(row, n_rows):
    return np.flatnonzero((row >= 0) & (row < n_rows))


def _check_diversify(ids, rel, k, lam):
    ids, rel = np.asarray(ids), np.asarray(rel, np.float32)
    if ids.ndim != 2 or rel.shape != ids.shape:
        raise ValueError("diversify: ids and rel must both be [Q, n]")
    n, k = ids.shape[1], int(k)
    if not 1 <= n <= MAX_K or not 1 <= k <= n:
        raise ValueError("diversify: n %d outside 1..%d or k %d outside 1..n" % (n, MAX_K, k))
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError("diversify: lambda %r outside [0, 1]" % (lam,))
    return ids.astype(np.int64), rel, k


def rank_keys(values, ids):
    """the retrieval family's 64-bit ranking key of fp32 values and int32 ids (csrc/rec_device.h: rec_key), uint64: a larger
    key ranks first -- fp32 values by their bits (so -0.0 behind +0.0), NaN behind every number, equal values by ascending
    id."""
    b = np.asarray(values, np.float32).view(np.uint32).astype(np.uint64)
    hi = np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    hi = np.where(np.isnan(np.asarray(values, np.float32)), np.uint64(1), hi)
    lo = ~np.asarray(ids, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return (hi << np.uint64(32)) | lo


def diversify_host(ids, rel, rows, k, lam):
    """mamdr_list_diversify on the host, in float64 on the given fp32 inputs (lambda as its fp32 value) -> (positions int32
    [Q, k], values float64 [Q, k]).  Per list the valid entries (0 <= id < n_rows), in list order, are e_0 .. e_{L-1};
    cos = (x_a . x_b) / (|x_a| |x_b|), exactly 0 when either norm is 0.  Step 0 picks the largest rel; step t >= 1 the
    largest lambda * rel_c - (1 - lambda) * m_c among the entries not yet picked, m_c = the running maximum (the first
    pick's cosine, then `cos > m ? cos : m`) of c's cosines with the picks so far.  Equal values go by ascending id, NaN
    behind every number.  min(k, L) picks; positions are those of the input list, -1 (value 0) behind a short list."""
    ids, rel, k = _check_diversify(ids, rel, k, lam)
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2:
        raise ValueError("diversify: rows must be [n_rows, emb_dim]")
    lam = float(np.float32(lam))
    oml = 1.0 - lam
    pos_out = np.full((ids.shape[0], k), -1, np.int32)
    val_out = np.zeros((ids.shape[0], k), np.float64)
    for q, row in enumerate(ids):
        at = _valid_entries(row, rows.shape[0])
        L = at.shape[0]
        if L == 0:
            continue
        x = rows[row[at]].astype(np.float64)
        norm = np.sqrt((x * x).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = (x @ x.T) / (norm[:, None] * norm[None, :])
        cos[(norm == 0)[:, None] | (norm == 0)[None, :]] = 0.0
        r, item = rel[q, at].astype(np.float64), row[at]
        picked = np.zeros(L, bool)
        m = np.zeros(L, np.float64)
        for t in range(min(k, L)):
            with np.errstate(invalid="ignore"):
                v = r if t == 0 else lam * r - oml * m
            nan = np.isnan(v)
            free = np.flatnonzero(~picked)
            # NaN last, then descending value, then ascending id
            best = free[np.lexsort((item[free], -np.where(nan[free], 0.0, v[free]), nan[free]))[0]]
            picked[best] = True
            pos_out[q, t], val_out[q, t] = at[best], v[best]
            c = cos[best]
            with np.errstate(invalid="ignore"):
                m = c.copy() if t == 0 else np.where(c > m, c, m)
    return pos_out, val_out


def diversify_audit(ids, rel, rows, pos, lam):
    """given picks `pos` [Q, k] (positions, -1 = none) for the problem of diversify_host, what the float64 definition says of
    every step, taking the EARLIER picks as given -> (shortfall, margin) float64 [Q, k]: shortfall = the largest float64
    value among the entries still free at that step minus the pick's own (0: the pick is a best one); margin = the largest
    minus the second largest (inf with one entry left): how far the step is from a tie.  Steps without a pick give 0 / inf.
    NaN values count as -inf."""
    ids, rel = np.asarray(ids).astype(np.int64), np.asarray(rel, np.float32)
    rows, pos = np.asarray(rows, np.float32), np.asarray(pos)
    lam = float(np.float32(lam))
    oml = 1.0 - lam
    shortfall = np.zeros(pos.shape, np.float64)
    margin = np.full(pos.shape, np.inf, np.float64)
    for q, row in enumerate(ids):
        at = _valid_entries(row, rows.shape[0])
        L = at.shape[0]
        if L == 0:
            continue
        where = {int(p): c for c, p in enumerate(at)}
        x = rows[row[at]].astype(np.float64)
        norm = np.sqrt((x * x).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = (x @ x.T) / (norm[:, None] * norm[None, :])
        cos[(norm == 0)[:, None] | (norm == 0)[None, :]] = 0.0
        r = rel[q, at].astype(np.float64)
        picked = np.zeros(L, bool)
        m = np.zeros(L, np.float64)
        for t in range(pos.shape[1]):
            if pos[q, t] < 0:
                break
            c = where[int(pos[q, t])]
            if picked[c]:
                raise ValueError("diversify audit: list %d picks position %d twice" % (q, pos[q, t]))
            with np.errstate(invalid="ignore"):
                v = r if t == 0 else lam * r - oml * m
            v = np.where(np.isnan(v), -np.inf, v)
            free = np.sort(v[~picked])[::-1]
            with np.errstate(invalid="ignore"):
                shortfall[q, t] = 0.0 if v[c] == free[0] else free[0] - v[c]
                margin[q, t] = free[0] - free[1] if free.size > 1 and free[0] != free[1] else (0.0 if free.size > 1 else np.inf)
            picked[c] = True
            with np.errstate(invalid="ignore"):
                m = cos[c].copy() if t == 0 else np.where(cos[c] > m, cos[c], m)
    return shortfall, margin


def diversify_replay(ids, rel, pair_cos, k, lam, n_rows=None):
    """mamdr_list_diversify's loop in numpy float32 -- 1 - lambda, the two products and the difference each rounded on their
    own, the pick by rank_keys -- on cosines supplied by the caller: pair_cos[q] is an [L_q, L_q] fp32 array over list q's
    valid entries in list order (0 <= id < n_rows; without n_rows every id >= 0), of which only [a, b] with a < b is read.
    Fed the device's own cosines it gives the device's bytes.  -> (positions int32 [Q, k], values float32 [Q, k])."""
    ids, rel, k = _check_diversify(ids, rel, k, lam)
    lam = np.float32(lam)
    oml = np.float32(1.0) - lam
    pos_out = np.full((ids.shape[0], k), -1, np.int32)
    val_out = np.zeros((ids.shape[0], k), np.float32)
    for q, row in enumerate(ids):
        at = np.flatnonzero(row >= 0) if n_rows is None else _valid_entries(row, int(n_rows))
        L = at.shape[0]
        if L == 0:
            continue
        pc = np.asarray(pair_cos[q], np.float32)
        if pc.shape != (L, L):
            raise ValueError("diversify replay: list %d has %d entries, its cosines are %r" % (q, L, pc.shape))
        cos = np.triu(pc, 1)
        cos = cos + cos.T
        r, item = rel[q, at], row[at]
        picked = np.zeros(L, bool)
        m = np.zeros(L, np.float32)
        for t in range(min(k, L)):
            with np.errstate(invalid="ignore", over="ignore"):
                v = r if t == 0 else (lam * r).astype(np.float32) - (oml * m).astype(np.float32)
            keys = rank_keys(v, item)
            keys[picked] = 0
            best = int(np.argmax(keys))
            picked[best] = True
            pos_out[q, t], val_out[q, t] = at[best], v[best]
            c = cos[best]
            with np.errstate(invalid="ignore"):
                m = c.copy() if t == 0 else np.where(c > m, c, m)
    return pos_out, val_out


def minmax_relevance(scores, ids, n_rows):
    """the relevance BaseModel.diversify feeds the re-ranking by default, fp32 [Q, n]: (s - lo) / (hi - lo) with lo / hi the
    smallest / largest score among the list's valid entries (0 <= id < n_rows), 0 when hi == lo and 0 on padding."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids)
    if scores.shape != ids.shape or ids.ndim != 2:
        raise ValueError("minmax relevance: scores and ids must both be [Q, n]")
    valid = (ids >= 0) & (ids < int(n_rows))
    lo = np.where(valid, scores, np.float32(np.inf)).min(axis=1, keepdims=True) if ids.shape[1] else scores
    hi = np.where(valid, scores, np.float32(-np.inf)).max(axis=1, keepdims=True) if ids.shape[1] else scores
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = ((scores - lo).astype(np.float32) / (hi - lo).astype(np.float32)).astype(np.float32)
    return np.where(valid & (hi > lo), rel, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------ the figures of one domain
def summarise(exposure, popularity, catalogue, k, sim_sum, pairs, n_lists=None):
    """the module docstring's figures of one domain, float64 -> {"coverage", "gini", "entropy", "novelty", "avg_popularity",
    "tail_share", "personalisation", "ild", "n_ild", "n_lists", "n_items", "n_shown"}.  exposure / popularity: integer
    vectors indexed by item id (at least max(catalogue) + 1 long); catalogue: the domain's distinct item ids; k: the lists'
    length; sim_sum / pairs: one entry per list.  n_lists = Q', the non-empty lists; by default ceil(C / k), which is Q'
    whenever at most one list is short."""
    cat = np.unique(np.asarray(catalogue, np.int64).ravel())
    n, k = int(cat.shape[0]), int(k)
    if n == 0 or k < 1:
        raise ValueError("list metrics: an empty catalogue or k < 1")
    exposure, popularity = np.asarray(exposure).ravel(), np.asarray(popularity).ravel()
    if cat[0] < 0 or cat[-1] >= min(exposure.shape[0], popularity.shape[0]):
        raise ValueError("list metrics: a catalogue id outside the exposure / popularity vectors")
    c, p = exposure[cat].astype(np.int64), popularity[cat].astype(np.int64)
    if (c < 0).any() or (p < 0).any():
        raise ValueError("list metrics: negative counts")
    C, P = int(c.sum()), int(p.sum())
    sim_sum, pairs = np.asarray(sim_sum, np.float64).ravel(), np.asarray(pairs, np.int64).ravel()
    if sim_sum.shape != pairs.shape:
        raise ValueError("list metrics: sim_sum and pairs differ in length")
    n_lists = -(-C // k) if n_lists is None else int(n_lists)
    out = {"coverage": float(np.count_nonzero(c)) / n, "gini": 0.0, "entropy": 0.0, "novelty": 0.0, "avg_popularity": 0.0,
           "tail_share": 0.0, "personalisation": 0.0, "ild": 0.0, "n_ild": 0, "n_lists": n_lists, "n_items": n, "n_shown": C}
    if C > 0:
        cf = c.astype(np.float64)
        j = np.arange(1, n + 1, dtype=np.float64)
        out["gini"] = float(((2.0 * j - n - 1.0) * np.sort(cf)).sum() / (float(n) * C))
        share = cf[c > 0] / C
        out["entropy"] = float(-(share * np.log2(share)).sum()) + 0.0
        out["novelty"] = float((cf * -np.log2((p.astype(np.float64) + 1.0) / (float(P) + n))).sum() / C)
        out["avg_popularity"] = float((cf * p.astype(np.float64)).sum() / C)
        # the head: by descending popularity, then ascending id (cat is ascending: a stable sort keeps the id order)
        order = np.argsort(-p, kind="stable")
        n_head = int(np.searchsorted(5 * np.cumsum(p[order]), 4 * P, side="left")) + 1 if P > 0 else 0
        out["tail_share"] = float(c[order[n_head:]].sum()) / C
    if n_lists >= 2:
        shared = int((c * (c - 1) // 2).sum())
        out["personalisation"] = 1.0 - shared / (n_lists * (n_lists - 1) / 2.0 * k)
    has = pairs > 0
    if has.any():
        out["n_ild"] = int(has.sum())
        out["ild"] = float((1.0 - sim_sum[has] / pairs[has].astype(np.float64)).mean())
    return out


# ------------------------------------------------------------------ run.py --list-metrics [K]
def report(model, k=DEFAULT_K, out_path=None):
    """`run.py --list-metrics [K]`: for every domain of the test set model.list_eval(d, k) -- the top-K lists of
    model.recommend(d, k) for its test users, their exposure counts, the train split's label-1 popularity counts and the
    lists' pairwise similarity on the item table of the weights that produced them (under the wrappers that keep a phi_d per
    domain, the best theta (+|*) phi_d of THAT domain) --, summarised.  Written to ONE .npz -- domains, k, per domain d
    catalogue_d [n], exposure_d / popularity_d [n] (in catalogue order), sim_sum_d / pairs_d [Q]; one [n domains] array per
    figure (FIGURES, n_ild) -- and printed, one line per domain.  -> (path, {domain: figures})."""
    k = check_k(k)
    domains = sorted(model.dataset.test_dataset)
    arrays, reports = {"domains": np.asarray(domains, np.int64), "k": np.asarray(k, np.int64)}, {}
    print("List metrics top-{} (what the lists are made of): ".format(k))
    for d in domains:
        r = model.list_eval(d, k)
        cat = np.asarray(r["catalogue"], np.int64)
        ids = np.asarray(r["ids"])
        m = reports[d] = summarise(r["exposure"], r["popularity"], cat, k, r["sim_sum"], r["pairs"],
                                   n_lists=int((ids >= 0).any(axis=1).sum()) if ids.size else 0)
        arrays["catalogue_%d" % d] = cat
        arrays["exposure_%d" % d] = np.asarray(r["exposure"], np.int64)[cat]
        arrays["popularity_%d" % d] = np.asarray(r["popularity"], np.int64)[cat]
        arrays["sim_sum_%d" % d] = np.asarray(r["sim_sum"], np.float64)
        arrays["pairs_%d" % d] = np.asarray(r["pairs"], np.int32)
        print("{}: Coverage@{k} {:.4f} Gini {:.4f} Entropy {:.3f} Novelty {:.3f} AvgPopularity {:.2f} TailShare {:.4f} "
              "Personalisation {:.4f} ILD {:.4f} ({} lists, {} items, {} lists with a pair)".format(
                  d, m["coverage"], m["gini"], m["entropy"], m["novelty"], m["avg_popularity"], m["tail_share"],
                  m["personalisation"], m["ild"], m["n_lists"], m["n_items"], m["n_ild"], k=k))
    for name in FIGURES:
        arrays[name] = np.asarray([reports[d][name] for d in domains], np.float64)
    arrays["n_ild"] = np.asarray([reports[d]["n_ild"] for d in domains], np.int64)
    if out_path is None:
        out_path = os.path.join(model.result_path, "list_metrics_top%d.npz" % k)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("List metrics written to {}".format(out_path))
    return out_path, reports


def headline(reports):
    """what result.json gains: domain_<figure> = {domain: value} for the eight FIGURES, and the plain means over the
    domains avg_coverage, avg_gini, avg_novelty, avg_personalisation and avg_ild (0.0 without a domain)."""
    out = {"domain_" + name: {str(d): r[name] for d, r in reports.items()} for name in FIGURES}
    for name in AVERAGED:
        out["avg_" + name] = float(np.mean([r[name] for r in reports.values()])) if reports else 0.0
    return out


# ------------------------------------------------------------------ run.py --diversify [LAMBDA]
def check_pool(k, pool=None):
    """the pool the K picks come from: by default min(128, 5 K); K <= pool <= 128."""
    k = check_k(k, "diversify")
    pool = min(MAX_K, 5 * k) if pool is None else int(pool)
    if not k <= pool <= MAX_K:
        raise ValueError("diversify: pool %d outside K = %d .. %d" % (pool, k, MAX_K))
    return k, pool


def check_lambda(lam):
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("diversify: lambda %r outside [0, 1]" % (lam,))
    return lam


SIDES = ("", "_diversified")        # a figure's key for the base top-K, for the re-ranked lists


def diversify_report(model, k=DEFAULT_K, lam=DEFAULT_LAMBDA, pool=None, out_path=None):
    """`run.py --diversify [LAMBDA]`: for every domain of the test set model.diversify_eval(d, k, pool, lam) -- each test
    user's top-`pool` list re-ranked to K items by mamdr_list_diversify on min-max relevance, and, for BOTH the base top-K and
    the re-ranked lists, exposure counts and pairwise similarity from the two device calls of `report` --; per side
    recommend.ranking_metrics against the test split's positives and `summarise`.  Written to ONE .npz -- domains, k, pool,
    lambda, per domain d users_d [Q], base_ids_d / ids_d / pos_d / values_d [Q, K]; one [n domains] array per figure
    (ACCURACY, FIGURES) and side (`<figure>`, `<figure>_diversified`) -- and printed, one line per domain with both sides.
    -> (path, {domain: {"base": figures, "diversified": figures}})."""
    from . import recommend as rec
    k, pool = check_pool(k, pool)
    lam = check_lambda(lam)
    domains = sorted(model.dataset.test_dataset)
    arrays = {"domains": np.asarray(domains, np.int64), "k": np.asarray(k, np.int64), "pool": np.asarray(pool, np.int64),
              "lambda": np.asarray(lam, np.float64)}
    reports = {}
    print("Diversify top-{} of top-{}, lambda {:g} (base -> re-ranked): ".format(k, pool, lam))
    for d in domains:
        r = model.diversify_eval(d, k, pool, lam)
        positives = rec.split_positives(model.dataset, d, r["users"])
        sides = {}
        for side, lists, pre in (("base", r["base_ids"], "base_"), ("diversified", r["ids"], "")):
            lists = np.asarray(lists)
            m = summarise(r[pre + "exposure"], r["popularity"], r["catalogue_ids"], k, r[pre + "sim_sum"], r[pre + "pairs"],
                          n_lists=int((lists >= 0).any(axis=1).sum()) if lists.size else 0)
            m.update(rec.ranking_metrics(lists, positives))
            sides[side] = m
        reports[d] = sides
        for name in ("users", "base_ids", "ids", "pos", "values"):
            arrays["%s_%d" % (name, d)] = np.asarray(r[name])
        b, v = sides["base"], sides["diversified"]
        print("{}: HitRate@{k} {:.4f} -> {:.4f} NDCG@{k} {:.4f} -> {:.4f} ILD {:.4f} -> {:.4f} Coverage@{k} {:.4f} -> {:.4f} "
              "Gini {:.4f} -> {:.4f} Novelty {:.3f} -> {:.3f} Personalisation {:.4f} -> {:.4f} ({} users, {} items)".format(
                  d, b["hit_rate"], v["hit_rate"], b["ndcg"], v["ndcg"], b["ild"], v["ild"], b["coverage"], v["coverage"],
                  b["gini"], v["gini"], b["novelty"], v["novelty"], b["personalisation"], v["personalisation"],
                  b["n_lists"], b["n_items"], k=k))
    for name in ACCURACY + FIGURES:
        for side, suffix in zip(("base", "diversified"), SIDES):
            arrays[name + suffix] = np.asarray([reports[d][side][name] for d in domains], np.float64)
    if out_path is None:
        out_path = os.path.join(model.result_path, "diversify_top%d.npz" % k)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Diversified lists written to {}".format(out_path))
    return out_path, reports


def diversify_headline(reports, lam, pool):
    """what result.json gains: diversify_lambda, diversify_pool; for the re-ranked lists domain_<figure>_diversified =
    {domain: value} for hit_rate / recall / ndcg and the eight FIGURES, avg_<figure>_diversified (AVERAGED) and
    avg_ndcg_diversified, the plain means over the domains (0.0 without one).  (The base side's figures are what
    --recommend and --list-metrics report.)"""
    out = {"diversify_lambda": float(lam), "diversify_pool": int(pool)}
    for name in ACCURACY + FIGURES:
        out["domain_%s_diversified" % name] = {str(d): r["diversified"][name] for d, r in reports.items()}
    for name in AVERAGED + ("ndcg",):
        out["avg_%s_diversified" % name] = float(np.mean([r["diversified"][name] for r in reports.values()])) if reports else 0.0
    return out
