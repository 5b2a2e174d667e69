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
