"""Similar items (`run.py --similar-items [K]`): exact cosine nearest neighbours of item-table rows, and what the
neighbour graph of a domain's catalogue looks like.  The documented host definitions of `mamdr_row_neighbours`
(include/mamdr_hip.h) and the report built on the device call.  No reference counterpart.

The call.  For every query row, its k nearest candidate rows by cos(q, c) = (x_q . x_c) / (|x_q| |x_c|), exactly 0 when
either norm is 0, ordered by (cosine descending, id ascending); the candidate with the query's own id is skipped under
exclude_self; an id outside [0, n_rows) is never a neighbour and, as a query, has no neighbours; a short list ends in
id -1 / sim 0.  `neighbours_host` is this in float64 on the given fp32 rows; `neighbours_replay` is the same selection on
given fp32 cosines under the device's ranking key (list_metrics.rank_keys), which a test feeds with the device's own
pair cosines to hold the selection byte for byte.

Figures per domain (`summarise`), n the catalogue's size, k' = min(k, n - 1), the lists those of every catalogue item
among the same catalogue:
  mean_sim_1, mean_sim_k   the mean cosine of the first / the k'-th neighbour over the items that have one
  in-degree N_k(j)         how many lists hold item j (`mamdr_id_counts` over the flattened lists)
  hubness                  the population skewness of N_k over the catalogue (Radovanovic et al. 2010), 0.0 at zero variance
  orphan_share             the share of items nobody lists (N_k = 0)
  max_in_degree            max N_k
  reciprocity              the share of edges i -> j whose reverse j -> i is in the lists
Across domains: affinity[d][d'] = the mean over d's catalogue of the top-1 cosine into d' 's catalogue (self excluded,
k = 1 calls; the diagonal is mean_sim_1), shared_items[d][d'] = the number of ids the two catalogues share.  This is the
embedding-space view of how close the domains are, beside the gradient-space view of `--conflict`.  With frozen tables
every domain reads the same pretrained table: the figures describe that table, not the training.

Determinism.  Distinct ids give distinct keys: a query's list is one list, whatever the grid, the order of the candidates
or the number of passes.  Against float64 a returned cosine is within list_metrics.error_bound(E), and a pick's float64
cosine is at least the float64 k-th best minus twice that.
"""
import os

import numpy as np

from . import list_metrics

MAX_K = 128                         # MAMDR_KNN_MAX_K
DEFAULT_K = 10                      # run.py --similar-items without a number
FIGURES = ("mean_sim_1", "mean_sim_k", "hubness", "orphan_share", "max_in_degree", "reciprocity")
AVERAGED = ("mean_sim_1", "mean_sim_k", "hubness", "orphan_share", "reciprocity")       # headline's avg_<figure>


def check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("similar items: k %d outside 1..%d" % (k, MAX_K))
    return k


# ------------------------------------------------------------------ host definitions of the device call
def _problem(n_rows, queries, k, candidates):
    k = check_k(k)
    q = np.asarray(queries).ravel().astype(np.int64)
    c = np.arange(n_rows, dtype=np.int64) if candidates is None else np.asarray(candidates).ravel().astype(np.int64)
    return q, c, k


def _select(keys, cand, k, sims, sim_dtype):
    """per row of `keys` [Q, C] (uint64, 0 = not eligible) the k largest, descending -> (ids int32 [Q, k], sims [Q, k])."""
    Q = keys.shape[0]
    ids_out = np.full((Q, k), -1, np.int32)
    sim_out = np.zeros((Q, k), sim_dtype)
    for i in range(Q):
        live = np.flatnonzero(keys[i])
        order = live[np.argsort(keys[i][live], kind="stable")[::-1]][:k]
        ids_out[i, :order.size] = cand[order]
        sim_out[i, :order.size] = sims[i][order]
    return ids_out, sim_out


def _eligible(q, c, n_rows, exclude_self):
    ok = ((q >= 0) & (q < n_rows))[:, None] & ((c >= 0) & (c < n_rows))[None, :]
    if exclude_self:
        ok &= q[:, None] != c[None, :]
    return ok


def neighbours_host(rows, queries, k, candidates=None, exclude_self=True):
    """mamdr_row_neighbours on the host, in float64 on the given fp32 rows -> (ids int32 [Q, k], sims float64 [Q, k]):
    per query the eligible candidates by (cosine descending, id ascending), NaN behind every number; -1 / 0.0 behind a
    short list."""
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 2:
        raise ValueError("similar items: rows must be [n_rows, emb_dim]")
    n_rows = rows.shape[0]
    q, c, k = _problem(n_rows, queries, k, candidates)
    ok = _eligible(q, c, n_rows, exclude_self)
    x = rows[np.clip(q, 0, n_rows - 1)].astype(np.float64)
    y = rows[np.clip(c, 0, n_rows - 1)].astype(np.float64)
    nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = (x @ y.T) / (nx[:, None] * ny[None, :])
    cos[(nx == 0)[:, None] | (ny == 0)[None, :]] = 0.0
    ids_out = np.full((q.size, k), -1, np.int32)
    sim_out = np.zeros((q.size, k), np.float64)
    for i in range(q.size):
        live = np.flatnonzero(ok[i])
        v = cos[i][live]
        # (cosine descending, id ascending), NaN last: lexsort's last key is the primary one
        order = live[np.lexsort((c[live], -np.where(np.isnan(v), -np.inf, v), np.isnan(v)))][:k]
        ids_out[i, :order.size] = c[order]
        sim_out[i, :order.size] = cos[i][order]
    return ids_out, sim_out


def neighbours_replay(pair_cos, queries, k, candidates=None, exclude_self=True, n_rows=None):
    """the device's selection on given fp32 cosines: pair_cos [Q, C] is cos(query i, candidate p) -> (ids int32 [Q, k],
    sims float32 [Q, k]) by the ranking key of (cos, id) -- fp32 values by their bits, NaN behind every number (returned as
    the quiet NaN), equal cosines by ascending id.  n_rows: the table's height (default: every id >= 0 is a row; with
    candidates None it is the number of columns)."""
    cos = np.asarray(pair_cos, np.float32)
    if cos.ndim != 2:
        raise ValueError("similar items: pair_cos must be [Q, C]")
    if n_rows is None:
        n_rows = cos.shape[1] if candidates is None else np.iinfo(np.int32).max
    q, c, k = _problem(int(n_rows), queries, k, candidates)
    if cos.shape != (q.size, c.size):
        raise ValueError("similar items: pair_cos %r for %d queries and %d candidates" % (cos.shape, q.size, c.size))
    keys = np.where(_eligible(q, c, int(n_rows), exclude_self), list_metrics.rank_keys(cos, np.broadcast_to(c, cos.shape)),
                    np.uint64(0))
    shown = np.where(np.isnan(cos), np.float32(np.nan), cos)          # (every NaN leaves as the quiet NaN)
    return _select(keys, c, k, shown, np.float32)


# ------------------------------------------------------------------ figures of one domain's neighbour graph
def summarise(items, ids, sims, catalogue, in_degree, k):
    """the figures (module docstring) of the lists ids / sims [Q, k] of the query items [Q] among `catalogue`; in_degree:
    N_k indexed by item id (at least max(catalogue) + 1 long)."""
    cat = np.unique(np.asarray(catalogue, np.int64).ravel())
    n, k = int(cat.shape[0]), int(k)
    items, ids, sims = np.asarray(items, np.int64).ravel(), np.asarray(ids, np.int64), np.asarray(sims, np.float64)
    if n == 0 or k < 1 or ids.ndim != 2 or ids.shape != sims.shape or ids.shape[0] != items.shape[0] or ids.shape[1] != k:
        raise ValueError("similar items: an empty catalogue, k < 1, or lists that are not [len(items), k]")
    in_degree = np.asarray(in_degree).ravel()
    if cat[0] < 0 or cat[-1] >= in_degree.shape[0]:
        raise ValueError("similar items: a catalogue id outside the in-degree vector")
    kk = min(k, n - 1)
    out = {"mean_sim_1": 0.0, "mean_sim_k": 0.0, "hubness": 0.0, "orphan_share": 0.0, "max_in_degree": 0, "reciprocity": 0.0,
           "n_items": n, "n_edges": int((ids >= 0).sum()), "k_eff": kk}
    if kk >= 1 and ids.shape[0]:
        first, last = ids[:, 0] >= 0, ids[:, kk - 1] >= 0
        out["mean_sim_1"] = float(sims[first, 0].mean()) if first.any() else 0.0
        out["mean_sim_k"] = float(sims[last, kk - 1].mean()) if last.any() else 0.0
    deg = in_degree[cat].astype(np.float64)
    mu = deg.mean()
    var = ((deg - mu) ** 2).mean()
    out["hubness"] = float(((deg - mu) ** 3).mean() / var ** 1.5) if var > 0 else 0.0
    out["orphan_share"] = float((deg == 0).mean())
    out["max_in_degree"] = int(deg.max())
    src = np.repeat(items, k)[(ids >= 0).ravel()]
    dst = ids.ravel()[(ids >= 0).ravel()]
    if src.size:
        base = int(max(src.max(), dst.max())) + 1
        out["reciprocity"] = float(np.isin(dst * base + src, src * base + dst).mean())
    return out


# ------------------------------------------------------------------ run.py --similar-items [K]
def report(model, k=DEFAULT_K, out_path=None):
    """`run.py --similar-items [K]`: for every domain d of the test set model.similar_items(d, k) -- the k nearest
    neighbours of every catalogue item among the same catalogue, on the item table of the domain's weights --, the
    in-degrees counted on the device, summarised; and for every ordered pair of domains the k = 1 call into the other
    catalogue (affinity).  Written to ONE .npz -- domains, k, per domain d catalogue_d [n], ids_d / sims_d [n, k],
    in_degree_d [n] (in catalogue order); one [n domains] array per figure (FIGURES); affinity / shared_items
    [n domains, n domains] -- and printed, one line per domain.  -> (path, {domain: figures + "affinity": {d': value}})."""
    import torch
    k = check_k(k)
    domains = sorted(model.dataset.test_dataset)
    eng = model.model
    arrays, reports, cats = {"domains": np.asarray(domains, np.int64), "k": np.asarray(k, np.int64)}, {}, {}
    frozen = not model.tables_trainable
    print("Similar items top-{} (exact cosine neighbours on the item table{}): ".format(
        k, "; the tables are frozen: this describes the pretrained table" if frozen else ""))
    for d in domains:
        r = model.similar_items(d, k)
        cat = cats[d] = np.asarray(r["catalogue"], np.int64)
        ids = np.ascontiguousarray(r["ids"], np.int32)
        n_item = int(eng.n_item)
        deg = list_metrics.to_host(eng.id_counts(torch.from_numpy(ids.ravel()).to(eng.device), n_item))
        deg = (deg.view(np.uint32) if deg.dtype == np.int32 else deg).astype(np.int64)
        m = reports[d] = summarise(r["items"], ids, r["sims"], cat, deg, k)
        arrays["catalogue_%d" % d] = cat
        arrays["ids_%d" % d] = ids
        arrays["sims_%d" % d] = np.asarray(r["sims"], np.float32)
        arrays["in_degree_%d" % d] = deg[cat]
        print("{}: MeanSim@1 {:.4f} MeanSim@{} {:.4f} Hubness {:.3f} OrphanShare {:.4f} MaxInDegree {} Reciprocity {:.4f} "
              "({} items, {} edges)".format(d, m["mean_sim_1"], m["k_eff"], m["mean_sim_k"], m["hubness"], m["orphan_share"],
                                            m["max_in_degree"], m["reciprocity"], m["n_items"], m["n_edges"]))
    affinity = np.zeros((len(domains), len(domains)), np.float64)
    shared = np.zeros((len(domains), len(domains)), np.int64)
    for i, d in enumerate(domains):
        for j, e in enumerate(domains):
            shared[i, j] = np.intersect1d(cats[d], cats[e]).size
            if i == j:
                affinity[i, j] = reports[d]["mean_sim_1"]
                continue
            r = model.similar_items(d, 1, target_domain=e)
            has = np.asarray(r["ids"])[:, 0] >= 0
            affinity[i, j] = float(np.asarray(r["sims"], np.float64)[has, 0].mean()) if has.any() else 0.0
        reports[d]["affinity"] = {int(e): float(affinity[i, j]) for j, e in enumerate(domains)}
    for name in FIGURES:
        arrays[name] = np.asarray([reports[d][name] for d in domains], np.float64)
    arrays["affinity"], arrays["shared_items"] = affinity, shared
    if len(domains) > 1:
        print("Embedding-space affinity (mean top-1 cosine of a row's items into a column's catalogue):")
        for i, d in enumerate(domains):
            print("{}: {}".format(d, " ".join("{:.4f}".format(v) for v in affinity[i])))
    if out_path is None:
        out_path = os.path.join(model.result_path, "similar_items_top%d.npz" % k)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Similar items written to {}".format(out_path))
    return out_path, reports


def headline(reports):
    """what result.json gains: domain_<figure> = {domain: value} for FIGURES, the plain means over the domains
    avg_<figure> for AVERAGED (0.0 without a domain), and domain_affinity = {domain: {domain: value}}."""
    out = {"domain_" + name: {str(d): r[name] for d, r in reports.items()} for name in FIGURES}
    for name in AVERAGED:
        out["avg_" + name] = float(np.mean([r[name] for r in reports.values()])) if reports else 0.0
    out["domain_affinity"] = {str(d): {str(e): v for e, v in r.get("affinity", {}).items()} for d, r in reports.items()}
    return out
