"""Domain-conflict report (no reference counterpart): how much do the domains' gradients on the SAME weights disagree?

MAMDR's premise is that domains conflict -- their gradients on the shared parameters point in different directions -- and
Domain Negotiation exists to raise the inner products of those gradients.  This module measures it: one gradient per domain
at one point of weight space (`engine.domain_gradients`: MAMDR_OPT_ACCUMULATE steps, dropout off), their D x D Gram matrix
over the whole flat vector, the meta range and every tensor (`engine.gram`: mamdr_gram, deterministic fp64 on the device),
and from it, on the host in numpy fp64, the pairwise cosines and two summaries: the share of domain pairs with a negative
cosine (`conflict_rate`) and the mean cosine.

What the gradient is.  It is the gradient of the TOTAL loss of a batch, the L2 terms included, summed over the batches and
divided by their number.  On trainable tables the L2 term 2 * l2 * w is the same vector for every domain: it is shared by
all of them and pulls their cosines up, the more the smaller the data term is.  The per-tensor rows of the report are there
so that the dense layers can be read apart from the tables ("all" is dominated by whatever tensor carries most norm).

Pure numpy here; the engine calls go through `measure`, which any object with `domain_gradients`, `gram`, `segments`,
`n_params`, `meta_off` and `n_meta` serves.
"""
import os

import numpy as np

DEFAULT_BATCHES = 8         # run.py --conflict without a number: batches per domain


def _host(x):
    """device tensor or array -> numpy."""
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def cosines(gram):
    """G_ij / sqrt(G_ii * G_jj) of Gram matrices [..., D, D], fp64.  A vector of zero norm (G_ii == 0) has no direction: its
    row and column are nan, the diagonal element included.  A symmetric G gives a symmetric result, with an exact 1 on the
    diagonal wherever G_ii > 0."""
    g = np.asarray(gram, np.float64)
    diag = np.diagonal(g, axis1=-2, axis2=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = g / np.sqrt(diag[..., :, None] * diag[..., None, :])
    dead = ~(diag > 0)
    cos = np.where(dead[..., :, None] | dead[..., None, :], np.nan, cos)
    return cos


def summary(cos):
    """over the pairs i < j of one cosine matrix [D, D] whose cosine is finite -> {"conflict_rate": share of them with
    cos < 0 (0.0 without pairs), "mean_cosine", "min_cosine", "min_pair": the (i, j) that attains it (nan, nan, None without
    pairs), "n_pairs"}."""
    cos = np.asarray(cos, np.float64)
    iu, ju = np.triu_indices(cos.shape[-1], k=1)
    vals = cos[iu, ju]
    keep = np.isfinite(vals)
    vals, iu, ju = vals[keep], iu[keep], ju[keep]
    if vals.size == 0:
        return {"conflict_rate": 0.0, "mean_cosine": float("nan"), "min_cosine": float("nan"), "min_pair": None, "n_pairs": 0}
    k = int(np.argmin(vals))
    return {"conflict_rate": float(np.count_nonzero(vals < 0)) / vals.size, "mean_cosine": float(vals.mean()),
            "min_cosine": float(vals[k]), "min_pair": (int(iu[k]), int(ju[k])), "n_pairs": int(vals.size)}


def range_table(engine):
    """[(name, offset, count)]: "all", "meta" (the engine's meta range) and every segment of the flat vector."""
    return [("all", 0, int(engine.n_params)), ("meta", int(engine.meta_off), int(engine.n_meta))] + \
        [(name, int(off), int(cnt)) for name, (off, cnt) in engine.segments.items()]


def measure(engine, domains, n_batches=None):
    """one gradient per domain at the engine's live weights and their Gram matrices over range_table(engine).
    n_batches: batches per domain (None or 0: whole passes).  -> {"domains" [D], "steps" [D], "ranges" (names), "offsets",
    "counts" [R], "gram" [R, D, D]: the Gram of the MEAN gradients -- the device's Gram of the summed gradients divided by
    steps_i * steps_j (a domain without steps keeps its zeros) --, "cosine" [R, D, D], "norm" [R, D]: the mean gradients'
    norms, "conflict_rate", "mean_cosine" [R]}."""
    domains = [int(d) for d in domains]
    table = range_table(engine)
    rows, steps = engine.domain_gradients(domains, n_batches or None)
    sums = _host(engine.gram(rows, [(off, cnt) for _, off, cnt in table])).astype(np.float64)
    steps = np.asarray(_host(steps), np.int64)
    s = np.where(steps > 0, steps, 1).astype(np.float64)
    gram = sums / (s[:, None] * s[None, :])
    cos = cosines(gram)
    stats = [summary(c) for c in cos]
    return {"domains": np.asarray(domains, np.int64), "steps": steps,
            "ranges": np.asarray([name for name, _, _ in table]),
            "offsets": np.asarray([off for _, off, _ in table], np.int64),
            "counts": np.asarray([cnt for _, _, cnt in table], np.int64),
            "gram": gram, "cosine": cos, "norm": np.sqrt(np.diagonal(gram, axis1=1, axis2=2)),
            "conflict_rate": np.asarray([m["conflict_rate"] for m in stats], np.float64),
            "mean_cosine": np.asarray([m["mean_cosine"] for m in stats], np.float64)}


def report(model, n_batches=DEFAULT_BATCHES, out_path=None):
    """`run.py --conflict [N]`: model.domain_conflict(n_batches) -- under MAMDR and its relatives at the best theta, the
    shared point Domain Negotiation works on -- written to ONE .npz (measure's keys) and printed, one line per range.
    -> (path, measure's dict)."""
    res = model.domain_conflict(n_batches)
    print("Domain conflict ({} domains, {} batches each; cosines between the domains' mean gradients): ".format(
        len(res["domains"]), "/".join(str(int(s)) for s in sorted(set(res["steps"].tolist())))))
    for r, name in enumerate(res["ranges"].tolist()):
        m = summary(res["cosine"][r])
        pair = "-" if m["min_pair"] is None else "domains {} / {}".format(int(res["domains"][m["min_pair"][0]]),
                                                                         int(res["domains"][m["min_pair"][1]]))
        print("{}: ConflictRate {:.4f} MeanCosine {:.4f} MinCosine {:.4f} ({}) over {} pairs, {} floats".format(
            name, m["conflict_rate"], m["mean_cosine"], m["min_cosine"], pair, m["n_pairs"], int(res["counts"][r])))
    if out_path is None:
        out_path = os.path.join(model.result_path, "domain_conflict.npz")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **res)
    print("Domain conflict written to {}".format(out_path))
    return out_path, res


def headline(res):
    """the four scalars result.json carries: conflict_rate / mean_cosine of the "all" and the "meta" range."""
    names = res["ranges"].tolist()
    out = {}
    for name in ("all", "meta"):
        r = names.index(name)
        out["conflict_rate_" + name] = float(res["conflict_rate"][r])
        out["mean_cosine_" + name] = float(res["mean_cosine"][r])
    return out
