"""Isotonic recalibration and the CORP score decomposition, host side: the documented host definition of
`mamdr_isotonic_fit`, `mamdr_isotonic_apply` and `mamdr_score_sums`, the report of one domain, its summary over domains and
`run.py --isotonic`.  Pure numpy and `fractions`.  The reference has no counterpart: it never looks at calibration.

Rows and runs.  Rows of one split: fp32 prediction p_i, label y_i.

- `key` is GAUC's order-preserving 32-bit key (`gauc.ordered_key`): NaN is lowest and equals NaN, -0 equals +0.
- `positive` is `label != 0`.

Sort by key ascending.  A run is a maximal set of rows with one key; run j has r_j rows and s_j positives.  Points
Q_0 = (0, 0), Q_{j+1} = Q_j + (r_j, s_j), R runs in all.  NaN predictions form the lowest run and take part like any other;
`n_nan` is reported.

Fit.  The blocks are the maximal groups of consecutive runs between consecutive *strict* vertices of the lower convex hull
of Q_0 .. Q_R: with A, B, C consecutive candidates, B is dropped exactly when
(B.x - A.x) * (C.y - B.y) - (B.y - A.y) * (C.x - B.x) <= 0 in int64 (coordinates are below 2^31, so the products are below
2^62).  Equivalently: pool adjacent violators (PAV) over the runs, pooling the last two blocks while
mean_left >= mean_right.  Block b has `first_key[b]` (the key of its first run), `rows[b]` and `positives[b]`; block means
are strictly increasing.  Value v_b = `(float)((double) positives[b] / (double) rows[b])`: one fp64 division, rounded once
to fp32.  The fit is the left derivative of the greatest convex minorant of the cumulative-sum diagram: exact and unique.

Apply.  For a row with key k: b = max(0, #{blocks with first_key <= k} - 1), output v_b -- a step function, clipped at both
ends.  scikit-learn's `IsotonicRegression` interpolates linearly between thresholds instead; on the fitted rows themselves
the two agree.

Score sums.  Two fp64 sums, with y = positive and p widened to fp64: the Brier sum, sum (p - y)^2, and the log-loss sum,
sum -[y ln q + (1 - y) ln(1 - q)] with q = clamp(p, 1e-7, 1 - 1e-7), the Keras epsilon.  A NaN prediction makes both sums
NaN: it is reported, not hidden.

CORP decomposition of a split's Brier score (Dimitriadis, Gneiting, Jordan, PNAS 2021), from the split's OWN fit, in fp64,
from the block table alone.  With n rows, P positives and S the Brier mean:

- S_c = sum_b positives_b * (rows_b - positives_b) / rows_b / n    (the Brier mean of the recalibrated predictions)
- UNC = P (n - P) / n^2
- MCB = S - S_c     (miscalibration: what recalibrating on the split itself would gain)
- DSC = UNC - S_c   (discrimination)
- S = MCB - DSC + UNC.

The device (csrc/isotonic_kernels.hip) sorts with a radix sort, counts runs with scans and builds the hull by levels of
per-tile monotone chains; `fit_host` uses `np.sort` and a stack of pooled blocks over the runs -- two algorithms for the
same integers.
"""
import math
import os

import numpy as np

from . import exact, gauc

# csrc/mamdr_kernels.h: the constants of the device chain (tests read them here)
POINT_TILE = 1024       # ISO_POINT_TILE: sorted positions per workgroup of k_iso_run_sums / k_iso_points
SCAN_TILE = 1024        # ISO_SCAN_TILE: 64-bit words per workgroup of the device-wide scans
HULL_TILE = 64          # ISO_HULL_TILE: points per tile of the hull's levels in mamdr_isotonic_fit
MIN_TILE = 4            # ISO_MIN_TILE = MAMDR_ISOTONIC_MIN_TILE: the smallest tile_points of mamdr_isotonic_fit_bounded
MAX_LEVELS = 32         # ISO_MAX_LEVELS
APPLY_TILE = 2048       # ISO_APPLY_TILE: rows per workgroup of k_iso_apply
APPLY_LDS = 4096        # ISO_APPLY_LDS: blocks up to which k_iso_apply searches first_key in LDS
SCORE_TILE = 1024       # ISO_SCORE_TILE: rows per workgroup of k_score_parts
COUNTS = ("n_blocks", "n_runs", "n_nan", "P")       # the words of d_counts, in order
MAX_BINS = exact.MAX_BINS
EPS = 1e-7              # the Keras epsilon of the log loss


def check_bins(n_bins, what="isotonic"):
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("%s: n_bins %d outside 1..%d" % (what, n_bins, MAX_BINS))
    return n_bins


def runs_host(pred, label):
    """the runs of equal keys in ascending order -> (key uint32 [R], rows int64 [R], positives int64 [R])."""
    comp = np.sort(exact.composites(pred, label))
    n = int(comp.shape[0])
    if n >= 2 ** 31:
        raise ValueError("isotonic: %d rows (positions are below 2^31)" % n)
    key = (comp >> np.uint64(1)).astype(np.uint32)
    positive = (comp & np.uint64(1)).astype(np.int64)
    if n == 0:
        return key, np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    edge = np.concatenate([head, [n]])
    cp = np.concatenate([[0], np.cumsum(positive, dtype=np.int64)])
    return key[head], np.diff(edge).astype(np.int64), (cp[edge[1:]] - cp[edge[:-1]]).astype(np.int64)


def fit_host(pred, label):
    """the definition on the host -> (counts [4] int64: n_blocks, n_runs, n_nan, P; first_key uint32 [n_blocks]; rows int64
    [n_blocks]; positives int64 [n_blocks]).  PAV over the runs: the last two blocks are pooled while
    mean_left >= mean_right, compared as positives_left * rows_right >= positives_right * rows_left in Python integers."""
    key, run_rows, run_pos = runs_host(pred, label)
    blocks = []                  # [first key, rows, positives]
    for k, r, s in zip(key.tolist(), run_rows.tolist(), run_pos.tolist()):
        blocks.append([k, r, s])
        while len(blocks) >= 2 and blocks[-2][2] * blocks[-1][1] >= blocks[-1][2] * blocks[-2][1]:
            _, r1, s1 = blocks.pop()
            blocks[-1][1] += r1
            blocks[-1][2] += s1
    table = np.asarray(blocks, np.int64).reshape(-1, 3)
    n_nan = int(run_rows[0]) if key.shape[0] and key[0] == 0 else 0
    counts = np.asarray([table.shape[0], key.shape[0], n_nan, int(run_pos.sum())], np.int64)
    return counts, table[:, 0].astype(np.uint32), table[:, 1].copy(), table[:, 2].copy()


def values(rows, positives):
    """v_b = (float)((double) positives_b / (double) rows_b): fp32 [n_blocks]."""
    return (np.asarray(positives, np.int64).astype(np.float64) / np.asarray(rows, np.int64).astype(np.float64)).astype(np.float32)


def apply_host(first_key, rows, positives, pred):
    """the step function of a fit at `pred` -> fp32 [n]: block max(0, #{first_key <= key} - 1) of every row."""
    first_key = np.asarray(first_key, np.uint32)
    key = gauc.ordered_key(pred)
    if key.shape[0] == 0:
        return np.zeros(0, np.float32)
    if first_key.shape[0] == 0:
        raise ValueError("isotonic: a fit without blocks cannot be applied")
    b = np.maximum(np.searchsorted(first_key, key, side="right") - 1, 0)
    return values(rows, positives)[b]


def score_sums_host(pred, label):
    """(Brier sum, log-loss sum) of the definition, each added exactly (math.fsum) from fp64 terms."""
    p = np.asarray(pred, np.float32).ravel().astype(np.float64)
    y = np.asarray(label).ravel() != 0
    if p.shape[0] != y.shape[0]:
        raise ValueError("isotonic: pred and label differ in length")
    d = p - y.astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where(p < EPS, EPS, np.where(p > 1.0 - EPS, 1.0 - EPS, p))       # (a NaN stays a NaN)
    terms = [-math.log(v) if v == v else v for v in np.where(y, q, 1.0 - q).tolist()]
    return math.fsum((d * d).tolist()), math.fsum(terms)


def corp(rows, positives, brier_mean):
    """the CORP decomposition of a split's Brier mean from the split's own block table -> {"mcb", "dsc", "unc"} in fp64;
    zeros for an empty split."""
    rows, positives = np.asarray(rows, np.int64), np.asarray(positives, np.int64)
    n, P = int(rows.sum()), int(positives.sum())
    if n == 0:
        return {"mcb": 0.0, "dsc": 0.0, "unc": 0.0}
    s_c = float(np.sum(positives * (rows - positives) / rows.astype(np.float64))) / n
    unc = P * (n - P) / float(n) ** 2
    return {"mcb": float(brier_mean) - s_c, "dsc": unc - s_c, "unc": unc}


def table(counts, first_key, rows, positives):
    """the block table of one fit from the outputs of mamdr_isotonic_fit / fit_host (arrays of any capacity >= n_blocks)
    -> {"n_blocks", "n_runs", "n_nan", "P", "n", "first_key" uint32, "first_pred" fp32 (the thresholds as predictions:
    exact.prediction_of_key), "rows", "positives" int64}."""
    c = [int(v) for v in np.asarray(counts).ravel()[:4]]
    nb = c[0]
    first_key = np.ascontiguousarray(first_key).ravel()[:nb]
    # (a device tensor holds the uint32 words as int32: reinterpret, do not convert)
    first_key = first_key.view(np.uint32) if first_key.dtype == np.int32 else first_key.astype(np.uint32)
    rows = np.asarray(rows, np.int64).ravel()[:nb].copy()
    out = dict(zip(COUNTS, c))
    out.update(n=int(rows.sum()), first_key=first_key.copy(), first_pred=exact.prediction_of_key(first_key),
               rows=rows, positives=np.asarray(positives, np.int64).ravel()[:nb].copy())
    return out


def finish(val_fit, test_fit, sums, sums_isotonic, exact_before, exact_after):
    """the report of one domain: val_fit / test_fit are `table`s of the val and the test split; sums / sums_isotonic the
    (Brier sum, log-loss sum) of the test split before and after val's fit is applied to it; exact_before / exact_after
    the exact.finish reports of the same two prediction vectors (ECE / PCOC side by side)."""
    n = test_fit["n"]
    mean = lambda v: float(v) / n if n else 0.0      # noqa: E731
    rep = {"n": n, "P": test_fit["P"], "n_nan": test_fit["n_nan"], "n_blocks": val_fit["n_blocks"],
           "n_blocks_test": test_fit["n_blocks"], "n_runs": test_fit["n_runs"],
           "brier": mean(sums[0]), "logloss": mean(sums[1]),
           "brier_isotonic": mean(sums_isotonic[0]), "logloss_isotonic": mean(sums_isotonic[1]),
           "ece": exact_before["ece"], "pcoc": exact_before["pcoc"],
           "ece_isotonic": exact_after["ece"], "pcoc_isotonic": exact_after["pcoc"],
           "val": val_fit, "test": test_fit}
    rep.update(corp(test_fit["rows"], test_fit["positives"], rep["brier"]))
    return rep


SUMMARY_KEYS = ("mcb", "dsc", "unc", "brier", "brier_isotonic", "logloss", "logloss_isotonic")


def summarise(reports):
    """{domain: report} -> {key: (plain mean over the domains, row-weighted mean)} for SUMMARY_KEYS; (0.0, 0.0) without rows."""
    reps = [r for r in reports.values() if r["n"]]
    rows = sum(r["n"] for r in reps)
    return {k: ((sum(r[k] for r in reps) / len(reps), sum(r["n"] * r[k] for r in reps) / rows) if reps else (0.0, 0.0))
            for k in SUMMARY_KEYS}


def headline(reports):
    """what result.json gains: the per-domain figures and the two means of MCB."""
    out = {}
    for name, key in (("domain_brier", "brier"), ("domain_brier_isotonic", "brier_isotonic"), ("domain_logloss", "logloss"),
                      ("domain_logloss_isotonic", "logloss_isotonic"), ("domain_ece_isotonic", "ece_isotonic"),
                      ("domain_pcoc_isotonic", "pcoc_isotonic"), ("domain_mcb", "mcb"), ("domain_dsc", "dsc"),
                      ("domain_unc", "unc"), ("domain_isotonic_blocks", "n_blocks")):
        out[name] = {str(d): r[key] for d, r in reports.items()}
    out["avg_mcb"], out["weighted_mcb"] = summarise(reports)["mcb"]
    return out


def levels(n, tile):
    """the levels of tiles mamdr_isotonic_fit_bounded runs before its final chain (iso_levels, csrc/isotonic_kernels.hip):
    fixed from n and tile_points alone, as if every level shrank by tile / 2."""
    count, most = 0, int(n) + 1
    while most > tile and count < MAX_LEVELS:
        most = 2 * -(-most // tile)
        count += 1
    return count


def level_counts_host(pred, label, tile):
    """the points alive before every level of the device's hull and before its final chain -- what the levels of per-tile
    chains leave (tools/isotonic_bench.py prints them) -> a list of levels(n, tile) + 1 counts."""
    _, run_rows, run_pos = runs_host(pred, label)
    pts = list(zip(np.concatenate([[0], np.cumsum(run_rows)]).tolist(), np.concatenate([[0], np.cumsum(run_pos)]).tolist()))
    alive = [len(pts)]
    for _ in range(levels(int(run_rows.sum()), tile)):
        kept = []
        for first in range(0, len(pts), tile):
            st = []
            for c in pts[first:first + tile]:
                while len(st) >= 2 and (st[-1][0] - st[-2][0]) * (c[1] - st[-1][1]) - (st[-1][1] - st[-2][1]) * (c[0] - st[-1][0]) <= 0:
                    st.pop()
                st.append(c)
            kept.extend(st)
        pts = kept
        alive.append(len(pts))
    return alive


def report(model, n_bins=20, out_path=None):
    """`run.py --isotonic [B]`: for every domain model.isotonic_eval (under the wrappers that keep a phi_d per domain, the
    best theta (+|*) phi_d of THAT domain): the isotonic fit of the val split, applied to the test split; the test split's
    Brier and log loss before and after, its ECE / PCOC over B equal-mass bins before and after, and the CORP decomposition
    of its Brier score from its own fit.  Written to ONE .npz -- domains, n_bins, per domain d the val block table
    (val_first_pred_d, val_first_key_d, val_rows_d, val_positives_d), the test block table (test_..._d) and counts_d (int64
    [2, 5]: n_blocks, n_runs, n_nan, P, n of val and test); mcb / dsc / unc / brier / brier_isotonic / logloss /
    logloss_isotonic [n domains] -- and printed, one line per domain.  -> (path, {domain: report})."""
    n_bins = check_bins(n_bins)
    domains = sorted(model.dataset.test_dataset)
    arrays, reports = {"domains": np.asarray(domains, np.int64), "n_bins": np.asarray(n_bins, np.int64)}, {}
    print("Isotonic recalibration (fitted on val, applied to test) and CORP decomposition of the test Brier score: ")
    for d in domains:
        r = reports[d] = model.isotonic_eval(d, n_bins)
        for split in ("val", "test"):
            for name in ("first_pred", "first_key", "rows", "positives"):
                arrays["%s_%s_%d" % (split, name, d)] = r[split][name]
        arrays["counts_%d" % d] = np.asarray([[r[s][k] for k in COUNTS + ("n",)] for s in ("val", "test")], np.int64)
        print("{}: Brier {:.6f} -> {:.6f} LogLoss {:.6f} -> {:.6f} ECE {:.4f} -> {:.4f} PCOC {:.3f} -> {:.3f} "
              "MCB {:.6f} DSC {:.6f} UNC {:.6f} ({} rows, {} val blocks, {} NaN)".format(
                  d, r["brier"], r["brier_isotonic"], r["logloss"], r["logloss_isotonic"], r["ece"], r["ece_isotonic"],
                  r["pcoc"], r["pcoc_isotonic"], r["mcb"], r["dsc"], r["unc"], r["n"], r["n_blocks"], r["n_nan"]))
    for k in SUMMARY_KEYS:
        arrays[k] = np.asarray([reports[d][k] for d in domains], np.float64)
    s = summarise(reports)
    print("Overall MCB: {}, Weighted MCB: {}; DSC: {}, Weighted DSC: {}".format(s["mcb"][0], s["mcb"][1], s["dsc"][0], s["dsc"][1]))
    if out_path is None:
        out_path = os.path.join(model.result_path, "isotonic.npz")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    np.savez(out_path, **arrays)
    print("Isotonic fits written to {}".format(out_path))
    return out_path, reports
