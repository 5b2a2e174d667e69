"""Exact AUC, average precision and equal-mass calibration of one split's predictions, host side: the documented host
definition, the report and its summary over domains.  Pure numpy.  The reference has no counterpart: every AUC it prints is
`AUC(num_thresholds=500)`, a trapezoid over 500 evenly spaced thresholds (base_model.py:111-144), which stays the metric
of parity, early stopping and checkpoints.

Definition.  For one split of n rows, per row:

- `key` is GAUC's order-preserving 32-bit key (`gauc.ordered_key`): NaN is lowest and equals NaN, -0 equals +0.
- `positive` is `label != 0`.
- The composite is `(uint64) key << 1 | positive`.

Sort the composites ascending.  Equal composites are indistinguishable, so the sorted array is unique.  Inside a run of
equal keys the negatives come first.  For sorted position i:

- `rs(i)` is the first position of i's run of equal keys.
- `cp(i)` is the number of positives at positions < i.
- `cn(i) = i - cp(i)`.

Results (every integer exact, in int64):

- `T = sum_{i positive} (cn(rs(i)) + cn(i))`.  This is `2 * #{s_p > s_n} + #{s_p == s_n}`, the integer
  `gauc.group_auc_host` gives for the whole split as one group.  `P`, `N`; `n_runs`, the number of distinct keys; `n_nan`.
  `AUC = T / (2 * P * N)`; when `P * N == 0` it is 0.0 with `valid = 0` (the convention of `recommend.ranking_metrics`).
- `ap_sum = sum_{i positive} (double)(P - cp(rs(i))) / (double)(n - rs(i))`; average precision is `ap_sum / P`, 0.0 when
  `P = 0`.  This is scikit-learn's step-wise definition: each positive contributes the precision at its own threshold.
- `bins` [3][n_bins]: every row of a run goes to bin `floor(rs(i) * n_bins / n)`: rows, positives, and the sum of the
  predictions in Q32 fixed point, `floor(clamp(p, 0, 1) * 2^32 + 0.5)` evaluated in fp64.  A NaN prediction adds 0 and is
  counted in `n_nan`.  A tie run is never split across bins, so bins may come out empty or unequal.

The device (csrc/exact_kernels.hip, `mamdr_exact_metrics`) sorts with a radix sort and scans; `metrics_host` uses
`np.sort` and `np.cumsum` -- two algorithms for the same integers.
"""
import numpy as np

from . import gauc

# csrc/mamdr_kernels.h: the tile and capacity constants of the device chain (tests read them here)
RADIX_BITS = 8          # EXACT_RADIX_BITS: digit width of the sort; ceil(33 / 8) = 5 passes
SORT_TILE = 2048        # EXACT_SORT_TILE: composites per workgroup of k_exact_hist / k_exact_scatter
SCAN_TILE = 512         # EXACT_SCAN_TILE: elements per workgroup of the device-wide scans
METRIC_TILE = 1024      # EXACT_METRIC_TILE: sorted positions per workgroup of k_exact_runs / k_exact_metrics
MAX_BINS = 4096         # MAMDR_EXACT_MAX_BINS
COUNTS = ("T", "P", "N", "n_runs", "n_nan")      # the words of d_counts, in order


def composites(pred, label):
    """uint64 [n]: (uint64) ordered_key(pred) << 1 | (label != 0), in file order."""
    key = gauc.ordered_key(pred).astype(np.uint64)
    positive = np.asarray(label).ravel() != 0
    if key.shape[0] != positive.shape[0]:
        raise ValueError("exact: pred and label differ in length")
    return (key << np.uint64(1)) | positive.astype(np.uint64)


def prediction_of_key(key):
    """the fp32 prediction behind an ordered key (NaN's key 0 gives a NaN)."""
    key = key.astype(np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).astype(np.uint32)
    return bits.view(np.float32)


def metrics_host(pred, label, n_bins, want_sorted=False):
    """the definition on the host -> (counts [5] int64: T, P, N, n_runs, n_nan; ap_sum float; bins [3][n_bins] int64)
    and, with want_sorted, the sorted composites as int64 [n]."""
    n_bins = int(n_bins)
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("exact: n_bins %d outside 1..%d" % (n_bins, MAX_BINS))
    comp = np.sort(composites(pred, label))
    n = int(comp.shape[0])
    counts = np.zeros(5, np.int64)
    bins = np.zeros((3, n_bins), np.int64)
    if n >= 2 ** 31:
        raise ValueError("exact: %d rows (positions are below 2^31)" % n)
    if n == 0:
        return (counts, 0.0, bins, comp.astype(np.int64)) if want_sorted else (counts, 0.0, bins)
    key = (comp >> np.uint64(1)).astype(np.uint32)
    positive = (comp & np.uint64(1)).astype(bool)
    pos = np.arange(n, dtype=np.int64)
    start = np.concatenate([[True], key[1:] != key[:-1]])
    rs = np.maximum.accumulate(np.where(start, pos, 0))
    cp = np.cumsum(positive, dtype=np.int64) - positive                # positives at positions < i
    cn = pos - cp
    P = int(positive.sum())
    counts[:] = (int((cn[rs] + cn)[positive].sum()), P, n - P, int(start.sum()), int((key == 0).sum()))
    # one division per positive, then the sum (the device adds the same terms over a fixed tree)
    ap_sum = float(((P - cp[rs])[positive].astype(np.float64) / (n - rs)[positive].astype(np.float64)).sum())
    which = rs * n_bins // n
    p = prediction_of_key(key).astype(np.float64)
    with np.errstate(invalid="ignore"):
        q32 = np.floor(np.clip(p, 0.0, 1.0) * 4294967296.0 + 0.5)
    q32 = np.where(key == 0, 0.0, q32).astype(np.int64)
    # `which` ascends with the position: every bin is a slice of the sorted order, its sums differences of int64 prefix sums
    edges = np.searchsorted(which, np.arange(n_bins + 1))
    for row, values in enumerate((np.ones(n, np.int64), positive.astype(np.int64), q32)):
        prefix = np.concatenate([[0], np.cumsum(values, dtype=np.int64)])
        bins[row] = prefix[edges[1:]] - prefix[edges[:-1]]
    return (counts, ap_sum, bins, comp.astype(np.int64)) if want_sorted else (counts, ap_sum, bins)


def finish(counts, ap_sum, bins):
    """the report of one split from the outputs of mamdr_exact_metrics / metrics_host: auc, ap, valid, P, N, n_runs,
    n_nan; ece = sum_b rows_b / n * |mean_pred_b - positives_b / rows_b| over the non-empty bins; pcoc = sum pred / P
    (predicted over observed clicks; 0.0 when P = 0); and the bin arrays: bin_rows, bin_positives, bin_pred_q32 (the device's exact Q32 sums) and bin_pred_sum (the same in
    prediction units)."""
    T, P, N, n_runs, n_nan = [int(c) for c in np.asarray(counts).ravel()[:5]]
    bins = np.asarray(bins, np.int64).reshape(3, -1)
    rows, positives = bins[0].copy(), bins[1].copy()
    pred_sum = bins[2].astype(np.float64) / 4294967296.0
    n = P + N
    valid = int(P > 0 and N > 0)
    full = rows > 0
    ece = 0.0
    if n:
        ece = float(np.sum(rows[full] / float(n) * np.abs(pred_sum[full] / rows[full] - positives[full] / rows[full].astype(np.float64))))
    ap_sum = float(np.asarray(ap_sum, np.float64).ravel()[0])
    return {"auc": T / (2 * P * N) if valid else 0.0, "ap": ap_sum / P if P else 0.0, "valid": valid,
            "P": P, "N": N, "n_runs": n_runs, "n_nan": n_nan, "ece": ece,
            "pcoc": float(pred_sum.sum()) / P if P else 0.0,
            "bin_rows": rows, "bin_positives": positives, "bin_pred_sum": pred_sum, "bin_pred_q32": bins[2].copy()}


def report_host(pred, label, n_bins):
    """finish(metrics_host(...)): the report of one split computed on the host."""
    return finish(*metrics_host(pred, label, n_bins))


def summarise(reports):
    """{domain: report} -> {"auc": (plain mean over the domains with `valid`, row-weighted mean), "ap": ..., "ece": ...};
    every pair is (0.0, 0.0) when no domain is valid."""
    reps = [r for r in reports.values() if r["valid"]]
    out = {}
    for k in ("auc", "ap", "ece"):
        if not reps:
            out[k] = (0.0, 0.0)
            continue
        rows = sum(r["P"] + r["N"] for r in reps)
        out[k] = (sum(r[k] for r in reps) / len(reps), sum((r["P"] + r["N"]) * r[k] for r in reps) / rows)
    return out
