"""Bootstrap confidence intervals for the exact AUC, host side: the documented host definition of `mamdr_auc_bootstrap`
(include/mamdr_hip.h), the summary of its replicates, paired comparisons and the summary over domains.  Pure numpy.  The
reference has no counterpart: every figure it reports is a point estimate.

Definition.  Rows order as in exact.py -- `key` is GAUC's order-preserving 32-bit key (NaN is lowest and equals NaN, -0
equals +0), `positive` is `label != 0`, inside a run of equal keys the negatives come first -- with the row index breaking
the remaining ties, which makes the sorted array unique.

- `unit(i)` is `(uint32) unit[i]` when a unit column is given, else `(uint32) i`: the split's uid column resamples users
  (the cluster bootstrap), none resamples rows.
- Replicate b = 1 .. n_rep weighs row i by `w(b, i) = poisson1(u32(b, unit(i)))`, where `u32(b, x)` is the high 32 bits of
  `mix64(mix64(seed + 0x9E3779B97F4A7C15 * b) ^ x)`, `mix64` is the splitmix64 finaliser (oracle/rng.py:80-85) and
  `poisson1(u)` is the number of k with `u >= THR[k]`, `THR[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)`.  Replicate 0 is
  the unweighted statistic: w(0, .) = 1.
- `P[b]`, `N[b]`: the weight of the positives, of the negatives.  `T[b] = sum_{positive i} w (Cn(rs(i)) + Cn(i))` with
  `Cn(j)` the weight of negatives at sorted positions < j and `rs(i)` the first position of i's run of equal keys: it is
  `2 * #{s_p > s_n} + #{s_p == s_n}` with every pair counted `w_p * w_n` times.  Slot 0 is exact.metrics_host's (T, P, N).
- `AUC_b = T[b] / (2 * P[b] * N[b])` in fp64; a replicate with `P[b] * N[b] == 0` is invalid: reported, not hidden.

Why Poisson weights and not multinomial draws: a row's weight is a pure function of (seed, b, unit), so the device needs
neither a state nor a stored draw and the host restates it bit for bit; Poisson(1) weights are the large-n limit of the
multinomial's counts.  The device (csrc/bootstrap_kernels.hip) sorts with exact_kernels.hip's radix sort and scans tiles;
`replicates_host` uses a stable `np.argsort` and `np.cumsum` -- two algorithms for the same integers.
"""
import decimal

import numpy as np

from . import exact

# include/mamdr_hip.h: MAMDR_BOOT_THR, MAMDR_BOOT_WMAX (thresholds() recomputes them)
THR = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
       4294966817, 4294967252, 4294967292, 4294967295)
WMAX = len(THR)
MAX_ROWS = 2 ** 27      # n < 2^27: the weights of a replicate add up to S < 2^27 * 13 < 2^31, so 2 P N <= S^2 / 2 < 2^61
MAX_REP = 65535
# csrc/mamdr_kernels.h: the tile, group and workspace constants of the device chain (tests read them here)
TILE = 1024             # BOOT_TILE: sorted positions per wave of k_boot_parts / k_boot_T
GROUP = 16              # BOOT_GROUP: replicates per workgroup
PART_WORDS = 1 << 24    # BOOT_PART_WORDS: 32-bit words of per-(tile, replicate) partials at a time; beyond it, chunks
GOLDEN = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def thresholds(digits=60):
    """THR recomputed with `decimal` at `digits` significant digits: floor(2^32 * CDF_Poisson(1)(k)) for k = 0, 1, ... up to
    and including the first that reaches 2^32 - 1."""
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        e1 = decimal.Decimal(-1).exp()
        cdf, fact, out, k = decimal.Decimal(0), decimal.Decimal(1), [], 0
        while True:
            if k:
                fact *= k
            cdf += e1 / fact
            out.append(int((cdf * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
            if out[-1] >= 2 ** 32 - 1:
                return tuple(out)
            k += 1


def mix64(z):
    """the splitmix64 finaliser on uint64 arrays (or one python integer), mod 2^64."""
    if isinstance(z, int):
        z &= _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def u32(seed, b, x):
    """high 32 bits of mix64(mix64(seed + GOLDEN * b) ^ x) for a uint32 array x -> uint32 array."""
    hb = mix64((int(seed) + GOLDEN * int(b)) & _M64)
    x = np.asarray(x).astype(np.uint32).astype(np.uint64)
    return (mix64(np.uint64(hb) ^ x) >> np.uint64(32)).astype(np.uint32)


def poisson1(u):
    """the number of k with u >= THR[k]."""
    return np.searchsorted(np.asarray(THR, np.uint32), np.asarray(u, np.uint32), side="right").astype(np.int64)


def units_of(unit, n):
    """the uint32 unit of every row: the given column through the (uint32) cast, else the row index."""
    if unit is None:
        return np.arange(n, dtype=np.uint32)
    unit = np.asarray(unit).ravel()
    if unit.shape[0] != n:
        raise ValueError("bootstrap: %d units for %d rows" % (unit.shape[0], n))
    return unit.astype(np.int32).view(np.uint32)


def weights(seed, b, units):
    """int64 [len(units)]: w(b, .) of the definition for the uint32 units (replicate 0: ones)."""
    units = np.asarray(units)
    if int(b) == 0:
        return np.ones(units.shape, np.int64)
    return poisson1(u32(seed, b, units))


def check_sizes(n, n_rep):
    if not 0 <= n < MAX_ROWS:
        raise ValueError("bootstrap: %d rows outside [0, 2^27)" % n)
    if not 0 <= int(n_rep) <= MAX_REP:
        raise ValueError("bootstrap: n_rep %d outside 0..%d" % (n_rep, MAX_REP))


def replicates_host(pred, label, n_rep, seed, unit=None):
    """the definition on the host -> (T uint64, P int64, N int64), arrays [n_rep + 1]."""
    comp = exact.composites(pred, label)
    n, n_rep = int(comp.shape[0]), int(n_rep)
    check_sizes(n, n_rep)
    T, P, N = np.zeros(n_rep + 1, np.uint64), np.zeros(n_rep + 1, np.int64), np.zeros(n_rep + 1, np.int64)
    if n == 0:
        return T, P, N
    units = units_of(unit, n)
    order = np.argsort(comp, kind="stable")          # (key, positive), rows ascending inside equal pairs
    comp, units = comp[order], units[order]
    key = comp >> np.uint64(1)
    positive = (comp & np.uint64(1)).astype(bool)
    start = np.concatenate([[True], key[1:] != key[:-1]])
    rs = np.maximum.accumulate(np.where(start, np.arange(n, dtype=np.int64), 0))
    assert n * WMAX < 2 ** 31                        # every sum below stays inside int64 (MAX_ROWS's derivation)
    for b in range(n_rep + 1):
        w = weights(seed, b, units)
        wn = np.where(positive, 0, w)
        cn = np.cumsum(wn, dtype=np.int64) - wn      # the weight of negatives at positions < i
        P[b] = int(w[positive].sum())
        N[b] = int(wn.sum())
        T[b] = int((w * (cn[rs] + cn))[positive].sum())
    return T, P, N


def aucs(T, P, N):
    """fp64 [n_rep + 1]: T / (2 P N) per slot, correctly rounded from the integers; NaN where P * N == 0."""
    out = np.full(len(T), np.nan, np.float64)
    for b, (t, p, n) in enumerate(zip(np.asarray(T).tolist(), np.asarray(P).tolist(), np.asarray(N).tolist())):
        if p > 0 and n > 0:
            out[b] = int(t) / (2 * int(p) * int(n))
    return out


def _interval(values, level):
    """(se, ci_lo, ci_hi) of the valid replicates: standard deviation with ddof 1 and the percentile interval (numpy's
    default linear interpolation); zeros with fewer than 2 of them."""
    if not 0.0 < level < 1.0:
        raise ValueError("bootstrap: level %r outside (0, 1)" % (level,))
    if values.shape[0] < 2:
        return 0.0, 0.0, 0.0
    lo, hi = np.percentile(values, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
    return float(np.std(values, ddof=1)), float(lo), float(hi)


def finish(T, P, N, level=0.95):
    """the report of one split from the outputs of mamdr_auc_bootstrap / replicates_host: auc (slot 0; 0.0 with valid = 0
    when P * N == 0, exact.finish's convention), n_rep, n_valid (the replicates 1 .. n_rep with P * N > 0), se, ci_lo,
    ci_hi (of those; 0.0 with fewer than 2 of them, n_valid telling why -- recommend.ranking_metrics' convention), level,
    replicates (fp64 [n_rep + 1], slot 0 the point estimate, NaN where invalid) and the integer arrays T, P, N."""
    T = np.asarray(T).ravel().astype(np.uint64)
    P, N = np.asarray(P, np.int64).ravel(), np.asarray(N, np.int64).ravel()
    if not (T.shape == P.shape == N.shape and T.shape[0] >= 1):
        raise ValueError("bootstrap: T, P and N must be arrays of one length n_rep + 1")
    rep = aucs(T, P, N)
    drawn = rep[1:][~np.isnan(rep[1:])]
    se, lo, hi = _interval(drawn, level)
    valid = int(not np.isnan(rep[0]))
    return {"auc": float(rep[0]) if valid else 0.0, "valid": valid, "n_rep": int(T.shape[0] - 1),
            "n_valid": int(drawn.shape[0]), "se": se, "ci_lo": lo, "ci_hi": hi, "level": float(level), "replicates": rep,
            "T": T, "P": P, "N": N}


def paired(rep_a, rep_b, level=0.95):
    """two calls made with the same seed, labels and units (their replicates are paired: every row had the same weights)
    -> the same summary of rep_a - rep_b over the replicates valid in both: diff (slot 0's; 0.0 with valid = 0 when either
    is invalid), n_rep, n_valid, se, ci_lo, ci_hi, level, replicates (the differences, NaN where either is invalid).
    rep_a / rep_b: finish's reports or their `replicates` arrays."""
    a, b = [np.asarray(r["replicates"] if isinstance(r, dict) else r, np.float64).ravel() for r in (rep_a, rep_b)]
    if a.shape != b.shape or a.shape[0] < 1:
        raise ValueError("bootstrap: paired replicates must be two arrays of one length n_rep + 1")
    diff = a - b
    drawn = diff[1:][~np.isnan(diff[1:])]
    se, lo, hi = _interval(drawn, level)
    valid = int(not np.isnan(diff[0]))
    return {"diff": float(diff[0]) if valid else 0.0, "valid": valid, "n_rep": int(a.shape[0] - 1),
            "n_valid": int(drawn.shape[0]), "se": se, "ci_lo": lo, "ci_hi": hi, "level": float(level), "replicates": diff}


def summarise(reports):
    """{domain: report} -> what result.json carries: {"domain_auc_ci_lo", "domain_auc_ci_hi", "domain_auc_se",
    "domain_auc_ci_valid"} -> {domain: value}; the last is n_valid."""
    return {"domain_auc_ci_lo": {d: r["ci_lo"] for d, r in reports.items()},
            "domain_auc_ci_hi": {d: r["ci_hi"] for d, r in reports.items()},
            "domain_auc_se": {d: r["se"] for d, r in reports.items()},
            "domain_auc_ci_valid": {d: r["n_valid"] for d, r in reports.items()}}
