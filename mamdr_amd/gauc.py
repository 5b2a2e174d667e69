"""Per-user grouped AUC (GAUC, Zhou et al., DIN, KDD 2018), host side: the grouping plan the device call needs, the
documented host definition, and the report.  Pure numpy.  The reference has no counterpart: its pipeline ends at one
500-threshold AUC per domain (base_model.py:111-144).

Definition.  For one split of one domain, group the rows by `uid`.  For a group u with r_u rows, P_u of them positive
(`label != 0`, as the eval histogram classifies) and N_u negative:

- `T_u = 2 * #{(p, n): s_p > s_n} + #{(p, n): s_p == s_n}` over positive rows p and negative rows n of the group.  It is
  an integer.  `AUC_u = T_u / (2 * P_u * N_u)`, the Mann-Whitney statistic with ties counted half.
- Predictions compare as IEEE floats, with three rules.  -0 equals +0.  A NaN is below every number, -inf included.
  Two NaNs are equal.
- A group is valid when `P_u > 0` and `N_u > 0`.
- `GAUC = sum_valid r_u * AUC_u / sum_valid r_u`.
- Report beside it `n_groups`, `n_valid` and `rows_valid = sum_valid r_u`.
- When no group is valid, GAUC is reported as 0.0 with `n_valid = 0`.  This is the convention of
  `recommend.ranking_metrics`.

The device (csrc/gauc_kernels.hip, `mamdr_group_auc`) counts pairs; `group_auc_host` sorts and sums mid-ranks -- two
algorithms for the same integers.
"""
import collections

import numpy as np

SMALL = 64        # groups of up to this many rows need no tile (csrc/mamdr_kernels.h: GAUC_SMALL)
TILE = 256        # positions per tile of a larger group (GAUC_TILE)

GroupPlan = collections.namedtuple("GroupPlan", "order group_off tile_group tile_first")


def group_plan(uid):
    """the grouping of one split for mamdr_group_auc -> GroupPlan(order, group_off, tile_group, tile_first):
    order [n] int32: row indices sorted by uid, stable (rows of one user keep their file order); group_off [G + 1] int64:
    group g -- the g-th smallest uid -- is order[group_off[g] : group_off[g + 1]]; every group of more than 64 rows is cut
    into tiles of up to 256 consecutive positions: tile t belongs to group tile_group[t] (int32) and starts at position
    tile_first[t] (int64) of `order`."""
    uid = np.asarray(uid).ravel()
    n = int(uid.shape[0])
    if n >= 2 ** 31:
        raise ValueError("group_plan: %d rows (row indices are int32)" % n)
    order = np.argsort(uid, kind="stable").astype(np.int32)
    su = uid[order]
    starts = np.flatnonzero(np.concatenate([[True], su[1:] != su[:-1]])) if n else np.zeros(0, np.int64)
    group_off = np.concatenate([starts, [n]]).astype(np.int64)
    sizes = np.diff(group_off)
    big = np.flatnonzero(sizes > SMALL)
    n_tiles = -(-sizes[big] // TILE)
    tile_group = np.repeat(big, n_tiles).astype(np.int32)
    # tile k of its group starts 256 k positions behind the group's first
    k = np.arange(int(n_tiles.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_tiles) - n_tiles, n_tiles)
    tile_first = (group_off[tile_group] + TILE * k).astype(np.int64)
    return GroupPlan(order, group_off, tile_group, tile_first)


def ordered_key(pred):
    """uint32 keys that compare as the definition compares predictions: NaN lowest and equal to NaN, -0 equal to +0."""
    p = np.ascontiguousarray(pred, np.float32).ravel()
    b = p.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[p == 0] = 0x80000000
    key[np.isnan(p)] = 0
    return key


def finish(num, rows_valid, n_valid, n_groups):
    """the report of one split from the four results of mamdr_group_auc / group_auc_host's sums."""
    n_valid, rows_valid = int(n_valid), int(rows_valid)
    return {"gauc": float(num) / rows_valid if n_valid else 0.0, "n_groups": int(n_groups), "n_valid": n_valid,
            "rows_valid": rows_valid}


def group_auc_host(pred, label, uid, want_groups=False):
    """the definition on the host -> finish(...)'s report; want_groups adds, per group in ascending uid order (the order of
    group_plan's groups), "uid", "rows" (r_u, int64), "T" (uint64) and "P" (uint32).

    Rank-sum form, in integers.  Sort the rows by (uid, key).  Inside a group, a row with L rows strictly below it and E
    rows equal to it (itself included) has the mid-rank L + (E + 1) / 2.  Summed over the group's positives, 2 L + E counts
    every (positive, negative) pair as T_u does, and every pair of positives, a positive with itself included, once in
    each direction: P_u^2 in all.  So T_u = sum_pos (2 L + E) - P_u^2.  No Python loop over users."""
    uid = np.asarray(uid).ravel()
    n = int(uid.shape[0])
    key = ordered_key(pred)
    positive = np.asarray(label).ravel() != 0
    if key.shape[0] != n or positive.shape[0] != n:
        raise ValueError("group_auc_host: pred, label and uid differ in length")
    if n == 0:
        rep = finish(0.0, 0, 0, 0)
        if want_groups:
            rep.update(uid=uid[:0], rows=np.zeros(0, np.int64), T=np.zeros(0, np.uint64), P=np.zeros(0, np.uint32))
        return rep
    order = np.lexsort((key, uid))
    su, sk, sp = uid[order], key[order], positive[order]
    new_group = np.concatenate([[True], su[1:] != su[:-1]])
    new_run = new_group | np.concatenate([[True], sk[1:] != sk[:-1]])          # a run: equal keys of one group
    g_start = np.flatnonzero(new_group)
    run_start = np.flatnonzero(new_run)
    rows = np.diff(np.concatenate([g_start, [n]])).astype(np.int64)
    run_len = np.diff(np.concatenate([run_start, [n]])).astype(np.int64)
    run_of = np.cumsum(new_run) - 1
    group_of = np.cumsum(new_group) - 1
    below = run_start[run_of] - g_start[group_of]                              # L
    twice_rank = np.where(sp, 2 * below + run_len[run_of], 0).astype(np.int64)
    P = np.add.reduceat(sp.astype(np.int64), g_start)
    T = np.add.reduceat(twice_rank, g_start) - P * P
    N = rows - P
    valid = (P > 0) & (N > 0)
    # one division, one multiplication per group, then the sum: the device's terms, bit for bit (its tree adds them in
    # another order; G non-negative terms: within a relative G * 2^-52 of each other)
    terms = rows[valid].astype(np.float64) * (T[valid].astype(np.float64) / (2 * P[valid] * N[valid]).astype(np.float64))
    rep = finish(float(terms.sum()), int(rows[valid].sum()), int(valid.sum()), int(rows.shape[0]))
    if want_groups:
        rep.update(uid=su[g_start], rows=rows, T=T.astype(np.uint64), P=P.astype(np.uint32))
    return rep


def summarise(reports):
    """{domain: report} -> (plain mean of gauc over the domains with a valid user, rows_valid-weighted mean); both 0.0
    when no domain has one."""
    reps = [r for r in reports.values() if r["n_valid"] > 0]
    if not reps:
        return 0.0, 0.0
    rows = sum(r["rows_valid"] for r in reps)
    return sum(r["gauc"] for r in reps) / len(reps), sum(r["rows_valid"] * r["gauc"] for r in reps) / rows
