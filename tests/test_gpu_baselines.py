"""The baselines' four device calls through raw ctypes against their host definitions (mamdr_amd/baselines.py):

- mamdr_item_cooc equals cooc_host exactly (integers) over the size ladder, a history longer than a workgroup, the hot pair,
  a planted position outside the catalogue, on a buffer pre-filled with 0xff between guard words;
- mamdr_history_scores byte for byte against the fp32 replay on the same counts, within (L + 8) 2^-24 of the float64 form,
  and the same rows wherever a query stands, however the loads are shaped;
- mamdr_rank_scores / mamdr_topk_scores exactly against rank_scores_host / topk_scores_host on the same fp32 scores, the
  rank <-> position link, and the same results from permuted columns;
- baselines.rank / report on a tower of each engine, and run.py with and without --baselines."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import _lib                      # noqa: E402
from mamdr_amd import baselines as bl           # noqa: E402
from mamdr_amd import recommend as rec          # noqa: E402
from test_gpu_knn import build, digest, train_pass                                         # noqa: E402
from test_gpu_list_metrics import dev as _dev, need_gpu, ptr, small_config, stream        # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
M_LADDER = (1, 2, 63, 64, 65, 130, 257)
GUARD = 64                                      # int32 words on either side of an output


def dev(a):
    return _dev(np.array(a))


def guarded(n, dtype, fill):
    """a device buffer of n elements between two runs of GUARD words, everything pre-filled -> (whole, the inner view)."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, fill):
    w = whole.cpu()
    return bool((w[:GUARD] == fill).all()) and bool((w[-GUARD:] == fill).all())


def cooc_dev(off, pos, m):
    """mamdr_item_cooc -> (uint32 [m, m] on the host, the device tensor int32 [m, m]); the buffer starts as 0xff bytes."""
    lib = _lib.load()
    d_off, d_pos = dev(np.asarray(off, np.int64)), (dev(np.asarray(pos, np.int32)) if len(pos) else None)
    whole, inner = guarded(m * m, torch.int32, -1)
    _lib.check(lib.mamdr_item_cooc(ptr(d_off), ptr(d_pos), len(pos), len(off) - 1, m, ptr(inner), stream()))
    assert guards_intact(whole, -1)
    return inner.cpu().numpy().view(np.uint32).reshape(m, m), inner.view(m, m)


def scores_dev(d_cooc, m, off, pos, queries, shrink, shift=0):
    """mamdr_history_scores -> fp32 [Q, m] on the host; the output starts as NaN between guard words.  shift: floats the
    output starts beyond a 16-byte boundary (the 4-byte load path)."""
    lib = _lib.load()
    q = np.asarray(queries, np.int32)
    d_off, d_pos, d_q = dev(np.asarray(off, np.int64)), (dev(np.asarray(pos, np.int32)) if len(pos) else None), dev(q)
    whole, inner = guarded(q.size * m + shift, torch.float32, float("nan"))
    inner = inner[shift:]
    _lib.check(lib.mamdr_history_scores(ptr(d_cooc), m, ptr(d_off), ptr(d_pos), len(pos), len(off) - 1, ptr(d_q), q.size,
                                        float(shrink), ptr(inner), stream()))
    w = whole.cpu().numpy()
    assert np.isnan(w[:GUARD + shift]).all() and np.isnan(w[-GUARD:]).all()
    return inner.cpu().numpy().reshape(q.size, m)


def rank_dev(scores, stride, n_query, n_cand, cand, excl, tgt):
    """mamdr_rank_scores -> (ranks, live, scores) on the host; the outputs start as garbage between guard words."""
    lib = _lib.load()
    d_s, d_c = dev(np.asarray(scores, F32)), (dev(np.asarray(cand, np.int32)) if cand is not None else None)
    d_eo, d_ei = (dev(excl[0]), dev(excl[1] if excl[1].size else np.zeros(1, np.int32))) if excl is not None else (None, None)
    n_tgt = int(tgt[1].size)
    d_to, d_ti = dev(tgt[0]), (dev(tgt[1]) if n_tgt else None)
    w_r, ranks = guarded(n_tgt, torch.int32, -7)
    w_l, live = guarded(n_query, torch.int32, -7)
    w_s, out = guarded(n_tgt, torch.float32, 7.0)
    _lib.check(lib.mamdr_rank_scores(ptr(d_s), stride, n_query, ptr(d_c), n_cand, ptr(d_eo), ptr(d_ei), ptr(d_to), ptr(d_ti), n_tgt,
                                     ptr(ranks if n_tgt else None), ptr(out if n_tgt else None), ptr(live), stream()))
    assert guards_intact(w_r, -7) and guards_intact(w_l, -7) and guards_intact(w_s, 7.0)
    return ranks.cpu().numpy(), live.cpu().numpy(), out.cpu().numpy()


def topk_dev(scores, stride, n_query, n_cand, cand, excl, k):
    lib = _lib.load()
    d_s, d_c = dev(np.asarray(scores, F32)), (dev(np.asarray(cand, np.int32)) if cand is not None else None)
    d_eo, d_ei = (dev(excl[0]), dev(excl[1] if excl[1].size else np.zeros(1, np.int32))) if excl is not None else (None, None)
    w_i, ids = guarded(n_query * k, torch.int32, -7)
    w_s, out = guarded(n_query * k, torch.float32, 7.0)
    _lib.check(lib.mamdr_topk_scores(ptr(d_s), stride, n_query, ptr(d_c), n_cand, ptr(d_eo), ptr(d_ei), k, ptr(ids), ptr(out), stream()))
    assert guards_intact(w_i, -7) and guards_intact(w_s, 7.0)
    return ids.cpu().numpy().reshape(n_query, k), out.cpu().numpy().reshape(n_query, k)


# ------------------------------------------------------------------ fixtures, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def histories(n_user, m, seed=0):
    """random histories whose lengths walk 0, 1, 2, 63, 64, 65 and m (a full row), cut to m -> (off, pos, cooc_host)."""
    rs = np.random.RandomState(1000 * n_user + m + seed)
    lengths = [min(m, (0, 1, 2, 63, 64, 65, m)[(u + seed) % 7]) for u in range(n_user)]
    rows = [np.sort(rs.choice(m, n, replace=False)) for n in lengths]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    pos = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    C = bl.cooc_host(off, pos, m)
    for a in (off, pos, C):
        a.setflags(write=False)
    return off, pos, C


# ------------------------------------------------------------------ 1. mamdr_item_cooc
@pytest.mark.parametrize("n_user", [1, 2, 65, 300])
def test_cooc_equals_the_host_definition(n_user):
    need_gpu()
    for m in M_LADDER:
        off, pos, want = histories(n_user, m)
        got, _ = cooc_dev(off, pos, m)
        assert np.array_equal(got, want), (n_user, m)
        assert np.array_equal(got, got.T)
        held = np.bincount(pos, minlength=m)                 # the diagonal: how many histories hold the item
        assert np.array_equal(np.diagonal(got), held)
        assert int(got.sum()) == bl.pair_counts(off)


def test_cooc_a_history_longer_than_a_workgroup_the_hot_pair_and_a_foreign_position():
    need_gpu()
    # one user, L = 300 at m = 320: the pair loops stride over the history
    h = np.sort(np.random.RandomState(3).choice(320, 300, replace=False)).astype(np.int32)
    got, _ = cooc_dev([0, 300], h, 320)
    assert np.array_equal(got, bl.cooc_host([0, 300], h, 320)) and int(got.sum()) == 300 * 300
    assert got[h[0], h[299]] == 1 and got[h[299], h[0]] == 1 and got[h[150], h[150]] == 1
    # 300 users that all hold {0, 1}: every add of the call lands on four words
    off = np.arange(301, dtype=np.int64) * 2
    got, _ = cooc_dev(off, np.tile([0, 1], 300), 5)
    assert got[:2, :2].tolist() == [[300, 300], [300, 300]] and int(got.sum()) == 1200
    # a position outside [0, m) planted in one history counts nowhere and corrupts nothing (the guards are checked in cooc_dev)
    off, pos, _ = histories(65, 130)
    bad = np.array(pos)
    at = int(off[5])                                          # user 5 has 65 entries
    for value in (130, -1, 2 ** 31 - 1):
        bad[at + 7] = value
        got, _ = cooc_dev(off, bad, 130)
        assert np.array_equal(got, bl.cooc_host(off, bad, 130))
        assert int(got.sum()) == bl.pair_counts(off) - (65 * 65 - 64 * 64)
    # offsets beyond nnz and below their start are clamped: wrong numbers perhaps, the host definition's, and no stray write
    wild = np.array([0, 40, 10 ** 12, 20, -5, 60], np.int64)
    got, _ = cooc_dev(wild, pos[:50], 130)
    assert np.array_equal(got, bl.cooc_host(wild, pos[:50], 130))
    # nobody holds anything: the call still zeroes the buffer
    got, _ = cooc_dev([0, 0, 0], [], 7)
    assert not got.any()


# ------------------------------------------------------------------ 2. mamdr_history_scores
@pytest.mark.parametrize("shrink", [0.0, 1.0, 10.0])
def test_history_scores_are_the_replays_bytes_and_within_the_bound(shrink):
    need_gpu()
    for m in M_LADDER:                                        # (1, 2, 63, 65, 130, 257: no multiple of 4 -> 4-byte loads; 64: 16-byte)
        off, pos, C = histories(65, m)
        _, d_cooc = cooc_dev(off, pos, m)
        q = np.arange(65)
        got = scores_dev(d_cooc, m, off, pos, q, shrink)
        want = bl.history_scores_host(C, off, pos, q, shrink)
        assert got.tobytes() == want.tobytes(), (shrink, m)
        ref = bl.history_scores_host(C, off, pos, q, shrink, dtype=np.float64)
        bound = np.array([bl.error_bound(n) for n in np.diff(off)])[:, None] * ref
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (shrink, m)
        assert not got[np.diff(off) == 0].view(np.uint32).any()          # an empty history: all +0.0f bits
    for m in (128, 1028):                                     # 16-byte loads, more than one column tile of a query
        off, pos, C = histories(65, m, seed=1)
        _, d_cooc = cooc_dev(off, pos, m)
        got = scores_dev(d_cooc, m, off, pos, np.arange(65), shrink)
        assert got.tobytes() == bl.history_scores_host(C, off, pos, np.arange(65), shrink).tobytes(), (shrink, m)


def test_a_row_is_the_same_bits_wherever_the_query_stands():
    need_gpu()
    for m in (130, 256):
        off, pos, C = histories(300, m)
        _, d_cooc = cooc_dev(off, pos, m)
        rs = np.random.RandomState(m)
        q257 = rs.randint(0, 300, 257)
        base = scores_dev(d_cooc, m, off, pos, q257, 10.0)
        assert base.tobytes() == bl.history_scores_host(C, off, pos, q257, 10.0).tobytes()
        perm = rs.permutation(257)
        assert scores_dev(d_cooc, m, off, pos, q257[perm], 10.0).tobytes() == base[perm].tobytes()
        dup = np.repeat(q257[:2], 2)
        assert scores_dev(d_cooc, m, off, pos, dup, 10.0).tobytes() == np.repeat(base[:2], 2, axis=0).tobytes()
        for i in (0, 1, 100, 256):                            # called one at a time
            assert scores_dev(d_cooc, m, off, pos, q257[i:i + 1], 10.0).tobytes() == base[i:i + 1].tobytes()
        assert scores_dev(d_cooc, m, off, pos, q257[:2], 10.0).tobytes() == base[:2].tobytes()
        # the load shape leaves no trace: an output that starts 4 bytes beyond a 16-byte boundary takes the 4-byte path
        assert scores_dev(d_cooc, m, off, pos, q257[:40], 10.0, shift=1).tobytes() == base[:40].tobytes()
        # a query index of -1 or n_user is no error: all zeros
        edge = scores_dev(d_cooc, m, off, pos, [-1, 300, int(q257[0]), 2 ** 31 - 1], 10.0)
        assert not edge[[0, 1, 3]].view(np.uint32).any() and edge[2].tobytes() == base[0].tobytes()


def test_an_item_nobody_has_scores_zero_at_shrink_zero_and_foreign_positions_are_skipped():
    need_gpu()
    off, pos, _ = histories(65, 63)
    m = 66                                                    # items 63, 64, 65: nobody holds them
    C = bl.cooc_host(off, pos, m)
    _, d_cooc = cooc_dev(off, pos, m)
    got = scores_dev(d_cooc, m, off, pos, np.arange(65), 0.0)
    assert got.tobytes() == bl.history_scores_host(C, off, pos, np.arange(65), 0.0).tobytes()
    assert not got[:, 63:].view(np.uint32).any() and not np.isnan(got).any() and got.max() > 0
    bad = np.array(pos)
    bad[int(off[5]) + 3] = 70
    bad[int(off[4]) + 1] = -2
    got = scores_dev(d_cooc, m, off, bad, np.arange(65), 1.0)
    assert got.tobytes() == bl.history_scores_host(C, off, bad, np.arange(65), 1.0).tobytes()


# ------------------------------------------------------------------ 3. mamdr_rank_scores / mamdr_topk_scores
def csr(lists):
    return rec.exclusion_csr(lists, len(lists))


def score_rows(rs, kind, n_query, n_cand):
    if kind == "random":
        return rs.standard_normal((n_query, n_cand)).astype(F32)
    if kind == "equal":
        return np.full((n_query, n_cand), 0.25, F32)
    if kind == "two":
        return rs.choice(np.array([-1.5, 2.0], F32), (n_query, n_cand))
    s = rs.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 1e-30], F32), (n_query, n_cand))      # "special"
    return s.astype(F32)


def problem(seed, n_query, n_cand, kind, stride_kind, with_cand, excl_kind):
    """-> (the scores as the device reads them, row_stride, the [Q, n_cand] (or [n_cand]) view the host reads, cand, excl, tgt)."""
    rs = np.random.RandomState(seed)
    cand = np.sort(rs.choice(5 * n_cand + 7, n_cand, replace=False)).astype(np.int32) if with_cand else None
    ids = cand if with_cand else np.arange(n_cand, dtype=np.int32)
    if stride_kind == 0:
        flat = score_rows(rs, kind, 1, n_cand)[0]
        view, stride = flat, 0
    else:
        stride = n_cand + (3 if stride_kind == 2 else 0)
        full = score_rows(rs, kind, n_query, stride)
        flat, view = full, full[:, :n_cand]
    foreign = np.setdiff1d(np.arange(ids.max() + 5), ids)[:3] if with_cand else np.array([n_cand, n_cand + 9])
    if excl_kind == "none":
        excl, lists = None, [np.zeros(0, np.int64)] * n_query
    else:
        lists = [ids if excl_kind == "all" else rs.choice(ids, rs.randint(0, n_cand + 1) // 2, replace=False) for _ in range(n_query)]
        if excl_kind == "partial":
            lists[0] = np.zeros(0, np.int64)                                  # an empty list among them
            lists = [np.concatenate([e, foreign[:1]]) for e in lists]         # an excluded id that is no candidate
        excl = csr(lists)
    targets = []
    for q in range(n_query):
        t = [rs.choice(ids, min(n_cand, 3), replace=False), foreign[:2]]       # live or excluded ones, and absent ones
        if len(lists[q]):
            t.append(np.asarray(lists[q])[:2])                                # certainly excluded ones
        targets.append(np.concatenate(t) if q % 5 != 4 else np.zeros(0, np.int64))      # a query without targets
    return flat, stride, view, cand, excl, csr(targets)


CASES = [(1, 1, "random", 1, False, "none"), (2, 63, "equal", 1, True, "partial"), (257, 64, "two", 0, True, "partial"),
         (2, 65, "special", 2, False, "partial"), (257, 129, "random", 2, True, "none"), (2, 1000, "special", 0, False, "all"),
         (257, 1000, "random", 1, True, "partial"), (1, 129, "two", 2, True, "all"), (2, 1000, "equal", 0, True, "partial"),
         (1, 2500, "special", 1, True, "partial")]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_ranks_and_lists_equal_the_host_definitions(case):
    need_gpu()
    n_query, n_cand, kind, stride_kind, with_cand, excl_kind = CASES[case]
    flat, stride, view, cand, excl, tgt = problem(case, n_query, n_cand, kind, stride_kind, with_cand, excl_kind)
    e_off, e_ids = excl if excl is not None else (None, None)
    ranks, live, out = rank_dev(flat, stride, n_query, n_cand, cand, excl, tgt)
    want = bl.rank_scores_host(view, n_query, tgt[0], tgt[1], cand, e_off, e_ids)
    assert np.array_equal(ranks, want[0]) and np.array_equal(live, want[1]) and out.tobytes() == want[2].tobytes()
    assert (ranks == -1).any()
    if excl_kind == "all":
        assert not live.any()
    ids_of = cand if cand is not None else np.arange(n_cand)
    for k in (1, 64, 128):                                    # (n_cand < k among the cases: short lists)
        ids, scores = topk_dev(flat, stride, n_query, n_cand, cand, excl, k)
        w_ids, w_scores = bl.topk_scores_host(view, n_query, k, cand, e_off, e_ids)
        assert np.array_equal(ids, w_ids) and scores.tobytes() == w_scores.tobytes(), k
        assert ((ids >= 0).sum(1) == np.minimum(live, k)).all()
        # the link: a live target sits at position r of the list exactly when its rank is r < k
        for q in range(n_query):
            ex = e_ids[e_off[q]:e_off[q + 1]] if excl is not None else ()
            for j in range(int(tgt[0][q]), int(tgt[0][q + 1])):
                t = tgt[1][j]
                if t in ids_of and t not in ex:
                    assert (ranks[j] < k) == (t in ids[q]) and (ranks[j] >= k or ids[q, ranks[j]] == t)
                else:
                    assert t not in ids[q]


def test_permuted_columns_with_the_candidates_resorted_give_the_same_results():
    need_gpu()
    n_query, n_cand = 33, 300
    flat, stride, view, cand, excl, tgt = problem(77, n_query, n_cand, "two", 1, True, "partial")
    base_r = rank_dev(flat, stride, n_query, n_cand, cand, excl, tgt)
    base_k = topk_dev(flat, stride, n_query, n_cand, cand, excl, 64)
    # the columns and d_cand permuted together and re-sorted by id are the call's input again: the same results
    perm = np.random.RandomState(5).permutation(n_cand)
    order = np.argsort(cand[perm])
    again = np.ascontiguousarray(view[:, perm][:, order])
    assert np.array_equal(cand[perm][order], cand)
    got_r = rank_dev(again, n_cand, n_query, n_cand, cand[perm][order], excl, tgt)
    assert all(np.array_equal(x, y) for x, y in zip(got_r[:2], base_r[:2])) and got_r[2].tobytes() == base_r[2].tobytes()
    got_k = topk_dev(again, n_cand, n_query, n_cand, cand[perm][order], excl, 64)
    assert np.array_equal(got_k[0], base_k[0]) and got_k[1].tobytes() == base_k[1].tobytes()
    # the same (id, score) pairs at OTHER positions: 211 more candidates, excluded for every query, stand between them
    rs = np.random.RandomState(6)
    more = rs.choice(np.setdiff1d(np.arange(cand.max() + 400), np.concatenate([cand, tgt[1], excl[1]])), 211, replace=False)
    wide_cand = np.sort(np.concatenate([cand, more])).astype(np.int32)
    wide = rs.standard_normal((n_query, wide_cand.size)).astype(F32) + 9          # (they would win every rank if they were live)
    wide[:, np.isin(wide_cand, cand)] = view
    wide_excl = csr([np.concatenate([excl[1][excl[0][q]:excl[0][q + 1]], more]) for q in range(n_query)])
    got_r = rank_dev(wide, wide_cand.size, n_query, wide_cand.size, wide_cand, wide_excl, tgt)
    assert all(np.array_equal(x, y) for x, y in zip(got_r[:2], base_r[:2])) and got_r[2].tobytes() == base_r[2].tobytes()
    got_k = topk_dev(wide, wide_cand.size, n_query, wide_cand.size, wide_cand, wide_excl, 64)
    assert np.array_equal(got_k[0], base_k[0]) and got_k[1].tobytes() == base_k[1].tobytes()
    # positions without ids (d_cand null) against the same call with the identity list
    ident = np.arange(n_cand, dtype=np.int32)
    t2 = csr([np.array([0, 5, n_cand - 1, n_cand + 3])] * n_query)
    a = rank_dev(flat, stride, n_query, n_cand, None, None, t2)
    b = rank_dev(flat, stride, n_query, n_cand, ident, None, t2)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2].tobytes() == b[2].tobytes()
    assert np.array_equal(topk_dev(flat, stride, n_query, n_cand, None, None, 128)[0], topk_dev(flat, stride, n_query, n_cand, ident, None, 128)[0])
    assert base_r[1].sum() > 0 and (base_k[0] >= 0).any()


def test_refusals_launch_nothing():
    need_gpu()
    lib = _lib.load()
    off, pos, _ = histories(65, 64)
    d_off, d_pos, d_q = dev(off), dev(pos), dev(np.arange(4, dtype=np.int32))
    cooc = torch.full((64, 64), 7, dtype=torch.int32, device="cuda")
    scores = torch.full((4, 64), 7.0, dtype=torch.float32, device="cuda")
    n = int(pos.size)
    for kw in (dict(m=0), dict(m=65536), dict(n_user=0), dict(nnz=-1)):
        a = dict(dict(nnz=n, n_user=65, m=64), **kw)
        assert lib.mamdr_item_cooc(ptr(d_off), ptr(d_pos), a["nnz"], a["n_user"], a["m"], ptr(cooc), stream()) == _lib.EINVAL, kw
    assert lib.mamdr_item_cooc(C.c_void_p(d_off.data_ptr() + 4), ptr(d_pos), n, 65, 64, ptr(cooc), stream()) == _lib.EINVAL
    for shrink in (-1.0, 2.0 ** 20 + 1, float("nan")):
        assert lib.mamdr_history_scores(ptr(cooc), 64, ptr(d_off), ptr(d_pos), n, 65, ptr(d_q), 4, shrink, ptr(scores), stream()) == _lib.EINVAL
    assert lib.mamdr_history_scores(ptr(cooc), 64, ptr(d_off), ptr(d_pos), n, 1 << 24, ptr(d_q), 4, 1.0, ptr(scores), stream()) == _lib.EINVAL
    ids = torch.full((4, 2), 7, dtype=torch.int32, device="cuda")
    t_off = dev(np.array([0, 1, 1, 1, 1], np.int64))
    for stride in (-1, 1, 63):
        assert lib.mamdr_topk_scores(ptr(scores), stride, 4, None, 64, None, None, 2, ptr(ids), ptr(scores), stream()) == _lib.EINVAL
        assert lib.mamdr_rank_scores(ptr(scores), stride, 4, None, 64, None, None, ptr(t_off), ptr(d_q), 1, ptr(ids), None, ptr(ids),
                                     stream()) == _lib.EINVAL
    for k in (0, 129):
        assert lib.mamdr_topk_scores(ptr(scores), 64, 4, None, 64, None, None, k, ptr(ids), ptr(scores), stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (cooc.cpu() == 7).all() and (scores.cpu() == 7.0).all() and (ids.cpu() == 7).all()          # nothing was written
    assert lib.mamdr_item_cooc(ptr(d_off), ptr(d_pos), n, 65, 64, ptr(cooc), stream()) == _lib.OK


# ------------------------------------------------------------------ 4. model level
def npz_arrays(path):
    with np.load(path) as z:
        return {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}


@pytest.mark.parametrize("kind", ["step", "generic"])
def test_model_baselines_equal_the_host_definitions(tmp_path, capsys, kind):
    need_gpu()
    model, eng = build(tmp_path / "a", kind)
    train_pass(eng)
    before = digest(eng, kind)
    for d in (0, 7):
        for who in bl.WHICH:
            got = bl.rank(model, d, who, 10.0, k=10)
            want = bl.rank_host(model, d, who, 10.0, k=10)
            assert np.array_equal(got["ranks"], want["ranks"]) and np.array_equal(got["live"], want["live"]), (d, who)
            assert np.array_equal(got["top_ids"], want["top_ids"]) and got["top_scores"].tobytes() == want["top_scores"].tobytes()
            assert got["ranks"].dtype == np.int32 and got["ranks"].size == got["ids"].size > 0
            tower = model.rank_eval(d)                        # the same problem, line for line
            for key in ("offsets", "ids", "listed", "live", "users", "catalogue", "n_positives"):
                assert np.array_equal(got[key], tower[key]), (d, who, key)
            few = bl.rank(model, d, who, 10.0, k=10, block=17)          # the block count leaves no trace
            assert few["ranks"].tobytes() == got["ranks"].tobytes() and few["top_ids"].tobytes() == got["top_ids"].tobytes()
            assert few["top_scores"].tobytes() == got["top_scores"].tobytes()
    out = str(tmp_path / "base.npz")
    path, reports = bl.report(model, [10, 50], 10, out, shrink=10.0, max_items=16384)
    assert path == out and sorted(reports) == list(range(10))
    with np.load(out) as z:
        assert z["domains"].tolist() == list(range(10)) and not z["skipped"].any() and z["ks"].tolist() == [10, 50]
        for d in (0, 7):
            for who in bl.WHICH:
                assert np.array_equal(z["ranks_%s_%d" % (who, d)], bl.rank_host(model, d, who, 10.0)["ranks"])
            assert z["m"][d] == model._retrieval_problem(d, None, True)[0].size
        for key in ("mrr_pop", "mrr_itemknn", "ndcg_at_10_pop", "recall_at_50_itemknn", "overlap_pop", "overlap_itemknn", "n_cold"):
            assert z[key].shape == (10,) and np.all(np.isfinite(z[key])), key
    head = bl.headline(reports, 10.0)
    assert head["baselines_shrink"] == 10.0 and head["baselines_skipped"] == [] and len(head["domain_mrr_itemknn"]) == 10
    assert set(head["domain_overlap_pop"]) == set(head["domain_cold_users"]) == {str(d) for d in range(10)}
    text = capsys.readouterr().out
    assert text.count(": tower ") == text.count(": pop ") == text.count(": itemknn ") == text.count(": overlap ") == 10
    print(text[text.index("Baselines under"):])
    assert digest(eng, kind) == before                       # the calls read state only
    eng.close()


def run_main(tmp_path, **train):
    from mamdr_amd import cli
    cfg = small_config(tmp_path, "mlp_meta_mamdr", False)
    cfg["train"].update(rank_eval=[10, 50], **train)
    built = []
    cli.main(cfg, on_model=built.append, recommend=10)
    model = built[0]
    rdir = [os.path.join(model.result_path, f) for f in os.listdir(model.result_path) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        return model, f.read()


def test_run_config_with_and_without_baselines(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 MAMDR config, shrunk: without the flag the module is never imported and the
    files are what they are with it, the flag's own keys and file aside."""
    need_gpu()
    kept = {name: sys.modules.pop(name) for name in list(sys.modules) if name == "mamdr_amd.baselines"}
    try:
        plain, plain_json = run_main(tmp_path / "a")
        assert "mamdr_amd.baselines" not in sys.modules
    finally:
        sys.modules.update(kept)
    assert "Baselines" not in capsys.readouterr().out
    assert sorted(f for f in os.listdir(plain.result_path) if f.endswith(".npz")) == ["rank_eval.npz", "recommend_top10.npz"]
    model, with_json = run_main(tmp_path / "b", baselines=10.0)
    text = capsys.readouterr().out
    result = json.loads(with_json)
    extra = bl.headline({d: {"m": 0, "n_cold": 0, "skipped": False, "pop": None, "itemknn": None} for d in range(10)}, 10.0)
    ours = [k for k in result if k in extra or k.endswith("_pop") or k.endswith("_itemknn")]
    assert json.dumps({k: v for k, v in result.items() if k not in ours}) == plain_json
    assert npz_arrays(os.path.join(model.result_path, "rank_eval.npz")) == npz_arrays(os.path.join(plain.result_path, "rank_eval.npz"))
    assert npz_arrays(os.path.join(model.result_path, "recommend_top10.npz")) == npz_arrays(os.path.join(plain.result_path, "recommend_top10.npz"))
    with np.load(os.path.join(model.result_path, "baselines.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and float(z["shrink"]) == 10.0 and int(z["k_lists"]) == 10
        for fig in bl.figures([10, 50]):
            for who in bl.WHICH:
                assert result["domain_%s_%s" % (fig, who)]["3"] == float(z["%s_%s" % (fig, who)][3])
                assert result["avg_%s_%s" % (fig, who)] == pytest.approx(float(np.mean(z["%s_%s" % (fig, who)])))
        assert result["domain_overlap_itemknn"]["6"] == float(z["overlap_itemknn"][6])
        assert result["domain_cold_users"]["2"] == int(z["n_cold"][2]) and result["baselines_skipped"] == []
        assert np.array_equal(z["ranks_pop_4"], bl.rank_host(model, 4, "pop")["ranks"])
    assert result["baselines_shrink"] == 10.0
    assert text.count(": itemknn ") == 10 and text.index("Ranks written to") < text.index("Baselines under")
    print(text[text.index("Baselines under"):])
