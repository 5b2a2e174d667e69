"""MostPopular / ItemKNN baselines and ranking from a score matrix, host side (no GPU): the four C declarations, bindings and
exports, the refusals that need no device, the host definitions (`baselines.cooc_host`, `history_scores_host`,
`rank_scores_host`, `topk_scores_host`) on hand-worked cases, the fp32 replay against its float64 form within the derived
bound, `baselines.histories` on a tiny dataset, the command line, and `run.py --rank-eval --baselines` end to end over a CPU
stand-in whose four calls are the host definitions."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import _lib, cli                     # noqa: E402
from mamdr_amd import baselines as bl               # noqa: E402
from mamdr_amd import list_metrics as lm            # noqa: E402
from mamdr_amd import recommend as rec              # noqa: E402
from test_rank_host import RankEngine               # noqa: E402
from test_recommend_host import RecommendingEngine, patch_emb_dim, tiny_config      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
HIST = ["const int64_t* d_hist_off", "const int32_t* d_hist_pos", "int64_t nnz", "int32_t n_user"]
SCORES = ["const float* d_scores", "int64_t row_stride", "int32_t n_query", "const int32_t* d_cand", "int64_t n_cand",
          "const int64_t* d_excl_off", "const int32_t* d_excl_ids"]
DECLARED = {
    "mamdr_item_cooc": HIST + ["int32_t m", "uint32_t* d_cooc", "void* stream"],
    "mamdr_history_scores": ["const uint32_t* d_cooc", "int32_t m"] + HIST + ["const int32_t* d_query", "int32_t n_query",
                                                                             "float shrink", "float* d_scores", "void* stream"],
    "mamdr_rank_scores": SCORES + ["const int64_t* d_tgt_off", "const int32_t* d_tgt_ids", "int64_t n_tgt", "int32_t* d_rank_out",
                                   "float* d_score_out", "int32_t* d_live_out", "void* stream"],
    "mamdr_topk_scores": SCORES + ["int32_t k", "int32_t* d_ids_out", "float* d_scores_out", "void* stream"],
}


# ------------------------------------------------------------------ C ABI
def test_the_four_calls_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    for name, args in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/mamdr_hip.h" % name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == args
        assert hasattr(_lib.load(), name)
        want = [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in args]
        assert _lib.SIGNATURES[name] == (C.c_int, want), name
    assert header.index("mamdr_row_neighbours_bounded") < header.index("mamdr_item_cooc") < header.index("mamdr_interp")
    assert re.search(r"#define\s+MAMDR_SCORES_MAX_K\s+128\b", header) and _lib.SCORES_MAX_K == bl.MAX_K == 128
    assert _lib.COOC_MAX_ITEMS == bl.MAX_ITEMS == 65535
    assert "NO REFERENCE COUNTERPART" in text[:text.index("int mamdr_item_cooc")].rsplit("/*", 1)[1]
    # new entry points only: the version stays
    assert _lib.ABI_VERSION == 19 and _lib.load().mamdr_abi_version() == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)


P = C.c_void_p(1 << 20)                 # an aligned non-null address: a refusal never dereferences it
ODD2, ODD4 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)


def refused(code, word):
    assert code == _lib.EINVAL, word
    assert word in _lib.load().mamdr_last_error(), (word, _lib.load().mamdr_last_error())


def test_cooc_and_history_scores_refuse_bad_arguments_without_a_device():
    lib = _lib.load()

    def cooc(off=P, pos=P, nnz=4, n_user=2, m=3, out=P):
        return lib.mamdr_item_cooc(off, pos, nnz, n_user, m, out, None)

    def hist(cooc_=P, m=3, off=P, pos=P, nnz=4, n_user=2, query=P, n_query=2, shrink=1.0, out=P):
        return lib.mamdr_history_scores(cooc_, m, off, pos, nnz, n_user, query, n_query, shrink, out, None)
    for call, name in ((cooc, b"mamdr_item_cooc:"), (hist, b"mamdr_history_scores:")):
        for kw, word in ((dict(off=None), b"null"), (dict(pos=None), b"null d_hist_pos"), (dict(out=None), b"null"),
                         (dict(off=ODD4), b"aligned"), (dict(pos=ODD2), b"aligned"), (dict(out=ODD2), b"aligned"),
                         (dict(nnz=-1), b"nnz -1"), (dict(m=0), b"m 0"), (dict(m=-3), b"m -3"), (dict(m=65536), b"m 65536"),
                         (dict(n_user=0), b"n_user 0"), (dict(n_user=-1), b"n_user -1")):
            refused(call(**kw), word)
            assert name in lib.mamdr_last_error()
    assert cooc(pos=None, nnz=0, out=None) == _lib.EINVAL          # (an empty history list is fine; a null output is not)
    for kw, word in ((dict(cooc_=None), b"null"), (dict(query=None), b"null"), (dict(cooc_=ODD2), b"aligned"),
                     (dict(query=ODD2), b"aligned"), (dict(n_user=1 << 24), b"n_user 16777216"),
                     (dict(n_query=0), b"n_query 0"), (dict(n_query=-5), b"n_query -5"),
                     (dict(shrink=-1.0), b"shrink -1"), (dict(shrink=2.0 ** 20 + 1), b"shrink 1.04858e+06"),
                     (dict(shrink=float("nan")), b"shrink nan"), (dict(shrink=float("inf")), b"shrink inf")):
        refused(hist(**kw), word)
    with pytest.raises(_lib.MamdrError):
        _lib.check(hist(shrink=-1.0))


def test_rank_and_topk_scores_refuse_bad_arguments_without_a_device():
    lib = _lib.load()

    def rank(scores=P, stride=8, n_query=2, cand=P, n_cand=8, eoff=P, eids=P, toff=P, tids=P, n_tgt=3, ranks=P, sout=P, live=P):
        return lib.mamdr_rank_scores(scores, stride, n_query, cand, n_cand, eoff, eids, toff, tids, n_tgt, ranks, sout, live, None)

    def topk(scores=P, stride=8, n_query=2, cand=P, n_cand=8, eoff=P, eids=P, k=4, ids=P, out=P):
        return lib.mamdr_topk_scores(scores, stride, n_query, cand, n_cand, eoff, eids, k, ids, out, None)
    shared = ((dict(scores=None), b"null d_scores"), (dict(scores=ODD2), b"aligned"), (dict(cand=ODD2), b"aligned"),
              (dict(eoff=ODD4), b"aligned"), (dict(eids=ODD2), b"aligned"), (dict(eoff=None), b"both"), (dict(eids=None), b"both"),
              (dict(n_query=0), b"n_query 0"), (dict(n_query=-1), b"n_query -1"), (dict(n_cand=0), b"n_cand 0"),
              (dict(n_cand=2 ** 31), b"n_cand 2147483648"), (dict(stride=-1), b"row_stride -1"), (dict(stride=7), b"row_stride 7"),
              (dict(stride=1), b"row_stride 1"))
    for call, name in ((rank, b"mamdr_rank_scores:"), (topk, b"mamdr_topk_scores:")):
        for kw, word in shared:
            refused(call(**kw), word)
            assert name in lib.mamdr_last_error()
    for kw, word in ((dict(toff=None), b"null"), (dict(live=None), b"null"), (dict(tids=None), b"null"), (dict(ranks=None), b"null"),
                     (dict(toff=ODD4), b"aligned"), (dict(tids=ODD2), b"aligned"), (dict(ranks=ODD2), b"aligned"),
                     (dict(sout=ODD2), b"aligned"), (dict(live=ODD2), b"aligned"), (dict(n_tgt=-1), b"n_tgt -1")):
        refused(rank(**kw), word)
    for kw, word in ((dict(ids=None), b"null"), (dict(out=None), b"null"), (dict(ids=ODD2), b"aligned"), (dict(out=ODD2), b"aligned"),
                     (dict(k=0), b"k 0"), (dict(k=129), b"k 129"), (dict(k=-1), b"k -1")):
        refused(topk(**kw), word)


# ------------------------------------------------------------------ the host definitions, hand-worked
OFF3, POS3 = np.array([0, 2, 5, 6], np.int64), np.array([0, 1, 0, 1, 2, 2], np.int32)          # {0, 1}, {0, 1, 2}, {2}


def test_cooc_of_three_users_by_hand():
    C3 = bl.cooc_host(OFF3, POS3, 3)
    assert C3.dtype == np.uint32 and C3.tolist() == [[2, 2, 1], [2, 2, 1], [1, 1, 2]]
    assert bl.pair_counts(OFF3) == 4 + 9 + 1 == int(C3.sum())
    # a position outside [0, m) counts nowhere; offsets beyond nnz are clamped; an end below its start is an empty range
    assert bl.cooc_host([0, 3], [0, 7, -1], 3).tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert bl.cooc_host([0, 9, 4], [1, 2], 3).tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 1]]
    assert not bl.cooc_host([0, 0], [], 4).any()
    with pytest.raises(ValueError):
        bl.check_csr([0, 2], [1, 1], 3)                      # not distinct
    with pytest.raises(ValueError):
        bl.check_csr([0, 2], [0, 3], 3)                      # outside the catalogue
    with pytest.raises(ValueError):
        bl.check_csr([0, 3], [0, 1], 3)                      # the offsets do not end at nnz
    off, pos = bl.check_csr([0, 2, 2, 3], [1, 2, 0], 3)     # a drop between two users is no disorder
    assert off.dtype == np.int64 and pos.dtype == np.int32


def test_history_scores_by_hand_at_shrink_zero():
    C3 = bl.cooc_host(OFF3, POS3, 3)
    s = bl.history_scores_host(C3, OFF3, POS3, [0, 1, 2, -1, 3], 0.0)
    assert s.dtype == F32 and s.shape == (5, 3)
    # sim(0, 1) = 2 / (sqrt 2 * sqrt 2), sim(0, 2) = sim(1, 2) = 1 / (sqrt 2 * sqrt 2): 1 and 1 / 2 in real numbers.  Under the
    # definition's separately rounded fp32 operations sqrtf(2)^2 rounds to 2 - 2^-23, so they are one ulp above: worked here
    # operation by operation.  A user's own item adds nothing.
    r2 = np.sqrt(F32(2))
    one, half = F32(2) / (r2 * r2), F32(1) / (r2 * r2)
    assert (r2 * r2).view(np.uint32) == 0x3fffffff and one.view(np.uint32) == 0x3f800001 and half.view(np.uint32) == 0x3f000001
    assert s[0].tolist() == [one, one, half + half]
    assert s[1].tolist() == [one + half, one + half, half + half]
    assert s[2].tolist() == [half, half, 0.0]
    assert s[3].tolist() == s[4].tolist() == [0.0, 0.0, 0.0] and not np.signbit(s[3:]).any()          # no such user: +0.0
    # with square counts every operation is exact: four users that all hold {0, 1}, one of them also 2 -> sim(0, 1) = 4 / (2 * 2)
    off4, pos4 = np.array([0, 2, 4, 6, 9]), np.array([0, 1, 0, 1, 0, 1, 0, 1, 2])
    C4 = bl.cooc_host(off4, pos4, 3)
    assert C4.tolist() == [[4, 4, 1], [4, 4, 1], [1, 1, 1]]
    assert bl.history_scores_host(C4, off4, pos4, [0, 3], 0.0).tolist() == [[1.0, 1.0, 1.0], [1.5, 1.5, 1.0]]
    sixth = F32(1) / F32(6)
    assert bl.history_scores_host(C4, off4, pos4, [0], 4.0).tolist() == [[0.5, 0.5, sixth + sixth]]
    s10 = bl.history_scores_host(C3, OFF3, POS3, [1], 10.0)
    assert s10[0, 0] == F32(2) / (r2 * r2 + F32(10)) + F32(1) / (r2 * r2 + F32(10))
    # an item nobody holds: +0.0 everywhere at shrink 0, never NaN (its counts are 0: no division happens)
    s4 = bl.history_scores_host(bl.cooc_host(OFF3, POS3, 4), OFF3, POS3, [0, 1, 2], 0.0)
    assert s4[:, 3].tolist() == [0.0, 0.0, 0.0] and np.array_equal(s4[:, :3], s[:3]) and not np.isnan(s4).any()
    for bad in (-1.0, 2.0 ** 20 + 1, float("nan")):
        with pytest.raises(ValueError):
            bl.history_scores_host(C3, OFF3, POS3, [0], bad)


def test_the_fp32_replay_is_within_the_derived_bound_of_its_float64_form():
    rs = np.random.RandomState(11)
    worst = 0.0
    for case in range(40):
        m, n_user = int(rs.randint(2, 201)), int(rs.randint(1, 60))
        held = rs.random_sample((n_user, m)) < rs.uniform(0.02, 0.9)
        off = np.concatenate([[0], np.cumsum(held.sum(1))]).astype(np.int64)
        pos = np.nonzero(held)[1].astype(np.int32)
        C = bl.cooc_host(off, pos, m)
        assert np.array_equal(C, (held.T.astype(np.int64) @ held.astype(np.int64)).astype(np.uint32))
        shrink = (0.0, 1.0, 10.0)[case % 3]
        q = np.arange(n_user)
        a = bl.history_scores_host(C, off, pos, q, shrink)
        b = bl.history_scores_host(C, off, pos, q, shrink, dtype=np.float64)
        assert a.dtype == F32 and b.dtype == np.float64 and (b >= 0).all()
        bound = np.array([bl.error_bound(n) for n in np.diff(off)])[:, None] * b
        assert (np.abs(a.astype(np.float64) - b) <= bound).all(), case
        nz = b > 0
        worst = max(worst, float((np.abs(a.astype(np.float64) - b)[nz] / np.broadcast_to(bound, b.shape)[nz]).max()) if nz.any() else 0.0)
    print("worst |fp32 - float64| as a share of (L + 8) 2^-24 float64: %.3f" % worst)
    assert 0 < worst <= 1


def csr(lists):
    return rec.exclusion_csr(lists, len(lists))


def test_ranks_and_lists_order_as_the_key_says():
    nan, inf = np.nan, np.inf
    # an all-equal row ranks by ascending id
    t_off, t_ids = csr([[3, 0, 5]])
    ranks, live, out = bl.rank_scores_host(np.full(6, 2.5, F32), 1, t_off, t_ids)
    assert ranks.tolist() == [0, 3, 5] and live.tolist() == [6] and out.tolist() == [2.5] * 3
    ids, scores = bl.topk_scores_host(np.full(6, 2.5, F32), 1, 4)
    assert ids.tolist() == [[0, 1, 2, 3]] and scores.dtype == F32
    # +inf, numbers, +0 = -0 (by id), negatives, -inf, NaN last
    row = np.array([0.0, nan, -inf, 3.0, -0.0, inf, -1.0, 3.0], F32)
    ids, scores = bl.topk_scores_host(row, 1, 8)
    assert ids.tolist() == [[5, 3, 7, 0, 4, 6, 2, 1]]
    assert scores[0, :7].tolist() == [inf, 3.0, 3.0, 0.0, 0.0, -1.0, -inf] and np.isnan(scores[0, 7])
    assert not np.signbit(scores[0, 4])                                      # the -0.0 leaves as +0.0
    t_off, t_ids = csr([np.arange(8)])
    ranks, live, out = bl.rank_scores_host(row, 1, t_off, t_ids)
    assert ranks.tolist() == [3, 7, 6, 1, 4, 0, 5, 2] and np.signbit(out[4]) and np.isnan(out[1])      # the raw bits come back
    # a rank below k is the position in the list
    assert all(ids[0, r] == t for t, r in enumerate(ranks))
    # candidates with ids of their own; a target that is no candidate gets -1 / 0; an excluded target is ranked against the live
    cand = np.array([10, 20, 30, 40], np.int32)
    sc = np.array([[1, 4, 3, 2], [9, 9, 9, 9]], F32)
    t_off, t_ids = csr([[20, 25, 40], [10, 30]])
    e_off, e_ids = csr([[30, 40], []])
    ranks, live, out = bl.rank_scores_host(sc, 2, t_off, t_ids, cand, e_off, e_ids)
    assert ranks.tolist() == [0, -1, 1, 0, 2] and live.tolist() == [2, 4] and out.tolist() == [4.0, 0.0, 2.0, 9.0, 9.0]
    ids, scores = bl.topk_scores_host(sc, 2, 3, cand, e_off, e_ids)
    assert ids.tolist() == [[20, 10, -1], [10, 20, 30]] and scores.tolist() == [[4.0, 1.0, 0.0], [9.0, 9.0, 9.0]]
    # one row for every query (stride 0) is the same row repeated
    one = bl.rank_scores_host(sc[0], 2, t_off, t_ids, cand, e_off, e_ids)
    two = bl.rank_scores_host(np.stack([sc[0], sc[0]]), 2, t_off, t_ids, cand, e_off, e_ids)
    assert all(np.array_equal(x, y) for x, y in zip(one, two))
    # every candidate excluded: nothing is live, the list is all padding
    e_off, e_ids = csr([[10, 20, 30, 40], [10, 20, 30, 40]])
    ranks, live, _ = bl.rank_scores_host(sc, 2, t_off, t_ids, cand, e_off, e_ids)
    assert ranks.tolist() == [0, -1, 0, 0, 0] and live.tolist() == [0, 0]
    assert bl.topk_scores_host(sc, 2, 2, cand, e_off, e_ids)[0].tolist() == [[-1, -1], [-1, -1]]
    for bad in (0, 129):
        with pytest.raises(ValueError):
            bl.topk_scores_host(sc, 2, bad)
    assert bl.jaccard([[1, 2, -1], [3, 4, 5], [-1, -1, -1]], [[2, 9, -1], [5, 4, 3], [-1, -1, -1]]) == pytest.approx((1 / 3 + 1) / 2)


# ------------------------------------------------------------------ histories of a tiny dataset
class TinyData(object):
    def __init__(self, uid, pid, label):
        self.train_dataset = {4: {"data": {"uid": np.asarray(uid), "pid": np.asarray(pid), "label": np.asarray(label, F32)}}}


def test_histories_of_a_tiny_dataset():
    #            user 7 holds 30 twice and 10; user 2 holds 50 (and 99: no catalogue item); user 5 only label-0 rows
    ds = TinyData(uid=[7, 7, 2, 7, 5, 2, 5, 9], pid=[30, 10, 50, 30, 10, 99, 30, 77], label=[1, 1, 1, 1, 0, 1, 0, 1])
    h = bl.histories(ds, 4, [10, 30, 50, 60])
    assert h["users"].tolist() == [2, 7]                     # 5 has no label-1 row, 9 none in the catalogue
    assert h["off"].tolist() == [0, 1, 3] and h["pos"].tolist() == [2, 0, 1]
    assert h["off"].dtype == np.int64 and h["pos"].dtype == np.int32
    assert h["popularity"].tolist() == [1, 2, 1, 0]          # rows, duplicates included; label-0 rows not
    bl.check_csr(h["off"], h["pos"], 4)
    assert np.array_equal(h["popularity"], lm.id_counts_host(ds.train_dataset[4]["data"]["pid"], 100,
                                                             ds.train_dataset[4]["data"]["label"])[[10, 30, 50, 60]])
    empty = bl.histories(ds, 3, [10, 30])                    # no such train split
    assert empty["users"].size == 0 and empty["off"].tolist() == [0] and empty["popularity"].tolist() == [0, 0]
    with pytest.raises(ValueError):
        bl.histories(ds, 4, [30, 10])


# ------------------------------------------------------------------ the command line
def test_flags_parse(monkeypatch, capsys):
    seen = []
    assert "--baselines [SHRINK]" in cli.__doc__ and "--baselines-out" in cli.__doc__ and "--baselines-max-items" in cli.__doc__
    assert "train.baselines" in cli.main.__doc__
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path, "--rank-eval"])
    cli.cli(["--config", cfg_path, "--rank-eval", "10,50", "--baselines"])
    cli.cli(["--config", cfg_path, "--rank-eval", "5", "--baselines", "2.5", "--baselines-out", "b.npz", "--baselines-max-items",
             "4000", "--recommend", "7"])
    train = [s[0][0]["train"] for s in seen]
    assert not any(key.startswith("baselines") for key in train[0]) and seen[0][1] == {}
    assert train[1]["baselines"] == 10.0 and train[1]["rank_eval"] == [10, 50] and "baselines_out" not in train[1]
    assert "baselines_max_items" not in train[1] and seen[1][1] == {}
    assert train[2]["baselines"] == 2.5 and train[2]["baselines_out"] == "b.npz" and train[2]["baselines_max_items"] == 4000
    assert seen[2][1] == {"recommend": 7, "recommend_out": None}
    for bad in (["--baselines"], ["--baselines", "3"],                                           # no --rank-eval
                ["--rank-eval", "--baselines", "-1"], ["--rank-eval", "--baselines", "1048577"], ["--rank-eval", "--baselines", "nan"],
                ["--rank-eval", "--baselines-out", "x.npz"], ["--rank-eval", "--baselines-max-items", "10"],
                ["--rank-eval", "--baselines", "--baselines-max-items", "0"],
                ["--rank-eval", "--baselines", "--baselines-max-items", "65536"],
                ["--rank-eval", "--baselines", "--recommend", "129"]):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path] + bad)
    assert "--baselines needs --rank-eval" in capsys.readouterr().err
    assert len(seen) == 3


def test_several_lanes_are_refused_by_name(tmp_path):
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr")
    cfg["train"].update(lanes=2, rank_eval=[10], baselines=10.0)
    with pytest.raises(NotImplementedError, match=r"train\.baselines \(run\.py --baselines\).*not ranked across processes "
                                                  r"or lanes.*one process"):
        cli.main(cfg, RecommendingEngine)
    cfg = tiny_config(tmp_path, "mlp")
    cfg["train"].update(baselines=10.0)
    with pytest.raises(ValueError, match=r"train\.baselines needs train\.rank_eval"):
        cli.main(cfg, RecommendingEngine)


# ------------------------------------------------------------------ the report over a CPU stand-in
def _np(x):
    return x if x is None else (x.numpy() if hasattr(x, "numpy") else np.asarray(x))


class BaselineEngine(RankEngine, RecommendingEngine):
    """the tower's rank_domain and recommend as numpy forwards, and the four score calls (and id_counts) as their host
    definitions over CPU tensors, with the engine methods' argument order and return types.  It records its score calls."""
    calls = []

    def id_counts(self, ids, n_bins, label=None):
        return torch.from_numpy(lm.id_counts_host(_np(ids), n_bins, None if label is None else _np(label)).astype(np.int32))

    def item_cooc(self, off, pos, m):
        type(self).calls.append(("item_cooc", int(m)))
        return torch.from_numpy(bl.cooc_host(_np(off), _np(pos), m).view(np.int32))

    def history_scores(self, cooc, off, pos, queries, shrink):
        type(self).calls.append(("history_scores", int(queries.shape[0])))
        return torch.from_numpy(bl.history_scores_host(_np(cooc).view(np.uint32), _np(off), _np(pos), _np(queries), shrink))

    def rank_scores(self, scores, n_query, tgt_off, tgt_ids, candidates=None, excl_off=None, excl_ids=None, want_scores=False):
        type(self).calls.append(("rank_scores", int(n_query), int(scores.dim())))
        r, live, s = bl.rank_scores_host(_np(scores), n_query, _np(tgt_off), _np(tgt_ids), _np(candidates), _np(excl_off), _np(excl_ids))
        out = (torch.from_numpy(r), torch.from_numpy(live))
        return out + (torch.from_numpy(s),) if want_scores else out

    def topk_scores(self, scores, n_query, k, candidates=None, excl_off=None, excl_ids=None):
        ids, s = bl.topk_scores_host(_np(scores), n_query, k, _np(candidates), _np(excl_off), _np(excl_ids))
        return torch.from_numpy(ids), torch.from_numpy(s)


def pop_ranks_by_counting(model, d):
    """MostPopular's ranks from the protocol's words alone: nothing of baselines.py but the popularity vector's meaning."""
    ds = model.dataset
    cat, users, exclude = model._retrieval_problem(d, None, True)
    tr = ds.train_dataset[d]["data"]
    pop = np.bincount(np.asarray(tr["pid"])[np.asarray(tr["label"]) > 0], minlength=int(cat.max()) + 1)[cat].astype(F32)
    out = []
    for q, pos in enumerate(rec.split_positives(ds, d, users)):
        ok = ~np.isin(cat, np.asarray(exclude[q], np.int64))
        for t in np.unique(pos):
            pt = pop[cat == t]
            out.append(int(((pop[ok] > pt) | ((pop[ok] == pt) & (cat[ok] < t))).sum()) if pt.size else -1)
    return out


def result_json(tmp_path, name, cfg):
    rdir = os.path.join(str(tmp_path / "result"), name, "Taobao", cfg["dataset"]["domain_split_path"])
    run = [p for p in os.listdir(rdir) if os.path.isdir(os.path.join(rdir, p))]
    assert len(run) == 1
    with open(os.path.join(rdir, run[0], "result.json")) as f:
        return json.load(f), rdir


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr"])
def test_report_and_headline_end_to_end_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    out = str(tmp_path / "base.npz")
    cfg["train"].update(rank_eval=[1, 10], baselines=10.0, baselines_out=out)
    built = []
    BaselineEngine.calls, RankEngine.log = [], []
    monkeypatch.setattr(bl, "block_queries", lambda m, n_query: 37)     # several blocks of queries per domain
    res = cli.main(cfg, BaselineEngine, on_model=built.append, recommend=5)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model = built[0]
    text = capsys.readouterr().out
    live = model.model.weights.numpy().copy()
    # the tower was ranked once per domain (rank_report's figures are reused, not recomputed)
    assert [d for d, _ in RankEngine.log] == [0, 1, 2]
    assert [c for c in BaselineEngine.calls if c[0] == "item_cooc"] == [("item_cooc", model._retrieval_problem(d, None, True)[0].size)
                                                                        for d in range(3)]
    assert max(c[1] for c in BaselineEngine.calls if c[0] == "history_scores") <= 37
    assert len([c for c in BaselineEngine.calls if c[0] == "history_scores"]) > 3
    assert {c[2] for c in BaselineEngine.calls if c[0] == "rank_scores"} == {1, 2}         # one row (pop) and a matrix (itemknn)
    with np.load(out) as z, np.load(os.path.join(model.result_path, "rank_eval.npz")) as zr:
        assert z["domains"].tolist() == [0, 1, 2] and z["ks"].tolist() == [1, 10] and float(z["shrink"]) == 10.0 and int(z["k_lists"]) == 5
        assert not z["skipped"].any()
        for d in range(3):
            cat = model._retrieval_problem(d, None, True)[0]
            assert z["m"][d] == cat.size
            for key in ("users", "offsets", "ids", "listed", "live"):            # the tower's problem, line for line
                assert np.array_equal(z["%s_%d" % (key, d)], zr["%s_%d" % (key, d)]), (key, d)
            for who in bl.WHICH:
                want = bl.rank_host(model, d, who, 10.0, k=5)
                assert np.array_equal(z["ranks_%s_%d" % (who, d)], want["ranks"]) and z["ranks_%s_%d" % (who, d)].dtype == np.int32
                one = bl.rank(model, d, who, 10.0, k=5, block=10 ** 6)           # one block: the same bytes
                assert one["ranks"].tobytes() == want["ranks"].tobytes() and one["top_ids"].tobytes() == want["top_ids"].tobytes()
                assert one["live"].tobytes() == want["live"].tobytes() == zr["live_%d" % d].tobytes()
                assert sorted(one) == sorted(["offsets", "ids", "ranks", "listed", "live", "users", "catalogue", "n_positives",
                                              "n_cold", "top_ids", "top_scores"])
                m = rec.rank_metrics(want["offsets"], want["ranks"], zr["listed_%d" % d], want["live"], np.diff(want["offsets"]), [1, 10])
                assert z["mrr_" + who][d] == m["mrr"] and z["ndcg_at_10_" + who][d] == m["ndcg"][1]
                assert z["hit_rate_at_1_" + who][d] == m["hit_rate"][0] and z["mean_percentile_" + who][d] == m["mean_percentile"]
            assert z["ranks_pop_%d" % d].tolist() == pop_ranks_by_counting(model, d)
            knn = bl.rank_host(model, d, "itemknn", 10.0, k=5)
            assert np.array_equal(z["itemknn_ids_%d" % d], knn["top_ids"]) and np.array_equal(z["itemknn_scores_%d" % d], knn["top_scores"])
            users = z["users_%d" % d]
            have = np.unique(model.dataset.train_dataset[d]["data"]["uid"][model.dataset.train_dataset[d]["data"]["label"] > 0])
            assert z["n_cold"][d] == (~np.isin(users, have)).sum()
            mine = model.recommend(d, 5)["ids"]
            assert z["overlap_pop"][d] == bl.jaccard(mine, bl.rank_host(model, d, "pop", k=5)["top_ids"])
            assert z["overlap_itemknn"][d] == bl.jaccard(mine, knn["top_ids"])
            assert re.search(r"^%d: tower +MRR \d\.\d{4} MeanPercentile \d\.\d{4} HitRate@1 " % d, text, flags=re.M)
            assert re.search(r"^%d: pop +MRR \d\.\d{4} .*NDCG@10 \d\.\d{4}$" % d, text, flags=re.M)
            assert re.search(r"^%d: itemknn +MRR \d\.\d{4} .*\(%d cold users" % (d, z["n_cold"][d]), text, flags=re.M)
            assert re.search(r"^%d: overlap +Jaccard@5 .*MostPopular \d\.\d{4} with ItemKNN \d\.\d{4}$" % d, text, flags=re.M)
        assert z["n_cold"].sum() > 0 and (z["mrr_itemknn"] > 0).all() and (z["mrr_pop"] > 0).all()
    assert "Baselines under the rank-eval protocol" in text and "shrink 10" in text and "Baselines written to" in text
    assert text.index("Ranks written to") < text.index("Baselines under")
    assert np.array_equal(model.model.weights.numpy(), live)             # the report reads state only
    result, _ = result_json(tmp_path, name, cfg)
    with np.load(out) as z:
        assert result["baselines_shrink"] == 10.0 and result["baselines_skipped"] == []
        for fig in bl.figures([1, 10]):
            for who in bl.WHICH:
                assert set(result["domain_%s_%s" % (fig, who)]) == {"0", "1", "2"}
                assert result["domain_%s_%s" % (fig, who)]["1"] == float(z["%s_%s" % (fig, who)][1])
                assert result["avg_%s_%s" % (fig, who)] == pytest.approx(float(np.mean(z["%s_%s" % (fig, who)])))
        assert result["domain_overlap_pop"]["2"] == float(z["overlap_pop"][2]) and set(result["domain_overlap_itemknn"]) == {"0", "1", "2"}
        assert result["domain_cold_users"] == {str(d): int(z["n_cold"][d]) for d in range(3)}
    assert "avg_auc" in result                                           # (save_result's own keys are still there)


def test_a_catalogue_beyond_max_items_gets_most_popular_only_and_is_named(tmp_path, monkeypatch, capsys):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "wdl", epochs=1)
    cfg["train"].update(rank_eval=[10], baselines=0.0, baselines_max_items=50)
    BaselineEngine.calls = []
    built = []
    cli.main(cfg, BaselineEngine, on_model=built.append)
    text = capsys.readouterr().out
    assert not [c for c in BaselineEngine.calls if c[0] in ("item_cooc", "history_scores")]
    for d in range(3):
        assert re.search(r"^%d: itemknn +skipped: \d+ items exceed train\.baselines_max_items = 50 .*MostPopular only$" % d, text, flags=re.M)
    assert "overlap" not in text                                         # no --recommend: no lists to compare
    result, rdir = result_json(tmp_path, "wdl", cfg)
    assert result["baselines_skipped"] == [0, 1, 2] and result["baselines_shrink"] == 0.0
    assert "domain_mrr_pop" in result and "avg_ndcg_at_10_pop" in result
    assert not [k for k in result if k.endswith("_itemknn")] and "domain_overlap_pop" not in result
    assert "baselines.npz" in os.listdir(rdir)                           # the default path
    with np.load(os.path.join(rdir, "baselines.npz")) as z:
        assert z["skipped"].all() and np.isnan(z["mrr_itemknn"]).all() and z["ranks_itemknn_0"].size == 0
        assert z["ranks_pop_1"].tolist() == pop_ranks_by_counting(built[0], 1)


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch, capsys):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "wdl", epochs=1)
    cfg["train"].update(rank_eval=[10])
    BaselineEngine.calls = []
    cli.main(cfg, BaselineEngine)
    assert not BaselineEngine.calls and "Baselines" not in capsys.readouterr().out
    result, rdir = result_json(tmp_path, "wdl", cfg)
    assert not [k for k in result if "baselines" in k or k.endswith("_pop")]
    assert [p for p in os.listdir(rdir) if p.endswith(".npz")] == ["rank_eval.npz"]
