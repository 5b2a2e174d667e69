"""Exact full-catalogue ranks, host side (no GPU): `recommend.rank_metrics` against `recommend.ranking_metrics` and
hand-computed cases, the C ABI's declaration and binding, `run.py --rank-eval`, and `recommend.rank_report` end to end
through `cli.main` over a CPU stand-in of the engine whose `rank_domain` ranks the oracle's predictions in numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gauc_host as gh          # tiny_config, patch_emb_dim: the 3-domain stand-in run of the GAUC host tests
from fake_engine import FakeEngine
from mamdr_amd import _lib, cli, recommend
from oracle import outer as oouter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ rank_metrics
def lists_from_ranks(offsets, ranks, listed, k):
    """a [Q, k] top-k table in which the listed target of rank r < k sits at position r under a code of its own (its flat
    position), every other position under a filler no positive set holds -> (ids, positives per query)."""
    nq = len(offsets) - 1
    ids = np.full((nq, k), -1, np.int64)
    positives = []
    for q in range(nq):
        ids[q] = 10 ** 6 + np.arange(k)
        positives.append(np.arange(offsets[q], offsets[q + 1]))
        for j in range(offsets[q], offsets[q + 1]):
            if listed[j] and ranks[j] < k:
                ids[q, ranks[j]] = j
    return ids, positives


def random_case(seed, n_query=40, live=300, p_unlisted=0.25):
    rs = np.random.RandomState(seed)
    counts = rs.randint(0, 9, n_query)
    counts[[3, 17]] = 0                                     # queries without positives
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    p = 1.0 / (np.arange(live) + 1.0)                       # distinct ranks per query, the early ones likelier (K = 1 has hits)
    ranks = np.concatenate([rs.choice(live, c, replace=False, p=p / p.sum()) for c in counts]
                           + [np.zeros(0, np.int64)]).astype(np.int32)
    listed = rs.random_sample(ranks.size) >= p_unlisted
    return offsets, ranks, listed, np.full(n_query, live, np.int32), counts.astype(np.int64)


@pytest.mark.parametrize("p_unlisted", [0.0, 0.25], ids=["all-listed", "some-unlisted"])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_rank_metrics_agree_with_ranking_metrics(k, p_unlisted):
    offsets, ranks, listed, live, n_pos = random_case(k, p_unlisted=p_unlisted)
    assert (n_pos == 0).sum() >= 2 and (p_unlisted == 0 or 0 < listed.sum() < listed.size)
    got = recommend.rank_metrics(offsets, ranks, listed, live, n_pos, [k])
    ids, positives = lists_from_ranks(offsets, ranks, listed, k)
    want = recommend.ranking_metrics(ids, positives)
    assert got["n_eval"] == want["n_eval"] == int((n_pos > 0).sum())
    assert got["ks"] == [k]
    for name in ("hit_rate", "recall", "ndcg"):
        assert got[name].shape == (1,) and got[name].dtype == np.float64
        assert abs(got[name][0] - want[name]) <= 1e-12, (name, got[name][0], want[name])
    assert want["hit_rate"] > 0
    # several K in one call are the single-K calls side by side
    many = recommend.rank_metrics(offsets, ranks, listed, live, n_pos, [1, 10, 128])
    i = [1, 10, 128].index(k)
    assert all(many[name][i] == got[name][0] for name in ("hit_rate", "recall", "ndcg"))
    assert many["mrr"] == got["mrr"] and many["mean_percentile"] == got["mean_percentile"]


def test_rank_metrics_hand_computed():
    # query 0: positives at ranks 4 and 0, both listed, 11 live; query 1: no positives (its stray entry is ignored);
    # query 2: ranks 9 (listed) and 2 (unlisted: a miss), 101 live; query 3: one positive, unlisted
    offsets = [0, 2, 2, 4, 5]
    ranks = [4, 0, 9, 2, 0]
    listed = [True, True, True, False, False]
    live = [11, 50, 101, 7]
    n_pos = [2, 0, 2, 1]
    m = recommend.rank_metrics(offsets, ranks, listed, live, n_pos, [1, 5, 10])
    assert m["n_eval"] == 3
    assert m["mrr"] == (1.0 / 1 + 1.0 / 10 + 0.0) / 3
    assert m["mean_percentile"] == (4 / 10.0 + 0 / 10.0 + 9 / 100.0) / 3          # over the three listed targets
    assert m["hit_rate"].tolist() == [1 / 3.0, 1 / 3.0, 2 / 3.0]
    assert m["recall"].tolist() == [(0.5 + 0 + 0) / 3, (1.0 + 0 + 0) / 3, (1.0 + 0.5 + 0) / 3]
    d = lambda r: 1.0 / np.log2(r + 2.0)      # noqa: E731
    assert abs(m["ndcg"][0] - (d(0) / d(0)) / 3) < 1e-15
    assert abs(m["ndcg"][1] - ((d(0) + d(4)) / (d(0) + d(1))) / 3) < 1e-15
    assert abs(m["ndcg"][2] - ((d(0) + d(4)) / (d(0) + d(1)) + d(9) / (d(0) + d(1))) / 3) < 1e-15
    # a single live candidate: the percentile's denominator is max(1, live - 1)
    one = recommend.rank_metrics([0, 1], [0], [True], [1], [1], [1])
    assert one["mean_percentile"] == 0.0 and one["mrr"] == 1.0 and one["hit_rate"].tolist() == [1.0]
    with pytest.raises(ValueError):
        recommend.rank_metrics([0, 2], [1], [True], [5], [1], [1])


def test_rank_metrics_all_empty():
    for offsets, n_pos in (([0], []), ([0, 0, 0], [0, 0])):
        m = recommend.rank_metrics(offsets, [], [], [5] * len(n_pos), n_pos, [1, 10])
        assert m["n_eval"] == 0 and m["mrr"] == 0.0 and m["mean_percentile"] == 0.0
        assert m["hit_rate"].tolist() == m["recall"].tolist() == m["ndcg"].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ C ABI
def test_rank_domain_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    m = re.search(r"\bint\s+mamdr_rank_domain\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "mamdr_rank_domain is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mamdr_ctx* ctx", "int32_t domain", "int32_t n_query", "const int32_t* d_uid", "const int32_t* d_cand",
                      "int64_t n_cand", "const int64_t* d_excl_off", "const int32_t* d_excl_ids", "const int64_t* d_tgt_off",
                      "const int32_t* d_tgt_ids", "int32_t* d_rank_out", "float* d_score_out", "int32_t* d_live_out"], params
    doc = header[:header.index("int mamdr_rank_domain")].rsplit("/*", 1)[1]
    assert "NO REFERENCE COUNTERPART" in doc
    for phrase in ("#{ c in candidates, live for q : key(q, c) > key(q, t) }", "The target never counts itself",
                   "A NaN-scored candidate is live", "exactly when its rank is r < k", "no floating-point atomic",
                   "MAMDR_REC_CHUNK", "Reads the state only"):
        assert phrase in doc, phrase
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_rank_domain"] == (C.c_int, [vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp])
    assert _lib.ABI_VERSION == 19 and re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert hasattr(_lib.load(), "mamdr_rank_domain")


# ------------------------------------------------------------------ the command line
def test_cli_flag_sets_train_rank_eval(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--rank-eval"])
    cli.cli(["--config", cfg_path, "--rank-eval", "5,128,1000"])
    cli.cli(["--config", cfg_path, "--rank-eval", "7", "--recommend", "10"])
    assert seen[0][1] == {} and len(seen[0][0]) == 1 and "rank_eval" not in seen[0][0][0]["train"]
    assert seen[1][1] == {} and len(seen[1][0]) == 1 and seen[1][0][0]["train"]["rank_eval"] == [10, 50, 200]
    assert seen[2][1] == {} and seen[2][0][0]["train"]["rank_eval"] == [5, 128, 1000]
    assert seen[3][1] == {"recommend": 10, "recommend_out": None} and seen[3][0][0]["train"]["rank_eval"] == [7]


def test_lanes_refuse_rank_eval_by_name(tmp_path, monkeypatch):
    gh.patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", rank_eval=[10], lanes=2)
    with pytest.raises(NotImplementedError, match="rank_eval"):
        cli.main(cfg, RankEngine)
    assert not loaded                    # refused before the data is loaded


# ------------------------------------------------------------------ run.py --rank-eval over a CPU stand-in
class RankEngine(FakeEngine):
    """FakeEngine with TowerEngine.rank_domain's contract, ranking the oracle's predictions in numpy (ties by ascending id);
    it records every call's domain and the live weights it ranked with."""
    log = []

    def rank_domain(self, uids, domain, targets, candidates=None, exclude=None, want_scores=False):
        uids = np.asarray(uids, np.int32).ravel()
        cand = np.arange(self.n_item, dtype=np.int32) if candidates is None else np.asarray(candidates, np.int32)
        t_off, t_ids = recommend.exclusion_csr(targets, uids.size, "targets")
        type(self).log.append((int(domain), self.weights.numpy().copy()))
        ranks, listed, live = np.zeros(t_ids.size, np.int32), np.zeros(t_ids.size, bool), np.zeros(uids.size, np.int32)
        for q, u in enumerate(uids):
            ex = np.unique(np.asarray(exclude[q], np.int64)) if exclude is not None else np.zeros(0, np.int64)
            ok = ~np.isin(cand, ex)
            live[q] = ok.sum()
            tq = t_ids[t_off[q]:t_off[q + 1]]
            if not tq.size:
                continue
            items = np.concatenate([cand, tq])
            s = self.oracle.predict(np.full(items.size, u, np.int32), items, np.full(items.size, domain, np.int32))
            sc, st = s[:cand.size][ok], s[cand.size:]
            for i, (t, x) in enumerate(zip(tq, st)):
                ranks[t_off[q] + i] = int(((sc > x) | ((sc == x) & (cand[ok] < t))).sum())
                listed[t_off[q] + i] = bool(np.isin(t, cand[ok]))
        return {"offsets": t_off, "ids": t_ids, "ranks": ranks, "listed": listed, "live": live}


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr"])
def test_rank_report_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    gh.patch_emb_dim(monkeypatch)
    RankEngine.log = []
    cfg = gh.tiny_config(tmp_path, name, epochs=2, rank_eval=[1, 10, 50])
    built = []
    res = cli.main(cfg, RankEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model = built[0]
    eng, ds = model.model, model.dataset
    assert [d for d, _ in RankEngine.log] == [0, 1, 2]                 # one call per domain, after the pipeline
    path = os.path.join(model.result_path, "rank_eval.npz")
    with np.load(path) as z:
        assert z["domains"].tolist() == [0, 1, 2] and z["ks"].tolist() == [1, 10, 50]
        assert z["mrr"].shape == z["mean_percentile"].shape == (3,)
        for n in ("hit_rate", "recall", "ndcg"):
            assert z[n].shape == (3, 3) and np.all((z[n] >= 0) & (z[n] <= 1))
        for n in ("hit_rate", "recall"):
            assert np.all(np.diff(z[n], axis=1) >= 0)                  # ... and grow with K
        for d in range(3):
            users, offsets, ids = z["users_%d" % d], z["offsets_%d" % d], z["ids_%d" % d]
            ranks, listed, live = z["ranks_%d" % d], z["listed_%d" % d], z["live_%d" % d]
            test = ds.test_dataset[d]["data"]
            assert np.array_equal(users, np.unique(test["uid"]))
            assert offsets.shape == (users.size + 1,) and offsets[-1] == ids.size == ranks.size == listed.size
            assert live.shape == (users.size,) and ranks.dtype == np.int32 and listed.dtype == bool
            # the targets are each user's label-1 items of the test split
            for q, u in enumerate(users.tolist()):
                want = np.unique(test["pid"][(test["uid"] == u) & (test["label"] > 0)])
                assert ids[offsets[q]:offsets[q + 1]].tolist() == want.tolist(), (d, u)
            assert np.all(ranks[listed] < np.repeat(live, np.diff(offsets))[listed])
            m = recommend.rank_metrics(offsets, ranks, listed, live, np.diff(offsets), [1, 10, 50])
            assert m["mrr"] == z["mrr"][d] and m["hit_rate"].tolist() == z["hit_rate"][d].tolist()
        assert z["mrr"].max() > 0
    text = capsys.readouterr().out
    assert "Rank eval" in text and text.count("MRR ") == 3 and text.count("HitRate@50") == 3 and "rank_eval.npz" in text
    if name == "mlp_meta_mamdr":
        # every domain was ranked under ITS merged best weights; the live vector is back afterwards
        for d, (dom, w) in enumerate(RankEngine.log):
            merged = oouter.merge(model.best_shared_weights.numpy(), model.best_domain_weights[d].numpy(),
                                  cfg["train"]["merged_method"])
            assert dom == d and np.array_equal(w, merged), d
        assert len({w.tobytes() for _, w in RankEngine.log}) == 3
        live_before = eng.weights.numpy().copy()
        again = model.rank_eval(1)
        assert np.array_equal(eng.weights.numpy(), live_before)
        assert np.array_equal(RankEngine.log[-1][1], RankEngine.log[1][1]) and not np.array_equal(live_before, RankEngine.log[1][1])
        with np.load(path) as z:
            assert np.array_equal(again["ranks"], z["ranks_1"])
    else:
        assert all(np.array_equal(w, eng.weights.numpy()) for _, w in RankEngine.log)
