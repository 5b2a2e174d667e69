"""Per-query slates and the sampled-negatives evaluation, host side (no GPU): `mamdr_rank_slates`' declaration and binding,
the refusals that need no device, `recommend.sample_negatives`' properties, `BaseModel.rerank` / `sampled_eval` and
`SpecificBase.sampled_eval` over a CPU stand-in of the engine whose `rank_slates` orders the oracle's predictions in numpy,
`recommend.sampled_report`, and `run.py --sampled-eval`."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import test_gauc_host as gh          # tiny_config, patch_emb_dim: the 3-domain stand-in run of the GAUC host tests
from mamdr_amd import _lib, cli, recommend
from oracle import outer as oouter
from test_recommend_host import RecommendingEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI
def test_rank_slates_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    m = re.search(r"\bint\s+mamdr_rank_slates\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "mamdr_rank_slates is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mamdr_ctx* ctx", "int32_t domain", "int32_t n_query", "const int32_t* d_uid",
                      "const int64_t* d_slate_off", "const int32_t* d_slate_ids", "float* d_score_out", "int32_t* d_pos_out",
                      "int32_t* d_order_out"], params
    doc = header[:header.index("int mamdr_rank_slates")].rsplit("/*", 1)[1]
    for phrase in ("NO REFERENCE COUNTERPART", "O(L^2)", "mamdr_rank_domain's job", "MAMDR_REC_CHUNK", "no atomics",
                   "Reads the state only", "MAMDR_ENOTBUILT"):
        assert phrase in doc, phrase
    vp, i32 = C.c_void_p, C.c_int32
    assert _lib.SIGNATURES["mamdr_rank_slates"] == (C.c_int, [vp, i32, i32, vp, vp, vp, vp, vp, vp])
    assert _lib.ABI_VERSION == 19 and re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert hasattr(_lib.load(), "mamdr_rank_slates")


def test_null_context_is_refused_without_a_device():
    lib = _lib.load()
    code = lib.mamdr_rank_slates(None, 0, 1, None, None, None, None, None, None)
    assert code == _lib.EINVAL
    assert b"null context" in lib.mamdr_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(code)


def test_generic_layer_engine_refuses_by_name():
    from mamdr_amd import graph_engine
    eng = graph_engine.GraphEngine.__new__(graph_engine.GraphEngine)      # (no device: the refusal needs none)
    eng.kind = "mmoe"
    with pytest.raises(NotImplementedError, match="generic-layer towers.*mmoe.*not built for retrieval"):
        eng.rank_slates([0], 0, [[1, 2]])
    eng.ctx = None


def test_slates_csr_keeps_order_and_refuses_duplicates():
    off, ids = recommend.slates_csr([[5, 1, 3], [], None, np.array([7]), (9, 2)], 5)
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert off.tolist() == [0, 3, 3, 3, 4, 6] and ids.tolist() == [5, 1, 3, 7, 9, 2]
    off, ids = recommend.slates_csr([], 0)
    assert off.tolist() == [0] and ids.size == 0
    assert recommend.slates_csr([[4, 5], [5, 4]], 2)[1].tolist() == [4, 5, 5, 4]      # the same id in two slates is fine
    with pytest.raises(ValueError, match="the call has 2"):
        recommend.slates_csr([[1]], 2)
    with pytest.raises(ValueError, match="out of range"):
        recommend.slates_csr([[-1]], 1)
    with pytest.raises(ValueError, match="item 3 is listed twice in the slate of query 1"):
        recommend.slates_csr([[3], [3, 8, 3]], 2)


# ------------------------------------------------------------------ sample_negatives
def test_sample_negatives_properties():
    rs = np.random.RandomState(5)
    cat = rs.choice(1000, 60, replace=False)
    n_slate, n_neg = 300, 20
    # forbidden lists in any order, with repeats and with ids outside the catalogue
    forbid = [np.concatenate([rs.choice(cat, rs.randint(0, 40)), rs.choice(1200, 5)]) for _ in range(n_slate)]
    for i in range(10, 30):
        forbid[i] = rs.permutation(cat[:33 + i])                 # 17 .. 0 free items: slates that take all they have
    forbid[7] = np.concatenate([cat, cat])                       # the whole catalogue forbidden, twice
    forbid[8] = cat[:55]                                         # five free items
    forbid[9] = np.zeros(0, np.int64)
    f_off = np.concatenate([[0], np.cumsum([f.size for f in forbid])])
    f_ids = np.concatenate(forbid)
    off, ids = recommend.sample_negatives(cat, f_off, f_ids, n_neg, seed=11)
    assert off.dtype == np.int64 and off.shape == (n_slate + 1,) and off[0] == 0 and off[-1] == ids.size
    for s in range(n_slate):
        got = ids[off[s]:off[s + 1]]
        free = np.setdiff1d(cat, forbid[s])
        assert got.size == min(n_neg, free.size), s
        assert np.isin(got, free).all() and np.unique(got).size == got.size, s
    assert off[8] == off[7] and off[9] - off[8] == 5 and off[10] - off[9] == n_neg
    assert (np.diff(off) < n_neg).sum() > 3 and (np.diff(off) == n_neg).sum() > 100
    # a function of its arguments: the same seed gives the same bytes, another seed another draw
    off2, ids2 = recommend.sample_negatives(cat, f_off, f_ids, n_neg, seed=11)
    assert off2.tobytes() == off.tobytes() and ids2.tobytes() == ids.tobytes()
    off3, ids3 = recommend.sample_negatives(cat, f_off, f_ids, n_neg, seed=12)
    assert off3.tobytes() == off.tobytes() and ids3.tobytes() != ids.tobytes()
    # nothing to do
    off0, ids0 = recommend.sample_negatives(cat, [0], [], n_neg, seed=0)
    assert off0.tolist() == [0] and ids0.size == 0
    off0, ids0 = recommend.sample_negatives(cat, [0, 0, 0], [], 0, seed=0)
    assert off0.tolist() == [0, 0, 0] and ids0.size == 0
    with pytest.raises(ValueError):
        recommend.sample_negatives(cat, [0, 3], [1], 2, seed=0)


def _pinned_case(f_len, n_neg):
    rs = np.random.RandomState(3)
    cat = rs.choice(5000, 400, replace=False)
    cnt = rs.randint(0, f_len + 1, 500)
    f_ids = np.concatenate([cat, [7, 9]])[rs.randint(0, 402, int(cnt.sum()))]
    return cat, np.concatenate([[0], np.cumsum(cnt)]), f_ids, n_neg, 21


@pytest.mark.parametrize("f_len,n_neg,digest", [(4, 30, "1f9b0f0ec3716494416c55f1141f5b424a507903"),
                                                (60, 30, "f8f17981681ca511b0c0beb539092ff7f2d265c5"),
                                                (4, 200, "31845082281dbe179b21c6b25b3df28808590fb2")])
def test_sample_negatives_draws_are_pinned(f_len, n_neg, digest, monkeypatch):
    """The draws are part of the function (evaluation protocols are compared across runs): the bytes that the first
    implementation -- one binary search per draw, a stable argsort per slate -- gave for forbidden lists of up to 4 ids (now
    compared through the per-slate table), of up to 60 (still searched) and for more draws per slate than 128; and the table
    and the search give the same bytes on the same input."""
    import hashlib
    off, ids = recommend.sample_negatives(*_pinned_case(f_len, n_neg))
    assert hashlib.sha1(off.tobytes() + ids.tobytes()).hexdigest() == digest
    monkeypatch.setattr(recommend, "SAMPLE_SCAN_MAX", 0 if f_len <= recommend.SAMPLE_SCAN_MAX else 64)
    off2, ids2 = recommend.sample_negatives(*_pinned_case(f_len, n_neg))
    assert off2.tobytes() == off.tobytes() and ids2.tobytes() == ids.tobytes()


def test_sample_negatives_is_uniform():
    """50 items, 10 forbidden, 5 of the 40 free ones per slate, 4,000 slates: every free item is expected 500 times with
    sigma = sqrt(4000 * (1/8) * (7/8)) = 20.9: all 40 counts within 5 sigma, [395, 605]."""
    cat = np.arange(100, 150)
    n_slate = 4000
    forbid = np.tile(np.arange(100, 150, 5), n_slate)
    off, ids = recommend.sample_negatives(cat, np.arange(n_slate + 1) * 10, forbid, 5, seed=2024)
    assert np.array_equal(np.diff(off), np.full(n_slate, 5))
    counts = np.bincount(ids, minlength=150)[100:]
    assert counts[::5].sum() == 0
    free = np.delete(counts, np.arange(0, 50, 5))
    print("counts of the free items: min %d max %d" % (free.min(), free.max()))
    assert free.shape == (40,) and free.sum() == 20000 and free.min() >= 395 and free.max() <= 605


def test_sample_negatives_has_no_loop_over_slates_on_the_common_path():
    n_slate = 100000
    rs = np.random.RandomState(0)
    f_ids = rs.randint(0, 5000, 3 * n_slate)
    t0 = time.time()
    off, ids = recommend.sample_negatives(np.arange(5000), np.arange(n_slate + 1) * 3, f_ids, 99, seed=1)
    dt = time.time() - t0
    print("100,000 slates x 99 draws: %.2f s" % dt)
    assert off[-1] == 99 * n_slate
    rows = ids.reshape(n_slate, 99)
    srt = np.sort(rows, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    assert not (rows[:, :, None] == f_ids.reshape(n_slate, 1, 3)).any()
    assert dt < 5.0            # a few seconds (a Python loop over the slates takes minutes)


# ------------------------------------------------------------------ the models over a CPU stand-in
class SlateEngine(RecommendingEngine):
    """the recommending stand-in + TowerEngine.rank_slates' contract: the oracle's predictions ordered in numpy (ties by
    ascending id); it records every call's domain and the live weights it ranked with."""
    log = []

    def rank_slates(self, uids, domain, slates, want_order=False):
        uids = np.asarray(uids, np.int32).ravel()
        off, ids = recommend.slates_csr(slates, uids.size)
        type(self).log.append((int(domain), self.weights.numpy().copy()))
        scores, pos = np.zeros(ids.size, np.float32), np.zeros(ids.size, np.int32)
        order = np.full(ids.size, -1, np.int32)
        for q, u in enumerate(uids):
            sl = slice(off[q], off[q + 1])
            it = ids[sl]
            if not it.size:
                continue
            s = self.oracle.predict(np.full(it.size, u, np.int32), it, np.full(it.size, domain, np.int32))
            scores[sl] = s
            pos[sl] = ((s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (it[None, :] < it[:, None]))).sum(1)
            order[off[q] + pos[sl]] = np.arange(it.size)
        res = {"offsets": off, "ids": ids, "scores": scores, "pos": pos}
        if want_order:
            res["order"] = order
        return res


def check_slates(ds, d, r, n_neg):
    """the composition of sampled_eval's slates on domain d -> the number of short ones, counted by hand."""
    test, train, val = (s[d]["data"] for s in (ds.test_dataset, ds.train_dataset, ds.val_dataset))
    catalogue = np.unique(np.concatenate([c["pid"] for c in (train, val, test)]))
    keep = test["label"] > 0
    pairs = np.unique(np.stack([test["uid"][keep], test["pid"][keep]], 1), axis=0)
    off, ids = r["offsets"], r["ids"]
    assert np.array_equal(r["users"], pairs[:, 0]) and np.array_equal(r["positives"], pairs[:, 1])
    assert off.shape == (pairs.shape[0] + 1,) and off[-1] == ids.size == r["scores"].size == r["pos"].size
    assert np.array_equal(ids[off[:-1]], pairs[:, 1])                         # entry 0 is the positive
    assert np.array_equal(r["rank"], r["pos"][off[:-1]]) and np.array_equal(r["slate_len"], np.diff(off))
    n_short = 0
    for s, (u, p) in enumerate(pairs.tolist()):
        neg = ids[off[s] + 1:off[s + 1]]
        seen = np.concatenate([c["pid"][c["uid"] == u] for c in (train, val)])
        mine = test["pid"][(test["uid"] == u) & keep]
        free = np.setdiff1d(catalogue, np.concatenate([seen, mine]))
        assert np.isin(neg, free).all() and np.unique(neg).size == neg.size, (d, u, p)
        assert neg.size == min(n_neg, free.size)
        n_short += neg.size < n_neg
        assert sorted(r["pos"][off[s]:off[s + 1]].tolist()) == list(range(off[s + 1] - off[s]))
    assert r["n_short"] == n_short
    return n_short


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr"])
def test_sampled_eval_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    gh.patch_emb_dim(monkeypatch)
    SlateEngine.log = []
    cfg = gh.tiny_config(tmp_path, name, epochs=2, sampled_eval=20, sampled_eval_ks=[1, 5], sampled_eval_seed=3)
    built = []
    res = cli.main(cfg, SlateEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model = built[0]
    eng, ds = model.model, model.dataset
    assert [d for d, _ in SlateEngine.log] == [0, 1, 2]                  # one call per domain, after the pipeline
    path = os.path.join(model.result_path, "sampled_eval_neg20.npz")
    text = capsys.readouterr().out
    with np.load(path) as z:
        want = {"domains", "ks", "n_neg", "seed", "mrr", "mean_percentile", "hit_rate", "recall", "ndcg", "n_short"}
        want |= {"%s_%d" % (n, d) for d in range(3) for n in ("users", "positives", "offsets", "ids", "scores", "pos", "rank")}
        assert set(z.files) == want
        assert z["domains"].tolist() == [0, 1, 2] and z["ks"].tolist() == [1, 5] and int(z["n_neg"]) == 20 and int(z["seed"]) == 3
        assert z["n_short"].tolist() == [0, 0, 0]
        for d in range(3):
            r = {n: z["%s_%d" % (n, d)] for n in ("users", "positives", "offsets", "ids", "scores", "pos", "rank")}
            r.update(slate_len=np.diff(r["offsets"]), n_short=0)
            assert check_slates(ds, d, r, 20) == 0
            n = r["rank"].size
            m = recommend.rank_metrics(np.arange(n + 1), r["rank"], np.ones(n, bool), r["slate_len"], np.ones(n), [1, 5])
            assert m["mrr"] == z["mrr"][d] and m["hit_rate"].tolist() == z["hit_rate"][d].tolist()
            assert m["ndcg"].tolist() == z["ndcg"][d].tolist()
            line = re.search(r"^%d: MRR (\d\.\d{4}) HitRate@1 (\d\.\d{4}) NDCG@1 \d\.\d{4} HitRate@5 (\d\.\d{4}) .*random ranking: "
                             r"HitRate@1 0\.0476 HitRate@5 0\.2381" % d, text, flags=re.M)
            assert line and [float(x) for x in line.groups()] == [round(m["mrr"], 4), round(m["hit_rate"][0], 4),
                                                                  round(m["hit_rate"][1], 4)]
        assert z["mrr"].max() > 0
    assert "Sampled eval (20 negatives" in text and "sampled_eval_neg20.npz" in text
    # the same seed draws the same slates; rerank is the engine's dict plus the users
    a, b = model.sampled_eval(1, 20, seed=3), model.sampled_eval(1, 20, seed=4)
    with np.load(path) as z:
        assert np.array_equal(a["ids"], z["ids_1"]) and np.array_equal(a["rank"], z["rank_1"])
    assert not np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["positives"], b["positives"])
    rr = model.rerank(2, [4, 2], [[7, 3, 9], [1]])
    assert set(rr) == {"offsets", "ids", "scores", "pos", "users"} and rr["users"].tolist() == [4, 2]
    assert rr["ids"].tolist() == [7, 3, 9, 1] and sorted(rr["pos"][:3].tolist()) == [0, 1, 2] and rr["pos"][3] == 0
    # a domain made too small: more negatives asked for than most users have free items
    n_cat = np.unique(np.concatenate([s[0]["data"]["pid"] for s in (ds.train_dataset, ds.val_dataset, ds.test_dataset)])).size
    short = model.sampled_eval(0, n_cat - 2, seed=0)
    assert check_slates(ds, 0, short, n_cat - 2) > 0
    if name == "mlp":
        # ... and a run whose catalogues are too small for 20 negatives: every slate is short and holds all its user has
        n_log = len(SlateEngine.log)
        small = gh.tiny_config(tmp_path / "small", name, epochs=1, sampled_eval=20)
        small["dataset"]["synthetic"].update(n_item=16)
        cli.main(small, SlateEngine, on_model=built.append)
        tiny = built[1]
        for d in range(3):
            r = tiny.sampled_eval(d, 20)
            assert check_slates(tiny.dataset, d, r, 20) == r["rank"].size > 0
        with np.load(os.path.join(tiny.result_path, "sampled_eval_neg20.npz")) as z:
            assert z["n_short"].tolist() == [tiny.sampled_eval(d, 20)["rank"].size for d in range(3)]
        SlateEngine.log = SlateEngine.log[:n_log]
    SlateEngine.log = SlateEngine.log[:3] + SlateEngine.log[-1:]
    if name == "mlp_meta_mamdr":
        # every domain was ranked under ITS merged best weights; the live vector is back afterwards, byte for byte
        for d, (dom, w) in enumerate(SlateEngine.log[:3]):
            merged = oouter.merge(model.best_shared_weights.numpy(), model.best_domain_weights[d].numpy(),
                                  cfg["train"]["merged_method"])
            assert dom == d and np.array_equal(w, merged), d
        assert len({w.tobytes() for _, w in SlateEngine.log[:3]}) == 3
        live_before = eng.weights.numpy().copy()
        model.sampled_eval(1, 20, seed=3)
        assert eng.weights.numpy().tobytes() == live_before.tobytes()
        assert np.array_equal(SlateEngine.log[-1][1], SlateEngine.log[1][1]) and not np.array_equal(live_before, SlateEngine.log[1][1])
    else:
        assert all(np.array_equal(w, eng.weights.numpy()) for _, w in SlateEngine.log)


# ------------------------------------------------------------------ sampled_report on made-up ranks
class MadeUpModel(object):
    """sampled_report's view of a model: two domains with made-up ranks."""
    class dataset(object):
        test_dataset = {4: None, 2: None}

    def __init__(self, result_path):
        self.result_path = result_path
        self.calls = []

    def sampled_eval(self, domain, n_neg, seed=0):
        self.calls.append((domain, n_neg, seed))
        rank = {2: [0, 3, 9, 1], 4: [5, 0]}[domain]
        lens = {2: [10, 10, 10, 4], 4: [10, 10]}[domain]
        off = np.concatenate([[0], np.cumsum(lens)])
        n = int(off[-1])
        return {"users": np.arange(len(rank)), "positives": np.arange(len(rank)) + 50, "offsets": off, "ids": np.arange(n, dtype=np.int32),
                "scores": np.linspace(0, 1, n).astype(np.float32), "pos": np.zeros(n, np.int32), "rank": np.asarray(rank, np.int32),
                "slate_len": np.asarray(lens), "n_short": int((np.asarray(lens) < n_neg + 1).sum())}


def test_sampled_report_metrics_by_hand(tmp_path, capsys):
    model = MadeUpModel(str(tmp_path / "res"))
    path, metrics = recommend.sampled_report(model, 9, [1, 5], seed=7)
    assert path == os.path.join(str(tmp_path / "res"), "sampled_eval_neg9.npz") and model.calls == [(2, 9, 7), (4, 9, 7)]
    d = lambda r: 1.0 / np.log2(r + 2.0)      # noqa: E731
    m = metrics[2]                            # ranks 0, 3, 9, 1 of one positive each
    assert m["n_eval"] == 4 and m["n_short"] == 1
    assert m["mrr"] == (1.0 + 1 / 4.0 + 1 / 10.0 + 1 / 2.0) / 4
    assert m["hit_rate"].tolist() == [1 / 4.0, 3 / 4.0] and m["recall"].tolist() == m["hit_rate"].tolist()
    assert abs(m["ndcg"][0] - 1 / 4.0) < 1e-15 and abs(m["ndcg"][1] - (d(0) + d(3) + d(1)) / 4) < 1e-15
    assert m["mean_percentile"] == (0 / 9.0 + 3 / 9.0 + 9 / 9.0 + 1 / 3.0) / 4
    want = recommend.rank_metrics(np.arange(3), [5, 0], [True, True], [10, 10], [1, 1], [1, 5])
    assert metrics[4]["mrr"] == want["mrr"] and metrics[4]["hit_rate"].tolist() == want["hit_rate"].tolist() == [0.5, 0.5]
    with np.load(path) as z:
        keys = {"domains", "ks", "n_neg", "seed", "mrr", "mean_percentile", "hit_rate", "recall", "ndcg", "n_short"}
        keys |= {"%s_%d" % (n, dd) for dd in (2, 4) for n in ("users", "positives", "offsets", "ids", "scores", "pos", "rank")}
        assert set(z.files) == keys
        assert z["domains"].tolist() == [2, 4] and z["ks"].tolist() == [1, 5] and int(z["n_neg"]) == 9 and int(z["seed"]) == 7
        assert z["hit_rate"].shape == (2, 2) and z["hit_rate"][0].tolist() == m["hit_rate"].tolist() and z["mrr"][0] == m["mrr"]
        assert z["n_short"].tolist() == [1, 0] and z["rank_2"].tolist() == [0, 3, 9, 1] and z["offsets_4"].tolist() == [0, 10, 20]
    text = capsys.readouterr().out
    assert re.search(r"^2: MRR 0\.4625 HitRate@1 0\.2500 NDCG@1 0\.2500 HitRate@5 0\.7500 .*4 pairs, 1 short slates; random ranking: "
                     r"HitRate@1 0\.1000 HitRate@5 0\.5000", text, flags=re.M)
    out = str(tmp_path / "elsewhere" / "x.npz")
    assert recommend.sampled_report(model, 9, [1], seed=0, out_path=out)[0] == out and os.path.exists(out)


# ------------------------------------------------------------------ the command line
def test_cli_flags_set_the_config_keys(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--sampled-eval"])
    cli.cli(["--config", cfg_path, "--sampled-eval", "49", "--sampled-eval-ks", "5,10,20"])
    cli.cli(["--config", cfg_path, "--sampled-eval", "7", "--recommend", "10"])
    train = seen[0][0][0]["train"]
    assert seen[0][1] == {} and len(seen[0][0]) == 1 and not any(k.startswith("sampled_eval") for k in train)
    assert seen[1][1] == {} and len(seen[1][0]) == 1 and seen[1][0][0]["train"]["sampled_eval"] == 99
    assert "sampled_eval_ks" not in seen[1][0][0]["train"]
    assert seen[2][1] == {} and seen[2][0][0]["train"]["sampled_eval"] == 49
    assert seen[2][0][0]["train"]["sampled_eval_ks"] == [5, 10, 20]
    assert seen[3][1] == {"recommend": 10, "recommend_out": None} and seen[3][0][0]["train"]["sampled_eval"] == 7
    with pytest.raises(SystemExit):
        cli.cli(["--config", cfg_path, "--sampled-eval", "0"])
    with pytest.raises(SystemExit):                      # the list of K alone would be set and never read
        cli.cli(["--config", cfg_path, "--sampled-eval-ks", "5,10"])
    assert len(seen) == 4


def test_lanes_refuse_sampled_eval_by_name(tmp_path, monkeypatch):
    gh.patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", sampled_eval=99, lanes=2)
    with pytest.raises(NotImplementedError, match=r"train\.sampled_eval"):
        cli.main(cfg, SlateEngine)
    assert not loaded                    # refused before the data is loaded
