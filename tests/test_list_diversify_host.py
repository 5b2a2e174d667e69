"""Diversified re-ranking of top-K lists (greedy MMR), host side (no GPU): the C ABI's declaration, binding and export, the
refusals that need no device, the float64 definition `list_metrics.diversify_host` on hand-worked cases, the fp32 replay
against it, the min-max relevance at its edges, the command line, and `BaseModel.diversify` / `run.py --diversify` end to end
over a CPU stand-in whose `list_diversify` is the host definition."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from mamdr_amd import _lib, cli
from mamdr_amd import list_metrics as lm
from test_list_metrics_host import ListEngine, _np
from test_recommend_host import RecommendingEngine, patch_emb_dim, tiny_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------ C ABI
def test_the_call_is_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+mamdr_list_diversify\s*\(([^;]*)\)\s*;", header)
    assert m, "mamdr_list_diversify is not declared in include/mamdr_hip.h"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "const int32_t* d_ids", "const float* d_rel", "int32_t n_list", "int32_t n", "int32_t k", "float lambda",
        "const float* d_rows", "int64_t n_rows", "int32_t emb_dim", "int32_t* d_pos_out", "float* d_value_out", "void* stream"]
    # declared beside mamdr_list_similarity, and the header says that the reference has nothing of the kind
    assert header.index("mamdr_list_similarity") < header.index("mamdr_list_diversify") < header.index("mamdr_interp")
    assert "NO REFERENCE COUNTERPART" in text[:text.index("int mamdr_list_diversify")].rsplit("/*", 1)[1]
    vp, i32, i64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert _lib.SIGNATURES["mamdr_list_diversify"] == (C.c_int, [vp, vp, i32, i32, i32, f, vp, i64, i32, vp, vp, vp])
    lib = _lib.load()
    assert hasattr(lib, "mamdr_list_diversify")
    # a new entry point only: the version stays
    assert _lib.ABI_VERSION == 19 and lib.mamdr_abi_version() == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    p = C.c_void_p(1 << 20)               # an aligned non-null address: a refusal never dereferences it
    odd4, odd16 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)

    def call(ids=p, rel=p, n_list=1, n=4, k=2, lam=0.5, rows=p, n_rows=5, emb=32, pos=p, val=p):
        return lib.mamdr_list_diversify(ids, rel, n_list, n, k, lam, rows, n_rows, emb, pos, val, None)

    for kw, word in ((dict(ids=None), b"null"), (dict(rel=None), b"null"), (dict(rows=None), b"null"), (dict(pos=None), b"null"),
                     (dict(ids=odd4), b"aligned"), (dict(rel=odd4), b"aligned"), (dict(pos=odd4), b"aligned"),
                     (dict(val=odd4), b"aligned"), (dict(rows=odd16), b"aligned"),
                     (dict(n_list=0), b"n_list"), (dict(n_list=-3), b"n_list"),
                     (dict(n=0, k=1), b"n 0"), (dict(n=129, k=1), b"n 129"),
                     (dict(k=0), b"k 0"), (dict(k=5), b"k 5"),
                     (dict(emb=96), b"emb_dim 96"), (dict(emb=16), b"emb_dim 16"), (dict(n_rows=0), b"n_rows"),
                     (dict(lam=-0.01), b"lambda"), (dict(lam=1.5), b"lambda"), (dict(lam=float("nan")), b"lambda")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.mamdr_last_error(), (kw, lib.mamdr_last_error())
    with pytest.raises(_lib.MamdrError):
        _lib.check(call(k=0))


# ------------------------------------------------------------------ the float64 definition, hand-worked
#        0: e0     1: e0 again  2: e1      3: zero   4: e2      5: e3      6: e0 + e1
ROWS = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0]], np.float32)


def test_two_identical_rows_and_one_orthogonal():
    ids, rel = np.array([[0, 1, 2]]), np.array([[0.875, 0.75, 0.125]], np.float32)
    pos, val = lm.diversify_host(ids, rel, ROWS, 3, 1.0)           # relevance alone
    assert pos.tolist() == [[0, 1, 2]] and val.tolist() == [[0.875, 0.75, 0.125]]
    pos, val = lm.diversify_host(ids, rel, ROWS, 3, 0.5)           # the copy (cos 1) falls behind the orthogonal row
    assert pos.tolist() == [[0, 2, 1]]
    assert val.tolist() == [[0.875, 0.5 * 0.125 - 0.5 * 0.0, 0.5 * 0.75 - 0.5 * 1.0]]
    pos, val = lm.diversify_host(ids, rel, ROWS, 3, 0.0)           # similarity alone (step 0 is still the most relevant)
    assert pos.tolist() == [[0, 2, 1]] and val.tolist() == [[0.875, 0.0, -1.0]]
    pos, val = lm.diversify_host(ids, rel, ROWS, 2, 0.5)           # k < L: a prefix
    assert pos.tolist() == [[0, 2]] and pos.dtype == np.int32 and val.dtype == np.float64
    # the running maximum: behind e0 and e1, e0 + e1 (cos 1 / sqrt 2 with both) stands at -m; e2 at 0
    pos, val = lm.diversify_host(np.array([[0, 2, 6, 4]]), np.array([[1.0, 0.5, 0.5, 0.0]], np.float32), ROWS, 4, 0.5)
    assert pos.tolist() == [[0, 1, 3, 2]]
    assert val[0, :3].tolist() == [1.0, 0.25, 0.0] and val[0, 3] == pytest.approx(0.25 - 0.5 / np.sqrt(2.0), abs=1e-15)


def test_equal_values_go_by_ascending_id_and_nan_goes_last():
    ids = np.array([[5, 2, 4]])
    pos, val = lm.diversify_host(ids, np.full((1, 3), 0.5, np.float32), ROWS, 3, 1.0)
    assert pos.tolist() == [[1, 2, 0]]
    pos, _ = lm.diversify_host(ids, np.full((1, 3), 0.5, np.float32), ROWS, 3, 0.5)     # all orthogonal: still a tie every step
    assert pos.tolist() == [[1, 2, 0]]
    pos, val = lm.diversify_host(ids, np.array([[np.nan, -np.inf, 0.25]], np.float32), ROWS, 3, 1.0)
    assert pos.tolist() == [[2, 1, 0]] and val[0, 1] == -np.inf and np.isnan(val[0, 2])


def test_a_zero_norm_row_has_cosine_zero():
    ids, rel = np.array([[0, 3, 1]]), np.array([[1.0, 0.5, 0.75]], np.float32)
    pos, val = lm.diversify_host(ids, rel, ROWS, 3, 0.5)
    assert pos.tolist() == [[0, 1, 2]] and val.tolist() == [[1.0, 0.25, 0.375 - 0.5]]
    short, margin = lm.diversify_audit(ids, rel, ROWS, pos, 0.5)
    assert short.tolist() == [[0.0, 0.0, 0.0]] and margin.tolist() == [[0.25, 0.375, np.inf]]


def test_padding_and_short_lists():
    ids = np.array([[-1, 7, 99, -5],                  # all padding (n_rows = 7)
                    [-1, 2, 7, 0],                    # two valid entries, at positions 1 and 3
                    [4, -1, -1, -1]])
    rel = np.array([[1, 1, 1, 1], [9, 0.25, 9, 0.5], [0.5, 9, 9, 9]], np.float32)
    pos, val = lm.diversify_host(ids, rel, ROWS, 3, 0.5)
    assert pos.tolist() == [[-1, -1, -1], [3, 1, -1], [0, -1, -1]]
    assert val.tolist() == [[0, 0, 0], [0.5, 0.125, 0], [0.5, 0, 0]]
    cos = [np.zeros((0, 0), np.float32), np.zeros((2, 2), np.float32), np.zeros((1, 1), np.float32)]
    rpos, rval = lm.diversify_replay(ids, rel, cos, 3, 0.5, n_rows=7)
    assert rpos.tolist() == pos.tolist() and rval.tolist() == val.tolist() and rval.dtype == np.float32
    for bad in (dict(k=0), dict(k=5), dict(lam=1.5), dict(lam=-0.5)):
        with pytest.raises(ValueError):
            lm.diversify_host(ids, rel, ROWS, bad.get("k", 2), bad.get("lam", 0.5))
    with pytest.raises(ValueError):
        lm.diversify_host(ids, rel[:, :3], ROWS, 2, 0.5)


def test_rank_keys_order_as_the_device_key():
    v = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-30, 1.0, np.inf], np.float32)
    keys = lm.rank_keys(v, np.full(v.shape, 3))
    assert np.all(np.diff(keys.astype(np.float64)) > 0) and keys[0] >> np.uint64(32) == 1 and np.all(keys > 0)
    assert lm.rank_keys([0.5, 0.5], [2, 7])[0] > lm.rank_keys([0.5, 0.5], [2, 7])[1]          # the smaller id ranks first


# ------------------------------------------------------------------ the fp32 replay against the definition
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
def test_replay_agrees_with_the_definition_where_the_margin_is_wide(lam):
    rng = np.random.default_rng(11)
    E, n, k, Q = 16, 24, 10, 60
    rows = rng.standard_normal((300, E)).astype(np.float32)
    ids = np.stack([rng.choice(300, n, replace=False) for _ in range(Q)])
    ids[rng.random(ids.shape) < 0.1] = -1
    rel = (1.0 / (1.0 + np.exp(-rng.normal(-1.0, 1.0, ids.shape)))).astype(np.float32)
    pos, val = lm.diversify_host(ids, rel, rows, k, lam)
    cos = []
    for row in ids:
        x = rows[row[row >= 0]].astype(np.float64)
        norm = np.sqrt((x * x).sum(1))
        cos.append(((x @ x.T) / (norm[:, None] * norm[None, :])).astype(np.float32))       # fp32-rounded float64 cosines
    rpos, rval = lm.diversify_replay(ids, rel, cos, k, lam)
    short, margin = lm.diversify_audit(ids, rel, rows, pos, lam)
    assert np.all(short == 0.0)                                    # the definition's own picks are best at every step
    tol = 8 * 2.0 ** -24                                           # (rounded cosines, three roundings of the value)
    wide = (margin > 2 * tol).all(axis=1)
    assert wide.mean() >= 0.9
    assert np.array_equal(rpos[wide], pos[wide])
    assert np.abs(rval[wide] - val[wide]).max() <= tol
    # and the replay's picks are never worse than 2 tol in float64
    assert lm.diversify_audit(ids, rel, rows, rpos, lam)[0].max() <= 2 * tol


def test_tolerance_formula():
    assert lm.diversify_tol(128, 0.7) == ((1.0 - 0.7) * (2 * 128 + 8) + 8) * 2.0 ** -24
    assert lm.diversify_tol(32, 1.0) == 8 * 2.0 ** -24
    assert lm.diversify_tol(64, 0.0) == lm.error_bound(64) + 8 * 2.0 ** -24


# ------------------------------------------------------------------ the relevance
def test_minmax_relevance_at_its_edges():
    ids = np.array([[3, 1, -1, 9],                    # 9 is outside n_rows = 5: padding, like -1
                    [2, 2, 2, 2],                     # hi == lo
                    [-1, -1, -1, -1],                 # nothing valid
                    [0, -1, -1, -1]])                 # one entry
    s = np.array([[0.75, 0.25, 100.0, -100.0], [0.5, 0.5, 0.5, 0.5], [1, 2, 3, 4], [0.3, 0, 0, 0]], np.float32)
    rel = lm.minmax_relevance(s, ids, 5)
    assert rel.dtype == np.float32 and rel.tolist() == [[1.0, 0.0, 0.0, 0.0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    s = np.array([[0.9, 0.3, 0.5]], np.float32)
    rel = lm.minmax_relevance(s, np.array([[0, 1, 2]]), 5)
    assert rel[0, 2] == (np.float32(0.5) - np.float32(0.3)) / (np.float32(0.9) - np.float32(0.3)) and rel[0, 0] == 1 and rel[0, 1] == 0
    with pytest.raises(ValueError):
        lm.minmax_relevance(s, np.array([[0, 1]]), 5)


# ------------------------------------------------------------------ the command line
def test_flags_parse(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--diversify"])
    cli.cli(["--config", cfg_path, "--recommend", "7", "--diversify", "0.25", "--diversify-pool", "40", "--diversify-out", "d.npz"])
    train = [s[0][0]["train"] for s in seen]
    assert not any(key.startswith("diversify") for key in train[0])
    assert train[1]["diversify"] == 0.7 and "diversify_pool" not in train[1] and seen[1][1] == {}
    assert train[2]["diversify"] == 0.25 and train[2]["diversify_pool"] == 40 and train[2]["diversify_out"] == "d.npz"
    assert seen[2][1] == {"recommend": 7, "recommend_out": None}
    for bad in (["--diversify", "1.5"], ["--diversify", "-0.1"], ["--diversify", "nan"], ["--diversify-pool", "40"],
                ["--diversify", "--diversify-pool", "9"], ["--diversify", "--diversify-pool", "129"],
                ["--diversify", "--recommend", "200"]):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path] + bad)
    assert "--diversify [LAMBDA]" in cli.__doc__ and "--diversify-pool" in cli.__doc__ and "--diversify-out" in cli.__doc__
    assert lm.check_pool(10) == (10, 50) and lm.check_pool(30) == (30, 128) and lm.check_pool(10, 10) == (10, 10)


def test_several_lanes_are_refused(tmp_path):
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr")
    cfg["train"].update(lanes=2, diversify=0.7)
    with pytest.raises(NotImplementedError, match=r"train\.diversify \(run\.py --diversify\).*not computed across processes "
                                                  r"or lanes.*one process"):
        cli.main(cfg, RecommendingEngine)


# ------------------------------------------------------------------ BaseModel.diversify and the report over a CPU stand-in
class DiversifyEngine(ListEngine):
    """ListEngine + `list_diversify` as its host definition (positions, and the values in fp32)."""
    def list_diversify(self, ids, rel, rows, k, lam, want_values=False):
        pos, val = lm.diversify_host(_np(ids), _np(rel), _np(rows), k, lam)
        return pos, (val.astype(np.float32) if want_values else None)


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr_finetune", "mlp_pcgrad"])
def test_diversify_and_its_report_end_to_end_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    out = str(tmp_path / "div.npz")
    cfg["train"].update(diversify=0.5, diversify_pool=20, diversify_out=out)
    built = []
    res = cli.main(cfg, DiversifyEngine, on_model=built.append, recommend=5)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model = built[0]
    text = capsys.readouterr().out
    live = model.model.weights.numpy().copy()
    rows = np.asarray(model.model.oracle.params["item_emb"], np.float32)
    figures = lm.ACCURACY + lm.FIGURES
    with np.load(out) as z:
        assert z["domains"].tolist() == [0, 1, 2] and int(z["k"]) == 5 and int(z["pool"]) == 20 and float(z["lambda"]) == 0.5
        for key in figures:
            for side in ("", "_diversified"):
                assert z[key + side].shape == (3,) and np.all(np.isfinite(z[key + side])), key + side
        for d in range(3):
            Q = np.unique(model.dataset.test_dataset[d]["data"]["uid"]).size
            assert z["users_%d" % d].shape == (Q,)
            for key in ("base_ids", "ids", "pos", "values"):
                assert z["%s_%d" % (key, d)].shape == (Q, 5), key
            assert re.search(r"^%d: HitRate@5 \d\.\d{4} -> \d\.\d{4} NDCG@5 \d\.\d{4} -> \d\.\d{4} ILD " % d, text, flags=re.M)
        if "mamdr" not in name:           # the live weights produced the lists
            for d in range(3):
                r = model.diversify(d, 5, 20, 0.5)
                base, pool = model.recommend(d, 5), model.recommend(d, 20)
                assert np.array_equal(r["base_ids"], base["ids"]) and np.array_equal(r["pool_ids"], pool["ids"])
                assert np.array_equal(r["users"], base["users"]) and r["catalogue"] == base["catalogue"]
                assert np.array_equal(z["ids_%d" % d], r["ids"]) and np.array_equal(z["base_ids_%d" % d], base["ids"])
                # the picks are the definition's on the min-max relevance of the pool
                rel = lm.minmax_relevance(pool["scores"], pool["ids"], rows.shape[0])
                pos, val = lm.diversify_host(pool["ids"], rel, rows, 5, 0.5)
                assert np.array_equal(r["pos"], pos) and np.array_equal(r["values"], val.astype(np.float32))
                assert np.array_equal(r["ids"], np.take_along_axis(pool["ids"], pos.astype(np.int64), 1))
                assert np.array_equal(r["scores"], np.take_along_axis(pool["scores"], pos.astype(np.int64), 1))
                assert np.all(r["pos"][:, 0] == 0)                 # step 0 is the most relevant entry
                # every figure of both sides is summarise / ranking_metrics over the host route
                from mamdr_amd import recommend as rec
                positives = rec.split_positives(model.dataset, d, r["users"])
                tr = model.dataset.train_dataset[d]["data"]
                pop = np.bincount(tr["pid"][tr["label"] > 0], minlength=model.n_pid)
                cat = np.unique(np.concatenate([s[d]["data"]["pid"] for s in (
                    model.dataset.train_dataset, model.dataset.val_dataset, model.dataset.test_dataset)]))
                for side, lists in (("", base["ids"]), ("_diversified", r["ids"])):
                    sim, pairs = lm.list_similarity_host(lists, rows)
                    want = lm.summarise(lm.id_counts_host(lists, model.n_pid), pop, cat, 5, sim, pairs, n_lists=lists.shape[0])
                    want.update(rec.ranking_metrics(lists, positives))
                    for key in figures:
                        assert z[key + side][d] == want[key], key + side
                # lambda = 1 on the scores as they are: the base lists
                same = model.diversify(d, 5, 20, 1.0, relevance="score")
                assert np.array_equal(same["ids"], base["ids"]) and np.array_equal(same["scores"], base["scores"])
                assert np.array_equal(same["pos"], np.tile(np.arange(5, dtype=np.int32), (base["ids"].shape[0], 1)))
            # trading relevance for dissimilarity does not lower the intra-list diversity of these lists
            assert np.all(z["ild_diversified"] >= z["ild"])
    with pytest.raises(ValueError):
        model.diversify(0, 5, 20, 0.5, relevance="rank")
    with pytest.raises(ValueError):
        model.diversify(0, 5, 4, 0.5)
    # the report reads state only
    assert np.array_equal(model.model.weights.numpy(), live)
    # result.json carries the headline
    rdir = os.path.join(str(tmp_path / "result"), name, "Taobao", cfg["dataset"]["domain_split_path"])
    run = [p for p in os.listdir(rdir) if os.path.isdir(os.path.join(rdir, p))]
    assert len(run) == 1
    with open(os.path.join(rdir, run[0], "result.json")) as f:
        result = json.load(f)
    assert result["diversify_lambda"] == 0.5 and result["diversify_pool"] == 20
    with np.load(out) as z:
        for key in figures:
            assert set(result["domain_%s_diversified" % key]) == {"0", "1", "2"}
            assert result["domain_%s_diversified" % key]["1"] == float(z[key + "_diversified"][1])
        for key in lm.AVERAGED + ("ndcg",):
            assert result["avg_%s_diversified" % key] == pytest.approx(float(np.mean(z[key + "_diversified"])))
    assert len(result) > 2 + len(figures) + len(lm.AVERAGED) + 1          # (save_result's own keys are still there)


def test_default_pool_and_path_and_no_flag_no_file(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "wdl", epochs=1)
    cfg["train"]["diversify"] = 0.7
    cli.main(cfg, DiversifyEngine)
    rdir = os.path.join(str(tmp_path / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert "diversify_top10.npz" in os.listdir(rdir)
    with np.load(os.path.join(rdir, "diversify_top10.npz")) as z:
        assert int(z["k"]) == 10 and int(z["pool"]) == 50 and float(z["lambda"]) == 0.7
    cli.main(tiny_config(tmp_path / "b", "wdl", epochs=1), DiversifyEngine)
    rdir = os.path.join(str(tmp_path / "b" / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert not [p for p in os.listdir(rdir) if p.endswith(".npz")]
