"""Similar items (exact cosine nearest neighbours), host side (no GPU): the C ABI's declaration, binding and export, the
refusals that need no device, the float64 definition `neighbours.neighbours_host` and the replay on hand-worked rows,
`neighbours.summarise` on a hand-built graph, the command line, and `BaseModel.similar_items` / `run.py --similar-items`
end to end over a CPU stand-in whose `row_neighbours` is the host definition."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from mamdr_amd import _lib, cli
from mamdr_amd import list_metrics as lm
from mamdr_amd import neighbours as nb
from test_list_metrics_host import ListEngine, _np
from test_recommend_host import RecommendingEngine, patch_emb_dim, tiny_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ARGS = ["const float* d_rows", "int64_t n_rows", "int32_t emb_dim", "const int32_t* d_query", "int32_t n_query",
        "const int32_t* d_cand", "int64_t n_cand", "int32_t exclude_self", "int32_t k", "int32_t* d_ids_out", "float* d_sim_out"]


# ------------------------------------------------------------------ C ABI
def test_the_calls_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, tail in (("mamdr_row_neighbours", ["void* stream"]), ("mamdr_row_neighbours_bounded", ["int32_t chunk", "void* stream"])):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/mamdr_hip.h" % name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == ARGS + tail
        assert hasattr(_lib.load(), name)
    assert header.index("mamdr_list_diversify") < header.index("mamdr_row_neighbours") < header.index("mamdr_interp")
    assert re.search(r"#define\s+MAMDR_KNN_MAX_K\s+128\b", header) and _lib.KNN_MAX_K == nb.MAX_K == 128
    assert "NO REFERENCE COUNTERPART" in text[:text.index("int mamdr_row_neighbours")].rsplit("/*", 1)[1]
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    head = [vp, i64, i32, vp, i32, vp, i64, i32, i32, vp, vp]
    assert _lib.SIGNATURES["mamdr_row_neighbours"] == (C.c_int, head + [vp])
    assert _lib.SIGNATURES["mamdr_row_neighbours_bounded"] == (C.c_int, head + [i32, vp])
    # new entry points only: the version stays
    assert _lib.ABI_VERSION == 19 and _lib.load().mamdr_abi_version() == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    p = C.c_void_p(1 << 20)               # an aligned non-null address: a refusal never dereferences it
    odd4, odd16 = C.c_void_p((1 << 20) + 2), C.c_void_p((1 << 20) + 4)

    def call(rows=p, n_rows=5, emb=32, query=p, n_query=2, cand=p, n_cand=4, excl=1, k=2, ids=p, sims=p, chunk=None):
        head = (rows, n_rows, emb, query, n_query, cand, n_cand, excl, k, ids, sims)
        if chunk is None:
            return lib.mamdr_row_neighbours(*head, None)
        return lib.mamdr_row_neighbours_bounded(*head, chunk, None)

    cases = ((dict(rows=None), b"null"), (dict(query=None), b"null"), (dict(ids=None), b"null"), (dict(sims=None), b"null"),
             (dict(rows=odd16), b"d_rows is not 16-byte aligned"), (dict(query=odd4), b"4-byte aligned"),
             (dict(cand=odd4), b"4-byte aligned"), (dict(ids=odd4), b"4-byte aligned"), (dict(sims=odd4), b"4-byte aligned"),
             (dict(n_rows=0), b"n_rows 0"), (dict(n_rows=-1), b"n_rows -1"), (dict(n_rows=2 ** 31), b"n_rows 2147483648"),
             (dict(emb=96), b"emb_dim 96"), (dict(emb=16), b"emb_dim 16"), (dict(emb=512), b"emb_dim 512"),
             (dict(n_query=0), b"n_query 0"), (dict(n_query=-2), b"n_query -2"),
             (dict(n_cand=0), b"n_cand 0"), (dict(n_cand=-4), b"n_cand -4"), (dict(cand=None, n_cand=4), b"null d_cand"),
             (dict(k=0), b"k 0"), (dict(k=129), b"k 129"))
    for chunk in (None, 64):
        for kw, word in cases:
            assert call(chunk=chunk, **kw) == _lib.EINVAL, kw
            err = lib.mamdr_last_error()
            assert word in err and (b"mamdr_row_neighbours_bounded:" in err) == (chunk is not None), (kw, err)
    for chunk in (0, -64):
        assert call(chunk=chunk) == _lib.EINVAL and b"chunk" in lib.mamdr_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(call(k=0))


# ------------------------------------------------------------------ the float64 definition, hand-worked
#        0: e0     1: e0 again  2: e1      3: zero   4: e0 + e1   5: 2 e0      6: -e0
ROWS = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [2, 0, 0, 0], [-1, 0, 0, 0]], np.float32)
R2 = 1.0 / np.sqrt(2.0)


def test_identical_rows_tie_by_ascending_id():
    ids, sims = nb.neighbours_host(ROWS, [0], 6)
    assert ids.tolist() == [[1, 5, 4, 2, 3, 6]] and ids.dtype == np.int32 and sims.dtype == np.float64
    assert sims[0, :2].tolist() == [1.0, 1.0] and sims[0, 2] == pytest.approx(R2, abs=1e-15) and sims[0, 3:].tolist() == [0.0, 0.0, -1.0]
    ids, _ = nb.neighbours_host(ROWS, [5, 1], 2)
    assert ids.tolist() == [[0, 1], [0, 5]]
    # the candidates' order is nothing: the same lists from a permuted candidate list
    perm = [6, 2, 5, 0, 3, 1, 4]
    assert nb.neighbours_host(ROWS, [0, 4], 6, perm)[0].tolist() == nb.neighbours_host(ROWS, [0, 4], 6)[0].tolist()


def test_a_zero_row_has_cosine_zero():
    ids, sims = nb.neighbours_host(ROWS, [3], 7)
    assert ids.tolist() == [[0, 1, 2, 4, 5, 6, -1]] and not sims.any()
    ids, sims = nb.neighbours_host(ROWS, [2], 3)               # e1: e0 + e1 first, then the zeros by id
    assert ids.tolist() == [[4, 0, 1]] and sims[0, 1:].tolist() == [0.0, 0.0]


def test_self_exclusion_short_lists_and_ids_out_of_range():
    ids, sims = nb.neighbours_host(ROWS, [0], 2, exclude_self=False)
    assert ids.tolist() == [[0, 1]] and sims.tolist() == [[1.0, 1.0]]
    ids, sims = nb.neighbours_host(ROWS, [0], 2, [0], exclude_self=True)         # the only candidate is the query
    assert ids.tolist() == [[-1, -1]] and sims.tolist() == [[0.0, 0.0]]
    ids, sims = nb.neighbours_host(ROWS, [0, 6], 4, [6, 1])                       # a short list is padded
    assert ids.tolist() == [[1, 6, -1, -1], [1, -1, -1, -1]] and sims.tolist() == [[1.0, -1.0, 0, 0], [-1.0, 0, 0, 0]]
    ids, sims = nb.neighbours_host(ROWS, [-1, 7, 2 ** 31 - 1, 0], 2)             # a query id out of range: all padding
    assert ids.tolist() == [[-1, -1]] * 3 + [[1, 5]] and not sims[:3].any()
    ids, sims = nb.neighbours_host(ROWS, [0], 4, [7, -1, 2, 2 ** 31 - 1, 5])     # a candidate id out of range: never returned
    assert ids.tolist() == [[5, 2, -1, -1]]
    for bad in (0, 129):
        with pytest.raises(ValueError):
            nb.neighbours_host(ROWS, [0], bad)


def test_replay_orders_by_the_device_key():
    nan = np.nan
    cos = np.array([[0.5, nan, 0.5, -0.0, 0.0, 1.0, -1.0]], np.float32)
    ids, sims = nb.neighbours_replay(cos, [3], 7)                                 # (query 3: its own column is skipped)
    assert ids.tolist() == [[5, 0, 2, 4, 6, 1, -1]] and sims.dtype == np.float32
    assert sims[0, :5].tolist() == [1.0, 0.5, 0.5, 0.0, -1.0] and np.isnan(sims[0, 5]) and sims[0, 6] == 0.0
    ids, _ = nb.neighbours_replay(cos, [3], 7, exclude_self=False)                # -0.0 stands behind +0.0
    assert ids.tolist() == [[5, 0, 2, 4, 3, 6, 1]]
    ids, _ = nb.neighbours_replay(cos[:, :3], [9], 2, [8, 400, 2], n_rows=300)
    assert ids.tolist() == [[2, 8]]
    # on fp32-rounded float64 cosines the replay is the definition wherever no two cosines round together
    rows = np.random.default_rng(5).standard_normal((40, 8)).astype(np.float32)
    want_ids, want_sims = nb.neighbours_host(rows, np.arange(40), 5)
    x = rows.astype(np.float64)
    n = np.sqrt((x * x).sum(1))
    got_ids, got_sims = nb.neighbours_replay(((x @ x.T) / (n[:, None] * n[None, :])).astype(np.float32), np.arange(40), 5)
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_sims, want_sims.astype(np.float32))
    with pytest.raises(ValueError):
        nb.neighbours_replay(cos, [3, 4], 2)


# ------------------------------------------------------------------ the figures of a hand-built graph
def test_summarise_on_a_hand_built_graph():
    # catalogue 10 .. 14, k = 2: 10 <-> 11 mutual, everybody lists 10, 14 is listed by nobody
    items = [10, 11, 12, 13, 14]
    ids = np.array([[11, 12], [10, 12], [10, 11], [10, 12], [10, 13]])
    sims = np.array([[0.9, 0.5], [0.9, 0.4], [0.5, 0.4], [0.3, 0.2], [0.1, 0.0]])
    deg = lm.id_counts_host(ids, 20)
    assert deg[10:15].tolist() == [4, 2, 3, 1, 0]
    m = nb.summarise(items, ids, sims, items, deg, 2)
    assert m["n_items"] == 5 and m["n_edges"] == 10 and m["k_eff"] == 2
    assert m["mean_sim_1"] == pytest.approx((0.9 + 0.9 + 0.5 + 0.3 + 0.1) / 5) and m["mean_sim_k"] == pytest.approx(1.5 / 5)
    d = np.array([4, 2, 3, 1, 0], np.float64) - 2.0
    assert m["hubness"] == pytest.approx((d ** 3).mean() / (d ** 2).mean() ** 1.5) and m["hubness"] == 0.0      # symmetric degrees
    assert m["orphan_share"] == 0.2 and m["max_in_degree"] == 4
    # mutual pairs: 10-11, 10-12, 11-12 -> 6 of the 10 edges have their reverse
    assert m["reciprocity"] == 0.6
    # one hub: positive skewness; equal degrees: zero variance -> 0.0
    hub = nb.summarise([0, 1, 2, 3], np.array([[3], [3], [3], [0]]), np.ones((4, 1)), [0, 1, 2, 3], [1, 0, 0, 3], 1)
    assert hub["hubness"] > 0 and hub["orphan_share"] == 0.5 and hub["reciprocity"] == 0.5
    ring = nb.summarise([0, 1, 2], np.array([[1], [2], [0]]), np.ones((3, 1)), [0, 1, 2], [1, 1, 1], 1)
    assert ring["hubness"] == 0.0 and ring["orphan_share"] == 0.0 and ring["reciprocity"] == 0.0
    # k beyond the catalogue: the k'-th neighbour is the last one there can be; short lists have no k'-th
    short = nb.summarise([0, 1], np.array([[1, -1, -1], [0, -1, -1]]), np.array([[0.5, 0, 0], [0.5, 0, 0]]), [0, 1], [1, 1], 3)
    assert short["k_eff"] == 1 and short["mean_sim_1"] == short["mean_sim_k"] == 0.5 and short["reciprocity"] == 1.0
    lone = nb.summarise([4], np.array([[-1, -1]]), np.zeros((1, 2)), [4], [0, 0, 0, 0, 0], 2)
    assert lone["k_eff"] == 0 and lone["mean_sim_1"] == 0.0 and lone["n_edges"] == 0 and lone["orphan_share"] == 1.0
    for bad in (dict(catalogue=[]), dict(catalogue=[99]), dict(k=1)):
        with pytest.raises(ValueError):
            nb.summarise(items, ids, sims, bad.get("catalogue", items), deg, bad.get("k", 2))
    h = nb.headline({0: dict(m, affinity={0: 0.5, 1: 0.25}), 1: dict(hub, affinity={0: 0.1, 1: 1.0})})
    assert h["domain_hubness"] == {"0": 0.0, "1": hub["hubness"]} and h["avg_orphan_share"] == pytest.approx(0.35)
    assert h["domain_affinity"] == {"0": {"0": 0.5, "1": 0.25}, "1": {"0": 0.1, "1": 1.0}} and "avg_max_in_degree" not in h
    assert nb.headline({})["avg_hubness"] == 0.0


# ------------------------------------------------------------------ the command line
def test_flags_parse(monkeypatch):
    seen = []
    assert "--similar-items [K]" in cli.__doc__ and "--similar-items-out" in cli.__doc__ and "train.similar_items" in cli.main.__doc__
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--similar-items"])
    cli.cli(["--config", cfg_path, "--similar-items", "25", "--similar-items-out", "s.npz", "--recommend", "7"])
    train = [s[0][0]["train"] for s in seen]
    assert not any(key.startswith("similar_items") for key in train[0]) and seen[0][1] == {}
    assert train[1]["similar_items"] == 10 and "similar_items_out" not in train[1] and seen[1][1] == {}
    assert train[2]["similar_items"] == 25 and train[2]["similar_items_out"] == "s.npz"
    assert seen[2][1] == {"recommend": 7, "recommend_out": None}
    for bad in ("0", "129", "-3"):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path, "--similar-items", bad])


def test_several_lanes_are_refused(tmp_path):
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr")
    cfg["train"].update(lanes=2, similar_items=5)
    with pytest.raises(NotImplementedError, match=r"train\.similar_items \(run\.py --similar-items\).*not computed across processes "
                                                  r"or lanes.*one process"):
        cli.main(cfg, RecommendingEngine)


# ------------------------------------------------------------------ BaseModel.similar_items and the report over a CPU stand-in
class NeighbourEngine(ListEngine):
    """ListEngine + `row_neighbours` as its host definition (the cosines in fp32)."""
    def row_neighbours(self, rows, queries, k, candidates=None, exclude_self=True, chunk=None):
        ids, sims = nb.neighbours_host(_np(rows), _np(queries), k, None if candidates is None else _np(candidates), exclude_self)
        return ids, sims.astype(np.float32)


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr_finetune", "mlp_pcgrad"])
def test_similar_items_and_the_report_end_to_end_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    out = str(tmp_path / "knn.npz")
    cfg["train"].update(similar_items=4, similar_items_out=out)
    built = []
    NeighbourEngine.log = []
    res = cli.main(cfg, NeighbourEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model, ds = built[0], built[0].dataset
    text = capsys.readouterr().out
    live = model.model.weights.numpy().copy()
    calls = NeighbourEngine.log
    # one k = 4 call per domain, then one k = 1 call per ordered pair of domains: each reads the item table once
    assert [c[0] for c in calls] == ["item_rows"] * (3 + 6)
    if "mamdr" in name:                 # ... under the QUERY domain's own weights: theta (+) phi_d differs between domains
        assert not np.array_equal(calls[0][1], calls[1][1])
        assert np.array_equal(calls[0][1], calls[3][1]) and np.array_equal(calls[0][1], calls[4][1])        # 0 -> 1, 0 -> 2
        assert np.array_equal(calls[1][1], calls[5][1]) and np.array_equal(calls[2][1], calls[8][1])
    rows = np.asarray(model.model.oracle.params["item_emb"], np.float32)
    cats = [np.unique(np.concatenate([s[d]["data"]["pid"] for s in (ds.train_dataset, ds.val_dataset, ds.test_dataset)]))
            for d in range(3)]
    with np.load(out) as z:
        assert z["domains"].tolist() == [0, 1, 2] and int(z["k"]) == 4
        assert z["affinity"].shape == z["shared_items"].shape == (3, 3)
        for key in nb.FIGURES:
            assert z[key].shape == (3,) and np.all(np.isfinite(z[key])), key
        for d in range(3):
            cat = cats[d]
            assert np.array_equal(z["catalogue_%d" % d], cat)
            want_ids, want_sims = nb.neighbours_host(rows, cat, 4, cat)
            assert np.array_equal(z["ids_%d" % d], want_ids) and np.array_equal(z["sims_%d" % d], want_sims.astype(np.float32))
            assert z["sims_%d" % d].dtype == np.float32 and z["ids_%d" % d].dtype == np.int32
            deg = lm.id_counts_host(want_ids, model.n_pid)
            assert np.array_equal(z["in_degree_%d" % d], deg[cat]) and z["in_degree_%d" % d].sum() == 4 * cat.size
            want = nb.summarise(cat, want_ids, want_sims.astype(np.float32), cat, deg, 4)
            for key in nb.FIGURES:
                assert z[key][d] == want[key], key
            assert z["affinity"][d, d] == want["mean_sim_1"] and z["shared_items"][d, d] == cat.size
            for e in range(3):
                assert z["shared_items"][d, e] == np.intersect1d(cat, cats[e]).size
                if e != d:
                    top_ids, top = nb.neighbours_host(rows, cat, 1, cats[e])
                    assert z["affinity"][d, e] == float(top.astype(np.float32).astype(np.float64)[top_ids[:, 0] >= 0, 0].mean())
            assert re.search(r"^%d: MeanSim@1 -?\d\.\d{4} MeanSim@4 -?\d\.\d{4} Hubness -?\d+\.\d{3} OrphanShare \d\.\d{4} " % d,
                             text, flags=re.M)
    assert "Similar items top-4" in text and "pretrained table" in text and "Embedding-space affinity" in text
    # the model call: items of my own, another catalogue, and the four keys
    r = model.similar_items(0, 3, items=cats[0][:5], target_domain=2)
    assert sorted(r) == ["catalogue", "ids", "items", "sims"] and np.array_equal(r["catalogue"], cats[2])
    assert np.array_equal(r["items"], cats[0][:5]) and r["ids"].shape == r["sims"].shape == (5, 3)
    assert np.array_equal(r["ids"], nb.neighbours_host(rows, cats[0][:5], 3, cats[2])[0])
    for q, row in zip(r["items"], r["ids"]):
        assert q not in row                 # an item both catalogues hold is not its own neighbour
    with pytest.raises(ValueError):
        model.similar_items(0, 129)
    # the report reads state only
    assert np.array_equal(model.model.weights.numpy(), live)
    # result.json carries the headline
    rdir = os.path.join(str(tmp_path / "result"), name, "Taobao", cfg["dataset"]["domain_split_path"])
    run = [p for p in os.listdir(rdir) if os.path.isdir(os.path.join(rdir, p))]
    assert len(run) == 1
    with open(os.path.join(rdir, run[0], "result.json")) as f:
        result = json.load(f)
    with np.load(out) as z:
        for key in nb.FIGURES:
            assert set(result["domain_" + key]) == {"0", "1", "2"} and result["domain_" + key]["1"] == float(z[key][1])
        for key in nb.AVERAGED:
            assert result["avg_" + key] == pytest.approx(float(np.mean(z[key])))
        assert result["domain_affinity"]["0"]["2"] == float(z["affinity"][0, 2]) and set(result["domain_affinity"]) == {"0", "1", "2"}
    assert len(result) > len(nb.FIGURES) + len(nb.AVERAGED) + 1          # (save_result's own keys are still there)


def test_default_path_and_no_flag_no_file(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "wdl", epochs=1)
    cfg["train"]["similar_items"] = 3
    cli.main(cfg, NeighbourEngine)
    rdir = os.path.join(str(tmp_path / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert "similar_items_top3.npz" in os.listdir(rdir)
    cli.main(tiny_config(tmp_path / "b", "wdl", epochs=1), NeighbourEngine)
    rdir = os.path.join(str(tmp_path / "b" / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert not [p for p in os.listdir(rdir) if p.endswith(".npz")]
