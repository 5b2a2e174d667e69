"""Beyond-accuracy report of top-K lists, host side (no GPU): the C ABI's declarations and binding, the refusals that need no
device, `list_metrics.summarise` on hand-computed cases, personalisation against the brute-force pairwise overlap, the host
definition of the list similarity against a plain double loop, the command line, and `run.py --list-metrics` end to end
over a CPU stand-in whose two device calls are the host definitions."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

from mamdr_amd import _lib, cli
from mamdr_amd import list_metrics as lm
from test_recommend_host import RecommendingEngine, patch_emb_dim, tiny_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------ C ABI
def test_both_calls_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mamdr_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mamdr_id_counts\s*\(([^;]*)\)\s*;", header)
    assert m and [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "const int32_t* d_ids", "const float* d_label", "int64_t n", "int64_t n_bins", "uint32_t* d_counts", "void* stream"]
    m = re.search(r"\bint\s+mamdr_list_similarity\s*\(([^;]*)\)\s*;", header)
    assert m and [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "const int32_t* d_ids", "int32_t n_list", "int32_t k", "const float* d_rows", "int64_t n_rows", "int32_t emb_dim",
        "double* d_sim_sum", "int32_t* d_pairs", "void* stream"]
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_id_counts"] == (C.c_int, [vp, vp, i64, i64, vp, vp])
    assert _lib.SIGNATURES["mamdr_list_similarity"] == (C.c_int, [vp, i32, i32, vp, i64, i32, vp, vp, vp])
    lib = _lib.load()
    assert hasattr(lib, "mamdr_id_counts") and hasattr(lib, "mamdr_list_similarity")
    # new entry points only: the version stays
    assert _lib.ABI_VERSION == 19 and lib.mamdr_abi_version() == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert re.search(r"#define\s+MAMDR_LIST_MAX_K\s+128\b", header) and _lib.LIST_MAX_K == lm.MAX_K == 128
    assert _lib.LIST_EMB_DIMS == lm.EMB_DIMS == (32, 64, 128, 256)


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    p = C.c_void_p(1 << 20)               # an aligned non-null address: a refusal never dereferences it
    assert lib.mamdr_id_counts(None, None, 0, 4, None, None) == _lib.EINVAL
    assert b"null counts" in lib.mamdr_last_error()
    assert lib.mamdr_id_counts(None, None, 5, 4, p, None) == _lib.EINVAL            # ids missing for n > 0
    assert lib.mamdr_id_counts(p, None, -1, 4, p, None) == _lib.EINVAL
    assert lib.mamdr_id_counts(p, None, 1 << 32, 4, p, None) == _lib.EINVAL
    assert lib.mamdr_id_counts(p, None, 5, 0, p, None) == _lib.EINVAL
    assert lib.mamdr_id_counts(C.c_void_p((1 << 20) + 2), None, 5, 4, p, None) == _lib.EINVAL
    assert b"aligned" in lib.mamdr_last_error()
    assert lib.mamdr_list_similarity(None, 1, 2, None, 1, 32, None, None, None) == _lib.EINVAL
    assert b"null" in lib.mamdr_last_error()
    for n_list, k, n_rows, emb, rows, word in ((0, 2, 5, 32, p, b"n_list"), (1, 0, 5, 32, p, b"k 0"), (1, 129, 5, 32, p, b"k 129"),
                                               (1, 2, 5, 96, p, b"emb_dim 96"), (1, 2, 0, 32, p, b"n_rows"),
                                               (1, 2, 5, 32, C.c_void_p((1 << 20) + 4), b"aligned")):
        assert lib.mamdr_list_similarity(p, n_list, k, rows, n_rows, emb, p, p, None) == _lib.EINVAL
        assert word in lib.mamdr_last_error(), lib.mamdr_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(_lib.EINVAL)


# ------------------------------------------------------------------ the host definitions of the two calls
def test_id_counts_host():
    ids = np.array([3, -1, 0, 3, 7, 2 ** 31 - 1, 3, 6], np.int32)
    assert lm.id_counts_host(ids, 7).tolist() == [1, 0, 0, 3, 0, 0, 1]
    label = np.array([1, 1, -0.0, 0.5, 1, 1, 0.0, np.nan], np.float32)
    assert lm.id_counts_host(ids, 7, label).tolist() == [0, 0, 0, 2, 0, 0, 1]          # -0.0 is 0, NaN is not
    assert lm.id_counts_host(np.zeros(0, np.int32), 3).tolist() == [0, 0, 0]
    assert lm.id_counts_host(ids.reshape(2, 4), 4).tolist() == [1, 0, 0, 3]
    with pytest.raises(ValueError):
        lm.id_counts_host(ids, 0)
    with pytest.raises(ValueError):
        lm.id_counts_host(ids, 7, label[:3])


def test_list_similarity_host_against_a_double_loop():
    rs = np.random.RandomState(5)
    rows = (rs.randn(40, 32) * 10.0 ** rs.uniform(-3, 3, (40, 1))).astype(np.float32)
    rows[7] = 0.0
    ids = rs.randint(0, 40, (9, 11)).astype(np.int32)
    ids[0, :] = -1                                    # all padding
    ids[1, 1:] = -1                                   # one entry
    ids[2, [2, 5, 6]] = [-1, 40, 2 ** 31 - 1]         # padding in the middle, n_rows and a huge id
    ids[3, :4] = [7, 7, 3, 3]                         # the zero row, duplicates
    sim, pairs = lm.list_similarity_host(ids, rows)
    assert sim.dtype == np.float64 and pairs.dtype == np.int32
    for q in range(ids.shape[0]):
        valid = [int(i) for i in ids[q] if 0 <= i < 40]
        want, n = 0.0, 0
        for a in range(len(valid)):
            for b in range(a + 1, len(valid)):
                x, y = rows[valid[a]].astype(np.float64), rows[valid[b]].astype(np.float64)
                nx, ny = math.sqrt(float(x @ x)), math.sqrt(float(y @ y))
                want += float(x @ y) / (nx * ny) if nx > 0 and ny > 0 else 0.0
                n += 1
        assert pairs[q] == n
        assert sim[q] == pytest.approx(want, abs=1e-12 * max(n, 1))
    assert pairs[0] == 0 and sim[0] == 0.0 and pairs[1] == 0 and sim[1] == 0.0
    # a duplicate pair is one pair with cosine 1
    s, p = lm.list_similarity_host(np.array([[3, 3]]), rows)
    assert p[0] == 1 and s[0] == pytest.approx(1.0, abs=1e-15)
    s, p = lm.list_similarity_host(np.array([[7, 3]]), rows)
    assert p[0] == 1 and s[0] == 0.0                  # exactly 0 with a zero row


# ------------------------------------------------------------------ summarise, hand-computed
def _vec(n_item, pairs_):
    v = np.zeros(n_item, np.int64)
    for i, c in pairs_:
        v[i] = c
    return v


def test_uniform_and_concentrated_exposure():
    n = 8
    cat = np.arange(2, 2 + n)
    m = lm.summarise(_vec(12, [(i, 5) for i in cat]), _vec(12, [(i, 1) for i in cat]), cat, 4, [], [])
    assert m["coverage"] == 1.0 and m["gini"] == pytest.approx(0.0, abs=1e-15) and m["entropy"] == pytest.approx(math.log2(n))
    assert m["n_items"] == n and m["n_shown"] == 40 and m["n_lists"] == 10 and m["ild"] == 0.0 and m["n_ild"] == 0
    # ids outside the catalogue are not part of the domain
    m = lm.summarise(_vec(12, [(i, 5) for i in cat] + [(0, 99)]), _vec(12, [(i, 1) for i in cat] + [(11, 7)]), cat, 4, [], [])
    assert m["gini"] == pytest.approx(0.0, abs=1e-15) and m["n_shown"] == 40
    # all exposure on one item
    m = lm.summarise(_vec(12, [(5, 30)]), _vec(12, [(i, 1) for i in cat]), cat, 1, [], [])
    assert m["coverage"] == 1.0 / n and m["gini"] == pytest.approx((n - 1.0) / n) and m["entropy"] == 0.0
    assert math.copysign(1.0, m["entropy"]) == 1.0
    # novelty / average popularity by hand: c = (3, 1), p = (6, 0) over a catalogue of 2: P + n = 8
    m = lm.summarise([3, 1], [6, 0], [0, 1], 2, [], [])
    assert m["novelty"] == pytest.approx((3 * -math.log2(7.0 / 8.0) + 1 * -math.log2(1.0 / 8.0)) / 4.0)
    assert m["avg_popularity"] == pytest.approx(18.0 / 4.0)
    assert m["gini"] == pytest.approx(((2 - 3) * 1 + (4 - 3) * 3) / (2.0 * 4.0))


def test_nothing_shown_and_one_list():
    m = lm.summarise(np.zeros(6, np.int64), [4, 0, 1, 0, 0, 2], np.arange(6), 3, [0.0, 0.0], [0, 0])
    for key in lm.FIGURES:
        assert m[key] == 0.0, key
    assert m["n_ild"] == 0 and m["n_lists"] == 0 and m["n_shown"] == 0
    # Q' = 1: no pair of lists
    m = lm.summarise([1, 1, 1, 0], [1, 1, 1, 1], np.arange(4), 3, [1.5], [3], n_lists=1)
    assert m["personalisation"] == 0.0 and m["coverage"] == 0.75
    assert m["ild"] == pytest.approx(0.5) and m["n_ild"] == 1
    with pytest.raises(ValueError):
        lm.summarise([1], [1], [], 3, [], [])
    with pytest.raises(ValueError):
        lm.summarise([1], [1], [4], 3, [], [])


def test_personalisation_identical_disjoint_and_brute_force():
    k, n_item = 5, 60
    same = np.tile(np.arange(10, 15), (7, 1))
    m = lm.summarise(lm.id_counts_host(same, n_item), np.ones(n_item, np.int64), np.arange(n_item), k, [], [], n_lists=7)
    assert m["personalisation"] == pytest.approx(0.0, abs=1e-15)
    assert lm.summarise(lm.id_counts_host(same, n_item), np.ones(n_item, np.int64), np.arange(n_item), k, [], [])["n_lists"] == 7
    disjoint = np.arange(35).reshape(7, 5)
    m = lm.summarise(lm.id_counts_host(disjoint, n_item), np.ones(n_item, np.int64), np.arange(n_item), k, [], [], n_lists=7)
    assert m["personalisation"] == 1.0
    # 40 random lists of distinct ids, some short: one minus the mean pairwise overlap / k, by brute force
    rs = np.random.RandomState(11)
    k = 8
    lists = np.full((40, k), -1, np.int32)
    for q in range(40):
        L = k if q % 5 else rs.randint(1, k)
        lists[q, :L] = rs.choice(30, L, replace=False)
    overlap = [len(set(lists[a][lists[a] >= 0]) & set(lists[b][lists[b] >= 0])) for a in range(40) for b in range(a + 1, 40)]
    want = 1.0 - float(np.mean(overlap)) / k
    m = lm.summarise(lm.id_counts_host(lists, 30), np.ones(30, np.int64), np.arange(30), k, [], [], n_lists=40)
    assert m["personalisation"] == pytest.approx(want, abs=1e-12) and 0.0 < want < 1.0


def test_tail_share_boundary_and_tie_by_id():
    # p = (4, 4, 1, 1) -> P = 10, 0.8 P = 8: the head {0, 1} reaches it EXACTLY (5 * 8 >= 4 * 10) and stops there
    c = [1, 2, 3, 4]
    m = lm.summarise(c, [4, 4, 1, 1], np.arange(4), 2, [], [])
    assert m["tail_share"] == pytest.approx(7.0 / 10.0)
    # one short of the boundary: p = (4, 3, 2, 1), head {0, 1} sums to 7 < 8 -> item 2 joins the head
    m = lm.summarise(c, [4, 3, 2, 1], np.arange(4), 2, [], [])
    assert m["tail_share"] == pytest.approx(4.0 / 10.0)
    # a tie at the head's edge is broken by ascending id: p = (1, 4, 4, 1, 0), 0.8 P = 8 = items 1 and 2; with
    # p = (2, 4, 2, 2), 0.8 P = 8 needs 4 + 2 + 2: items 1, 0, 2 -- not 3
    m = lm.summarise([1, 2, 3, 4, 5], [1, 4, 4, 1, 0], np.arange(5), 2, [], [])
    assert m["tail_share"] == pytest.approx((1 + 4 + 5) / 15.0)
    m = lm.summarise([1, 2, 4, 8], [2, 4, 2, 2], np.arange(4), 2, [], [])
    assert m["tail_share"] == pytest.approx(8.0 / 15.0)
    # catalogue ids, not positions, break the tie: the same counts on ids (9, 3, 5, 7) in any order of `catalogue`
    expo, pop = _vec(10, [(9, 1), (3, 2), (5, 4), (7, 8)]), _vec(10, [(9, 2), (3, 4), (5, 2), (7, 2)])
    m = lm.summarise(expo, pop, [9, 3, 5, 7], 2, [], [])            # head: 3 (p 4), then 5, 7 by id; tail: 9
    assert m["tail_share"] == pytest.approx(1.0 / 15.0)
    # nobody ever clicked: the head is empty
    assert lm.summarise(c, [0, 0, 0, 0], np.arange(4), 2, [], [])["tail_share"] == 1.0


def test_ild_skips_lists_without_a_pair():
    m = lm.summarise([2, 2, 2], [1, 1, 1], np.arange(3), 3, [0.0, 0.3, -0.5, 0.0], [0, 3, 1, 0], n_lists=3)
    assert m["n_ild"] == 2 and m["ild"] == pytest.approx(((1 - 0.1) + (1 + 0.5)) / 2.0)
    with pytest.raises(ValueError):
        lm.summarise([2], [1], [0], 3, [0.0], [0, 1])
    assert lm.error_bound(128) == (2 * 128 + 8) * 2.0 ** -24
    with pytest.raises(ValueError):
        lm.check_k(129)


# ------------------------------------------------------------------ the command line
def test_flags_parse_and_their_absence_calls_main_as_before(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--list-metrics"])
    cli.cli(["--config", cfg_path, "--recommend", "7", "--list-metrics"])
    cli.cli(["--config", cfg_path, "--list-metrics", "20", "--list-metrics-out", "x.npz", "--recommend", "7"])
    assert seen[0][1] == {} and len(seen[0][0]) == 1
    assert "list_metrics" not in seen[0][0][0]["train"] and "list_metrics_out" not in seen[0][0][0]["train"]
    assert seen[1][1] == {} and seen[1][0][0]["train"]["list_metrics"] == 10
    assert seen[2][1] == {"recommend": 7, "recommend_out": None} and seen[2][0][0]["train"]["list_metrics"] == 7
    assert seen[3][0][0]["train"]["list_metrics"] == 20 and seen[3][0][0]["train"]["list_metrics_out"] == "x.npz"
    for bad in ("0", "129"):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path, "--list-metrics", bad])
    assert "--list-metrics" in cli.__doc__ and "--list-metrics-out" in cli.__doc__


def test_several_lanes_are_refused(tmp_path):
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr")
    cfg["train"].update(lanes=2, list_metrics=5)
    with pytest.raises(NotImplementedError, match=r"train\.list_metrics \(run\.py --list-metrics\).*one process"):
        cli.main(cfg, RecommendingEngine)


# ------------------------------------------------------------------ run.py --list-metrics over a CPU stand-in
def _np(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


class ListEngine(RecommendingEngine):
    """RecommendingEngine + the two device calls as their host definitions and `item_rows` as the oracle's item table.  It
    records the live weights at every `recommend` and `item_rows` call."""
    log = []

    def recommend(self, *a, **kw):
        type(self).log.append(("recommend", self.weights.numpy().copy()))
        return RecommendingEngine.recommend(self, *a, **kw)

    def item_rows(self):
        type(self).log.append(("item_rows", self.weights.numpy().copy()))
        return self.oracle.params["item_emb"]

    def id_counts(self, ids, n_bins, label=None):
        return lm.id_counts_host(_np(ids), n_bins, None if label is None else _np(label))

    def list_similarity(self, ids, rows):
        return lm.list_similarity_host(_np(ids), _np(rows))


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr_finetune", "mlp_pcgrad"])
def test_report_and_headline_end_to_end_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    out = str(tmp_path / "lm.npz")
    cfg["train"].update(list_metrics=5, list_metrics_out=out)
    built = []
    ListEngine.log = []
    res = cli.main(cfg, ListEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model, ds = built[0], built[0].dataset
    text = capsys.readouterr().out
    live = model.model.weights.numpy().copy()
    # the lists are scored and the item table is read under the same installed weights, domain by domain
    calls = ListEngine.log
    assert [c[0] for c in calls] == ["recommend", "item_rows"] * 3
    for d in range(3):
        assert np.array_equal(calls[2 * d][1], calls[2 * d + 1][1])
    if "mamdr" in name:                 # ... which are the domain's own: theta (+) phi_d differs between domains
        assert not np.array_equal(calls[0][1], calls[2][1])
    rows = model.model.oracle.params["item_emb"]
    with np.load(out) as z:
        assert z["domains"].tolist() == [0, 1, 2] and int(z["k"]) == 5
        for key in lm.FIGURES + ("n_ild",):
            assert z[key].shape == (3,) and np.all(np.isfinite(z[key]))
        for d in range(3):
            cat = np.unique(np.concatenate([s[d]["data"]["pid"] for s in (ds.train_dataset, ds.val_dataset, ds.test_dataset)]))
            assert np.array_equal(z["catalogue_%d" % d], cat)
            tr = ds.train_dataset[d]["data"]
            assert np.array_equal(z["popularity_%d" % d], np.bincount(tr["pid"][tr["label"] > 0], minlength=model.n_pid)[cat])
            n_users = np.unique(ds.test_dataset[d]["data"]["uid"]).size
            assert z["exposure_%d" % d].shape == cat.shape and z["exposure_%d" % d].sum() == 5 * n_users
            assert z["sim_sum_%d" % d].shape == z["pairs_%d" % d].shape == (n_users,)
            assert z["sim_sum_%d" % d].dtype == np.float64 and np.all(z["pairs_%d" % d] == 10)
            assert 0.0 < z["coverage"][d] <= 1.0 and 0.0 <= z["gini"][d] < 1.0 and 0.0 <= z["personalisation"][d] <= 1.0
            assert re.search(r"^%d: Coverage@5 \d\.\d{4} Gini \d\.\d{4} " % d, text, flags=re.M)
        if "mamdr" not in name:         # the live weights produced the lists: the report is summarise over the host route
            for d in range(3):
                r = model.recommend(d, 5)
                sim, pairs = lm.list_similarity_host(r["ids"], rows)
                want = lm.summarise(lm.id_counts_host(r["ids"], model.n_pid), np.bincount(
                    ds.train_dataset[d]["data"]["pid"][ds.train_dataset[d]["data"]["label"] > 0], minlength=model.n_pid),
                    z["catalogue_%d" % d], 5, sim, pairs, n_lists=r["ids"].shape[0])
                for key in lm.FIGURES:
                    assert z[key][d] == want[key], key
    # the report reads state only
    assert np.array_equal(model.model.weights.numpy(), live)
    # result.json carries the headline
    rdir = os.path.join(str(tmp_path / "result"), name, "Taobao", cfg["dataset"]["domain_split_path"])
    run = [p for p in os.listdir(rdir) if os.path.isdir(os.path.join(rdir, p))]
    assert len(run) == 1
    with open(os.path.join(rdir, run[0], "result.json")) as f:
        result = json.load(f)
    for key in lm.FIGURES:
        assert set(result["domain_" + key]) == {"0", "1", "2"}
    with np.load(out) as z:
        for key in lm.AVERAGED:
            assert result["avg_" + key] == pytest.approx(float(np.mean(z[key])))
        assert result["domain_coverage"]["1"] == float(z["coverage"][1])
    assert len(result) > len(lm.FIGURES) + len(lm.AVERAGED)          # (save_result's own keys are still there)


def test_default_path_and_no_flag_no_file(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "wdl", epochs=1)
    cfg["train"]["list_metrics"] = 3
    cli.main(cfg, ListEngine)
    rdir = os.path.join(str(tmp_path / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert "list_metrics_top3.npz" in os.listdir(rdir)
    ListEngine.log = []
    cli.main(tiny_config(tmp_path / "b", "wdl", epochs=1), ListEngine)
    assert ListEngine.log == []
    rdir = os.path.join(str(tmp_path / "b" / "result"), "wdl", "Taobao", cfg["dataset"]["domain_split_path"])
    assert not [p for p in os.listdir(rdir) if p.endswith(".npz")]
