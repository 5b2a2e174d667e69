"""Top-K retrieval, host side (no GPU): the C ABI's declaration and binding, argument refusals that need no device, the
exclusion lists' CSR form, the ranking metrics on hand-computed cases, and `run.py --recommend K` end to end over a CPU
stand-in of the engine whose `recommend` is a numpy forward."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from fake_engine import FakeEngine
from mamdr_amd import _lib, cli, synthetic
from mamdr_amd import recommend as rec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def tiny_config(tmp_path, name, epochs=1):
    """the shipped Taobao-10 config shrunk to 3 domains, 8-wide tables and a [16, 8, 4] tower (tests/test_host_logic.py's)."""
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name, hidden_dim=[16, 8, 4], user_dim=8, item_dim=8, domain_dim=8)
    cfg["train"].update(epoch=epochs, patience=1, sample_num=2, result_save_path=str(tmp_path / "result"),
                        checkpoint_path=str(tmp_path / "checkpoint"))
    cfg["dataset"].update(batch_size=64, synthetic={"name": "Taobao", "split": "s", "n_domain": 3, "n_user": 300,
                                                    "n_item": 200, "n_train": 900, "n_val": 300, "n_test": 300,
                                                    "pretrained": True})
    return cfg


def patch_emb_dim(monkeypatch):
    real = synthetic.generate
    monkeypatch.setattr(synthetic, "generate", lambda *a, **k: real(*a, **dict(k, emb_dim=8)))


# ------------------------------------------------------------------ C ABI
def test_recommend_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    m = re.search(r"\bint\s+mamdr_recommend\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "mamdr_recommend is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mamdr_ctx* ctx", "int32_t n_query", "const int32_t* d_uid", "const int32_t* d_domain",
                      "const int32_t* d_cand", "int64_t n_cand", "const int64_t* d_excl_off", "const int32_t* d_excl_ids",
                      "int32_t k", "int32_t* d_ids_out", "float* d_scores_out", "float* d_scores_all"], params
    # the header says plainly that the reference has nothing of the kind
    doc = header[:header.index("int mamdr_recommend")].rsplit("/*", 1)[1]
    assert "NO REFERENCE COUNTERPART" in doc
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_recommend"] == (C.c_int, [vp, i32, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp])
    assert _lib.ABI_VERSION == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert any(t[0] == "MAMDR_REC_CHUNK" for t in _lib.env_switches())


def test_null_context_is_refused_without_a_device():
    lib = _lib.load()
    code = lib.mamdr_recommend(None, 1, None, None, None, 0, None, None, 10, None, None, None)
    assert code == _lib.EINVAL
    assert b"null context" in lib.mamdr_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(code)


# ------------------------------------------------------------------ exclusion lists
def test_exclusion_csr_sorts_and_deduplicates():
    off, ids = rec.exclusion_csr([[5, 1, 3, 1, 5], [], None, np.array([7]), (9, 2, 2)], 5)
    assert off.dtype == np.int64 and ids.dtype == np.int32
    assert off.tolist() == [0, 3, 3, 3, 4, 6]
    assert ids.tolist() == [1, 3, 5, 7, 2, 9]
    off, ids = rec.exclusion_csr([[], []], 2)
    assert off.tolist() == [0, 0, 0] and ids.size == 0
    off, ids = rec.exclusion_csr([], 0)
    assert off.tolist() == [0] and ids.size == 0
    with pytest.raises(ValueError):
        rec.exclusion_csr([[1]], 2)                  # one list per query
    with pytest.raises(ValueError):
        rec.exclusion_csr([[-1]], 1)


# ------------------------------------------------------------------ metrics
def test_ranking_metrics_hand_computed():
    d = lambda r: 1.0 / np.log2(r + 2.0)      # noqa: E731
    ids = np.array([[4, 9, 2, 7],             # positives {9, 7, 1}: hits at ranks 1 and 3
                    [3, 5, 6, 8],             # positives {0}: no hit
                    [1, 2, 3, 4],             # no positives: left out of the averages
                    [6, -1, -1, -1]], np.int32)      # short list, positives {6, 5}: hit at rank 0
    pos = [np.array([9, 7, 1]), [0], [], [5, 6, 6]]
    m = rec.ranking_metrics(ids, pos)
    assert m["n_eval"] == 3
    assert m["hit_rate"] == pytest.approx(2.0 / 3.0)
    assert m["recall"] == pytest.approx((2.0 / 3.0 + 0.0 + 1.0 / 2.0) / 3.0)
    ndcg0 = (d(1) + d(3)) / (d(0) + d(1) + d(2))
    ndcg3 = d(0) / (d(0) + d(1))
    assert m["ndcg"] == pytest.approx((ndcg0 + 0.0 + ndcg3) / 3.0)
    # the padding id never counts as a hit, not even for a "positive" of -1
    assert rec.ranking_metrics(np.array([[-1, -1]]), [[-1]])["hit_rate"] == 0.0
    # a perfect list
    m = rec.ranking_metrics(np.array([[2, 1, 0]]), [[0, 1, 2]])
    assert m["hit_rate"] == 1.0 and m["recall"] == 1.0 and m["ndcg"] == pytest.approx(1.0)
    # nobody has a positive
    assert rec.ranking_metrics(np.array([[1, 2]]), [[]]) == {"hit_rate": 0.0, "recall": 0.0, "ndcg": 0.0, "n_eval": 0}
    with pytest.raises(ValueError):
        rec.ranking_metrics(np.array([1, 2]), [[1]])


# ------------------------------------------------------------------ run.py --recommend K over a CPU stand-in
class RecommendingEngine(FakeEngine):
    """FakeEngine + `recommend` as a numpy forward of the oracle's tower (TowerEngine.recommend's contract)."""
    calls_recommend = 0

    def recommend(self, uids, domains, k, candidates=None, exclude=None, want_scores=False):
        type(self).calls_recommend += 1
        uid = np.asarray(uids, np.int32).ravel()
        dom = np.broadcast_to(np.asarray(domains, np.int32), uid.shape)
        cand = np.arange(self.n_item, dtype=np.int32) if candidates is None else np.asarray(candidates, np.int32)
        off, ex = rec.exclusion_csr(exclude if exclude is not None else [()] * uid.size, uid.size)
        ids = np.full((uid.size, k), -1, np.int32)
        scores = np.zeros((uid.size, k), np.float32)
        all_scores = np.zeros((uid.size, cand.size), np.float32)
        for q in range(uid.size):
            p = self.oracle.predict(np.full(cand.size, uid[q], np.int32), cand, np.full(cand.size, dom[q], np.int32))
            keep = ~np.isin(cand, ex[off[q]:off[q + 1]])
            all_scores[q] = np.where(keep, p, 0)
            order = np.lexsort((cand[keep], -p[keep]))[:k]
            ids[q, :order.size], scores[q, :order.size] = cand[keep][order], p[keep][order]
        return (ids, scores, all_scores) if want_scores else (ids, scores)


@pytest.mark.parametrize("name", ["mlp_meta_mamdr_finetune", "wdl", "mlp_uncertainty_weight", "mlp_pcgrad"])
def test_run_recommend_flag_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    """reachable through every kind of wrapper cli.build_model returns (meta wrappers' and UncertaintyWeight's __getattr__)."""
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, name, epochs=1)
    built = []
    out = str(tmp_path / "top5.npz")
    res = cli.main(cfg, RecommendingEngine, on_model=built.append, recommend=5, recommend_out=out)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}
    model = built[0]
    ds = model.dataset
    text = capsys.readouterr().out
    with np.load(out) as z:
        assert z["domains"].tolist() == [0, 1, 2] and int(z["k"]) == 5
        for name_ in ("hit_rate", "recall", "ndcg"):
            assert z[name_].shape == (3,) and np.all(np.isfinite(z[name_])) and np.all((z[name_] >= 0) & (z[name_] <= 1))
        for d in range(3):
            users, ids, scores = z["users_%d" % d], z["ids_%d" % d], z["scores_%d" % d]
            test_uids = np.unique(ds.test_dataset[d]["data"]["uid"])
            assert np.array_equal(users, test_uids)
            assert ids.shape == scores.shape == (users.size, 5) and ids.dtype == np.int32 and scores.dtype == np.float32
            catalogue = np.unique(np.concatenate([s[d]["data"]["pid"] for s in (ds.train_dataset, ds.val_dataset, ds.test_dataset)]))
            assert np.all(np.isin(ids[ids >= 0], catalogue))
            for q, u in enumerate(users):
                seen = np.concatenate([s[d]["data"]["pid"][s[d]["data"]["uid"] == u] for s in (ds.train_dataset, ds.val_dataset)])
                got = ids[q][ids[q] >= 0]
                assert not np.isin(got, seen).any() and np.unique(got).size == got.size
                assert np.all(np.diff(scores[q][:got.size]) <= 0)
            assert re.search(r"^%d: HitRate@5 \d\.\d{4} Recall@5 \d\.\d{4} NDCG@5 \d\.\d{4}" % d, text, flags=re.M)
    # BaseModel.recommend itself, through the wrapper: explicit users, nothing excluded
    r = model.recommend(1, 3, users=[4, 2], exclude_seen=False)
    assert r["users"].tolist() == [4, 2] and r["ids"].shape == r["scores"].shape == (2, 3)
    # default output path: under train.result_save_path
    cli.main(tiny_config(tmp_path / "again", name, epochs=1), RecommendingEngine, recommend=2)
    rdir = os.path.join(str(tmp_path / "again" / "result"), name, "Taobao", cfg["dataset"]["domain_split_path"])
    assert "recommend_top2.npz" in os.listdir(rdir)


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    RecommendingEngine.calls_recommend = 0
    with_flag = cli.main(tiny_config(tmp_path / "a", "mlp", epochs=1), RecommendingEngine, recommend=3)
    n_calls = RecommendingEngine.calls_recommend
    assert n_calls == 3
    without = cli.main(tiny_config(tmp_path / "b", "mlp", epochs=1), RecommendingEngine)
    assert RecommendingEngine.calls_recommend == n_calls             # no recommend call at all
    assert without == with_flag                                      # ... and the same result tuple, to the bit
    rdir = os.path.join(str(tmp_path / "b" / "result"), "mlp", "Taobao", tiny_config(tmp_path, "mlp")["dataset"]["domain_split_path"])
    runs = os.listdir(rdir)
    assert len(runs) == 1 and os.path.isdir(os.path.join(rdir, runs[0]))          # the run's folder, no extra file
    assert set(os.listdir(os.path.join(rdir, runs[0]))) == {"dataset_info.json", "config.json.example", "result.json",
                                                            "model_parameters.npz"}
    # the command line: the flags parse, and their absence calls main exactly as before
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--recommend", "10", "--recommend-out", "x.npz"])
    assert seen[0][1] == {} and len(seen[0][0]) == 1
    assert seen[1][1] == {"recommend": 10, "recommend_out": "x.npz"}


def test_generic_layer_engine_refuses_by_name():
    from mamdr_amd import graph_engine
    eng = graph_engine.GraphEngine.__new__(graph_engine.GraphEngine)      # (no device: the refusal needs none)
    eng.kind = "mmoe"
    with pytest.raises(NotImplementedError, match="generic-layer towers.*mmoe.*not built for retrieval"):
        eng.recommend([0], [0], 5)
    eng.ctx = None
