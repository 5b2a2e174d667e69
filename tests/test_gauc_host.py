"""Per-user grouped AUC, host side (no GPU): the C ABI's declaration, binding and device-free refusals, `gauc.group_plan`
on crafted uids, `gauc.group_auc_host` on hand-computed cases and against a brute-force double loop, and `run.py --gauc`
end to end over a CPU stand-in of the engine whose `evaluate` honours `want_gauc` through `group_auc_host`."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from fake_engine import ReportingFakeEngine
from mamdr_amd import _lib, cli, gauc, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAN = float("nan")


def tiny_config(tmp_path, name, epochs=1, **train):
    """the shipped Taobao-10 config shrunk to 3 domains, 8-wide tables and a [16, 8, 4] tower (tests/test_host_logic.py's)."""
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name, hidden_dim=[16, 8, 4], user_dim=8, item_dim=8, domain_dim=8)
    cfg["train"].update(epoch=epochs, patience=1, sample_num=2, result_save_path=str(tmp_path / "result"),
                        checkpoint_path=str(tmp_path / "checkpoint"), **train)
    cfg["dataset"].update(batch_size=64, synthetic={"name": "Taobao", "split": "s", "n_domain": 3, "n_user": 300,
                                                    "n_item": 200, "n_train": 900, "n_val": 300, "n_test": 300,
                                                    "pretrained": True})
    return cfg


def patch_emb_dim(monkeypatch):
    real = synthetic.generate
    monkeypatch.setattr(synthetic, "generate", lambda *a, **k: real(*a, **dict(k, emb_dim=8)))


def brute_force(pred, label, uid):
    """the definition as a double loop over the rows of every user -> {uid: (T, P, r)} in python integers."""
    pred, label, uid = np.asarray(pred, np.float32), np.asarray(label), np.asarray(uid)

    def cmp(a, b):          # -1 / 0 / 1 under the definition's three rules
        a_nan, b_nan = a != a, b != b
        if a_nan or b_nan:
            return 0 if (a_nan and b_nan) else (-1 if a_nan else 1)
        return (a > b) - (a < b)         # (IEEE: -0.0 == 0.0)
    out = {}
    for u in np.unique(uid):
        rows = np.flatnonzero(uid == u)
        pos = [float(pred[i]) for i in rows if label[i] != 0]
        neg = [float(pred[i]) for i in rows if label[i] == 0]
        t = 0
        for p in pos:
            for q in neg:
                c = cmp(p, q)
                t += 2 if c > 0 else (1 if c == 0 else 0)
        out[int(u)] = (t, len(pos), len(rows))
    return out


def report_of(groups):
    """{uid: (T, P, r)} -> the report, terms added in ascending uid order."""
    num, rows_valid, n_valid = 0.0, 0, 0
    for u in sorted(groups):
        t, p, r = groups[u]
        if p > 0 and r - p > 0:
            num += float(r) * (float(t) / float(2 * p * (r - p)))
            rows_valid += r
            n_valid += 1
    return gauc.finish(num, rows_valid, n_valid, len(groups))


# ------------------------------------------------------------------ C ABI
def test_group_auc_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    m = re.search(r"\bint\s+mamdr_group_auc\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "mamdr_group_auc is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* d_pred", "const float* d_label", "const int32_t* d_order", "int64_t n",
                      "const int64_t* d_group_off", "int64_t n_groups", "const int32_t* d_tile_group",
                      "const int64_t* d_tile_first", "int64_t n_tiles", "uint64_t* d_T", "uint32_t* d_P", "double* d_result",
                      "void* stream"], params
    doc = header[:header.index("int mamdr_group_auc")].rsplit("/*", 1)[1]
    assert "NO REFERENCE COUNTERPART" in doc
    for phrase in ("T_u = 2 * #{(p, n): s_p > s_n} + #{(p, n): s_p == s_n}", "AUC_u = T_u / (2 * P_u * N_u)",
                   "-0 equals +0", "A NaN is below every number, -inf included", "Two NaNs are equal",
                   "GAUC = sum_valid r_u * AUC_u / sum_valid r_u"):
        assert phrase in doc and phrase in gauc.__doc__, phrase
    vp, i64 = C.c_void_p, C.c_int64
    assert _lib.SIGNATURES["mamdr_group_auc"] == (C.c_int, [vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp])
    assert _lib.ABI_VERSION == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    x = C.c_void_p(64)            # never dereferenced: every case below is refused before any device call

    def call(pred=x, label=x, order=x, n=8, off=x, groups=2, tg=None, tf=None, tiles=0, result=x):
        return lib.mamdr_group_auc(pred, label, order, n, off, groups, tg, tf, tiles, None, None, result, None)
    cases = {"null result": dict(result=None), "null offsets": dict(off=None), "null pred": dict(pred=None),
             "null label": dict(label=None), "null order": dict(order=None), "n < 0": dict(n=-1, groups=0),
             "G < 0": dict(groups=-1), "G > n": dict(groups=9), "tile list without tiles": dict(tg=x, tf=x, tiles=0),
             "tiles without their lists": dict(tiles=1), "one list only": dict(tg=x, tiles=1), "tiles < 0": dict(tiles=-1)}
    for what, kw in cases.items():
        assert call(**kw) == _lib.EINVAL, what
        assert b"mamdr_group_auc" in lib.mamdr_last_error(), what
    with pytest.raises(_lib.MamdrError, match="tile list given without tiles"):
        _lib.check(call(tg=x, tf=x, tiles=0))


# ------------------------------------------------------------------ the plan
def check_plan(uid, plan):
    uid = np.asarray(uid)
    n = uid.size
    assert plan.order.dtype == np.int32 and plan.group_off.dtype == np.int64
    assert plan.tile_group.dtype == np.int32 and plan.tile_first.dtype == np.int64
    assert sorted(plan.order.tolist()) == list(range(n))
    assert plan.group_off[0] == 0 and plan.group_off[-1] == n and np.all(np.diff(plan.group_off) > 0)
    users = []
    for g in range(plan.group_off.size - 1):
        rows = plan.order[plan.group_off[g]:plan.group_off[g + 1]]
        assert np.unique(uid[rows]).size == 1
        assert np.all(np.diff(rows) > 0)                   # stable: file order inside a group
        users.append(uid[rows[0]])
    assert users == sorted(set(uid.tolist()))             # every user once, ascending
    # every group of more than 64 rows is covered exactly once by tiles of at most 256
    covered = np.zeros(n, np.int64)
    sizes = np.diff(plan.group_off)
    for g, first in zip(plan.tile_group.tolist(), plan.tile_first.tolist()):
        assert sizes[g] > 64
        last = min(first + 256, plan.group_off[g + 1])
        assert plan.group_off[g] <= first < last
        covered[first:last] += 1
    in_big = np.repeat(sizes > 64, sizes)
    assert np.array_equal(covered, in_big.astype(np.int64))


def test_group_plan_on_crafted_uids():
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1100, 3]
    uid = np.repeat(np.array([50, 7, 3, 90, 12, 41, 8, 77, 5, 60, 1]), sizes)
    uid = uid[np.random.RandomState(0).permutation(uid.size)]
    plan = gauc.group_plan(uid)
    check_plan(uid, plan)
    by_uid = dict(zip([50, 7, 3, 90, 12, 41, 8, 77, 5, 60, 1], sizes))
    assert np.diff(plan.group_off).tolist() == [by_uid[u] for u in sorted(by_uid)]
    tiles_of = {u: -(-s // 256) for u, s in by_uid.items() if s > 64}
    assert plan.tile_group.size == sum(tiles_of.values()) == 1 + 1 + 1 + 2 + 3 + 5
    # a tiny explicit case: offsets and the stable order
    plan = gauc.group_plan([4, 2, 4, 9, 2, 4])
    assert plan.order.tolist() == [1, 4, 0, 2, 5, 3] and plan.group_off.tolist() == [0, 2, 5, 6]
    assert plan.tile_group.size == 0 and plan.tile_first.size == 0
    # an empty split
    plan = gauc.group_plan(np.zeros(0, np.int32))
    assert plan.order.size == 0 and plan.group_off.tolist() == [0] and plan.tile_group.size == 0
    # a single user: one group, here of three tiles
    plan = gauc.group_plan(np.full(600, 5))
    assert plan.order.tolist() == list(range(600)) and plan.group_off.tolist() == [0, 600]
    assert plan.tile_group.tolist() == [0, 0, 0] and plan.tile_first.tolist() == [0, 256, 512]
    plan = gauc.group_plan([3])
    assert plan.order.tolist() == [0] and plan.group_off.tolist() == [0, 1]


# ------------------------------------------------------------------ the host definition
def test_group_auc_host_hand_computed():
    # user 1: positives .9 .5, negatives .5 .1 -> pairs (.9,.5) 2 (.9,.1) 2 (.5,.5) 1 (.5,.1) 2: T 7, AUC 7/8
    # user 2: all positive (left out); user 3: all negative (left out)
    # user 4: positive .2, negatives .7 .2 .1 (r 4) -> 0 + 1 + 2 = 3, AUC 3/6
    uid = [1, 2, 1, 4, 3, 1, 4, 2, 1, 4, 4, 3]
    pred = [.9, .3, .5, .2, .8, .5, .7, .6, .1, .2, .1, .4]
    lab = [1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    r = gauc.group_auc_host(pred, lab, uid, want_groups=True)
    assert r["uid"].tolist() == [1, 2, 3, 4] and r["rows"].tolist() == [4, 2, 2, 4]
    assert r["T"].tolist() == [7, 0, 0, 3] and r["P"].tolist() == [2, 2, 0, 1]
    assert r["T"].dtype == np.uint64 and r["P"].dtype == np.uint32
    assert (r["n_groups"], r["n_valid"], r["rows_valid"]) == (4, 2, 8)
    assert r["gauc"] == (4 * (7 / 8.0) + 4 * (3 / 6.0)) / 8          # weighting by r_u
    # weighting: a 2-row user with AUC 1 beside a 6-row user with AUC 0
    r = gauc.group_auc_host([.9, .1, .1, .1, .1, .9, .9, .9], [1, 0, 1, 1, 1, 0, 0, 0], [0, 0, 1, 1, 1, 1, 1, 1])
    assert r["gauc"] == (2 * 1.0 + 6 * (0 / 18.0)) / 8 and r["rows_valid"] == 8
    # NaN below -inf, NaN == NaN, -0 == +0
    ninf = -np.inf
    r = gauc.group_auc_host([NAN, ninf, NAN, -0.0, 0.0, ninf, NAN], [1, 0, 0, 1, 0, 1, 0], [0, 0, 0, 1, 1, 2, 2], want_groups=True)
    assert r["T"].tolist() == [0 + 1, 1, 2] and r["P"].tolist() == [1, 1, 1]
    # labels: anything but 0 is positive, as the eval histogram classifies
    r = gauc.group_auc_host([.9, .1], [0.5, 0.0], [0, 0], want_groups=True)
    assert r["T"].tolist() == [2] and r["gauc"] == 1.0
    # nobody is valid: 0.0 with n_valid 0 (recommend.ranking_metrics' convention); an empty split
    assert gauc.group_auc_host([.1, .2], [1, 1], [0, 1]) == {"gauc": 0.0, "n_groups": 2, "n_valid": 0, "rows_valid": 0}
    assert gauc.group_auc_host([], [], []) == {"gauc": 0.0, "n_groups": 0, "n_valid": 0, "rows_valid": 0}
    assert gauc.finish(3.0, 4, 2, 5) == {"gauc": 0.75, "n_groups": 5, "n_valid": 2, "rows_valid": 4}
    with pytest.raises(ValueError):
        gauc.group_auc_host([.1], [1, 0], [0, 0])


def test_group_auc_host_against_brute_force():
    """300 users of 1 .. 40 rows in shuffled file order, predictions quantised to 8 levels so ties abound."""
    rs = np.random.RandomState(5)
    sizes = rs.randint(1, 41, 300)
    uid = np.repeat(rs.permutation(5000)[:300], sizes)
    uid = uid[rs.permutation(uid.size)]
    pred = (rs.randint(0, 8, uid.size) / 8.0).astype(np.float32)
    label = (rs.random_sample(uid.size) < 0.3).astype(np.float32)
    want = brute_force(pred, label, uid)
    got = gauc.group_auc_host(pred, label, uid, want_groups=True)
    assert got["uid"].tolist() == sorted(want)
    assert got["T"].tolist() == [want[u][0] for u in sorted(want)]
    assert got["P"].tolist() == [want[u][1] for u in sorted(want)]
    assert got["rows"].tolist() == [want[u][2] for u in sorted(want)]
    ref = report_of(want)
    assert (got["n_groups"], got["n_valid"], got["rows_valid"]) == (300, ref["n_valid"], ref["rows_valid"])
    assert 0 < ref["n_valid"] < 300
    assert abs(got["gauc"] - ref["gauc"]) <= 300 * 2.0 ** -52 * ref["gauc"]        # two summation orders of 300 terms
    # a different file order of the same rows: the same integers, the same scalar to the bit
    p = rs.permutation(uid.size)
    again = gauc.group_auc_host(pred[p], label[p], uid[p], want_groups=True)
    assert again["T"].tolist() == got["T"].tolist() and again["gauc"] == got["gauc"]


# ------------------------------------------------------------------ run.py --gauc over a CPU stand-in
def result_json(tmp_path, cfg):
    rdir = os.path.join(str(tmp_path / "result"), cfg["model"]["name"], "Taobao", cfg["dataset"]["domain_split_path"])
    runs = os.listdir(rdir)
    assert len(runs) == 1
    with open(os.path.join(rdir, runs[0], "result.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr"])
def test_run_gauc_flag_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    cfg = tiny_config(tmp_path, name, epochs=2, report_gauc=True)
    built = []
    res = cli.main(cfg, ReportingFakeEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}                  # still (loss, auc) per domain
    model = built[0]
    assert ReportingFakeEngine.seen and all(kw == {"want_gauc": True} for kw in ReportingFakeEngine.seen)
    result = result_json(tmp_path, cfg)
    assert set(result) == {"avg_loss", "avg_auc", "domain_loss", "domain_auc", "avg_gauc", "weighted_gauc", "domain_gauc",
                           "domain_gauc_users"}
    assert set(result["domain_gauc"]) == set(result["domain_gauc_users"]) == {"0", "1", "2"}
    # the saved values are those of the LAST test evaluation of every domain
    last = {}
    for d, split, report_name, weights, report in ReportingFakeEngine.log:
        if split == "test" and report_name == "gauc":
            last[d] = (weights, report)
    valid = [d for d in range(3) if last[d][1]["n_valid"] > 0]
    assert valid, "the stand-in's test splits hold no user with both classes"
    for d in range(3):
        assert result["domain_gauc"][str(d)] == last[d][1]["gauc"] and 0.0 <= last[d][1]["gauc"] <= 1.0
        assert result["domain_gauc_users"][str(d)] == last[d][1]["n_valid"]
    assert result["avg_gauc"] == sum(last[d][1]["gauc"] for d in valid) / len(valid)
    rows = sum(last[d][1]["rows_valid"] for d in valid)
    assert result["weighted_gauc"] == sum(last[d][1]["rows_valid"] * last[d][1]["gauc"] for d in valid) / rows
    # the printed lines: a GAUC block per domain behind the AUC block, then the overall line
    text = capsys.readouterr().out
    tail = text[text.rindex("Overall test Loss:"):]
    assert re.search(r"^GAUC: \n0: [\d.e-]+\n1: [\d.e-]+\n2: [\d.e-]+\nOverall test GAUC: [\d.e-]+, Weighted GAUC: [\d.e-]+$",
                     tail, flags=re.M), tail
    assert "Overall test GAUC: {}, Weighted GAUC: {}".format(result["avg_gauc"], result["weighted_gauc"]) in tail
    assert text.count("Overall val GAUC:") >= 1
    if name == "mlp_meta_mamdr":
        # every domain was scored under ITS merged weights: theta (+) phi_d of the best checkpoint
        from oracle import outer as oouter
        eng = model.model
        for d in range(3):
            merged = oouter.merge(model.best_shared_weights.numpy(), model.best_domain_weights[d].numpy(),
                                  cfg["train"]["merged_method"])
            assert np.array_equal(last[d][0], merged), d
            eng.set_weights(torch.from_numpy(merged.copy()))
            cols = eng.data[(d, "test")]
            _, preds = eng.oracle.evaluate(cols, eng.batch_size)
            again = gauc.group_auc_host(preds, cols["label"], cols["uid"])
            assert again == last[d][1] and result["domain_gauc"][str(d)] == again["gauc"]
        assert len({last[d][0].tobytes() for d in range(3)}) == 3            # three different weight vectors


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch, capsys):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    cfg = tiny_config(tmp_path, "mlp", epochs=1)
    without = cli.main(cfg, ReportingFakeEngine)
    assert ReportingFakeEngine.seen and all(kw == {} for kw in ReportingFakeEngine.seen)          # evaluate never receives want_gauc
    assert set(result_json(tmp_path, cfg)) == {"avg_loss", "avg_auc", "domain_loss", "domain_auc"}
    assert "GAUC" not in capsys.readouterr().out
    # ... and the flag changes neither the returned tuple nor what was saved before
    cfg2 = tiny_config(tmp_path / "b", "mlp", epochs=1, report_gauc=True)
    assert cli.main(cfg2, ReportingFakeEngine) == without
    both = result_json(tmp_path / "b", cfg2)
    assert {k: both[k] for k in ("avg_loss", "avg_auc", "domain_loss", "domain_auc")} == result_json(tmp_path, cfg)
    # the command line: --gauc sets train.report_gauc, its absence calls main exactly as before
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--gauc"])
    assert seen[0][1] == {} and len(seen[0][0]) == 1 and "report_gauc" not in seen[0][0][0]["train"]
    assert seen[1][1] == {} and len(seen[1][0]) == 1 and seen[1][0][0]["train"]["report_gauc"] is True


def test_lanes_refuse_report_gauc_by_name(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr", report_gauc=True, lanes=2)
    with pytest.raises(NotImplementedError, match="report_gauc"):
        cli.main(cfg, ReportingFakeEngine)
    assert not loaded                    # refused before the data is loaded
