"""Exact AUC, average precision and calibration, host side (no GPU): the C ABI's declaration, binding and device-free
refusals, `exact.metrics_host` against scikit-learn and against `gauc.group_auc_host`, the bins' invariants, the measured gap
between the 500-threshold AUC and the exact one that motivates the feature, and `run.py --exact-metrics` end to end over a
CPU stand-in of the engine whose `evaluate` honours `want_exact` through `metrics_host`."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from fake_engine import ReportingFakeEngine
from mamdr_amd import _lib, cli, exact, gauc
from oracle import auc as oauc
from test_gauc_host import patch_emb_dim, result_json, tiny_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
NAN = float("nan")


# ------------------------------------------------------------------ C ABI
def test_exact_metrics_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    m = re.search(r"\bint\s+mamdr_exact_metrics\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m, "mamdr_exact_metrics is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* d_pred", "const float* d_label", "int64_t n", "int32_t n_bins", "int64_t* d_counts",
                      "double* d_ap", "int64_t* d_bins", "int64_t* d_sorted_out", "void* stream"], params
    assert header.index("int mamdr_group_auc") < header.index("int mamdr_exact_metrics") < header.index("int mamdr_gram(")
    doc = header[:header.index("int mamdr_exact_metrics")].rsplit("/*", 1)[1]
    flat = lambda s: " ".join(s.replace(" * ", " ").replace("`", "").split())      # noqa: E731 (the comment's line starts)
    assert "NO REFERENCE COUNTERPART" in doc and "Added within ABI 19" in doc
    for phrase in ("NaN is lowest and equals NaN, -0 equals +0", "positive is label != 0",
                   "The composite is (uint64) key << 1 | positive", "Inside a run of equal keys the negatives come first",
                   "rs(i) is the first position of i's run of equal keys",
                   "cp(i) is the number of positives at positions < i", "cn(i) = i - cp(i)",
                   "T = sum_{i positive} (cn(rs(i)) + cn(i))", "2 #{s_p > s_n} + #{s_p == s_n}",
                   "sum_{i positive} (double)(P - cp(rs(i))) / (double)(n - rs(i))", "floor(rs(i) n_bins / n)",
                   "floor(clamp(p, 0, 1) 2^32 + 0.5)", "A NaN prediction adds 0 and is counted in n_nan",
                   "A tie run is never split across bins"):
        assert phrase in flat(doc) and phrase in flat(exact.__doc__), phrase
    for phrase in ("EMPTY or UNEQUAL", "No floating-point atomics", "hipMallocAsync / hipFreeAsync",
                   "under any permutation of the rows", "n = 0 writes zeros"):
        assert phrase in flat(doc), phrase
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_exact_metrics"] == (C.c_int, [vp, vp, i64, i32, vp, vp, vp, vp, vp])
    assert _lib.ABI_VERSION == 19 and re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert re.search(r"#define\s+MAMDR_EXACT_MAX_BINS\s+%d\b" % exact.MAX_BINS, header)


def test_the_tile_constants_are_the_kernels():
    """exact.SORT_TILE and its kin are what csrc/mamdr_kernels.h compiles in (the GPU tests size their cases by them)."""
    text = open(os.path.join(ROOT, "mamdr_amd", "csrc", "mamdr_kernels.h")).read()
    for name in ("RADIX_BITS", "SORT_TILE", "SCAN_TILE", "METRIC_TILE", "MAX_BINS"):
        m = re.search(r"constexpr int EXACT_%s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(exact, name), name
    from mamdr_amd import build
    flags = dict(build.SOURCES)["exact_kernels.hip"]
    assert "-ffp-contract=off" in flags and "-Rpass-analysis=kernel-resource-usage" in flags


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    x = C.c_void_p(64)            # never dereferenced: every case below is refused before any device call

    def call(pred=x, label=x, n=8, bins=10, counts=x, ap=x, out=x, sorted_out=None):
        return lib.mamdr_exact_metrics(pred, label, n, bins, counts, ap, out, sorted_out, None)
    cases = {"null counts": dict(counts=None), "null ap": dict(ap=None), "null bins": dict(out=None),
             "null pred": dict(pred=None), "null label": dict(label=None), "n < 0": dict(n=-1), "n = 2^31": dict(n=2 ** 31),
             "no bins": dict(bins=0), "negative bins": dict(bins=-3), "too many bins": dict(bins=4097),
             "misaligned pred": dict(pred=C.c_void_p(66)), "misaligned label": dict(label=C.c_void_p(65)),
             "misaligned counts": dict(counts=C.c_void_p(68)), "misaligned ap": dict(ap=C.c_void_p(68)),
             "misaligned bins": dict(out=C.c_void_p(68)), "misaligned sorted_out": dict(sorted_out=C.c_void_p(68))}
    for what, kw in cases.items():
        assert call(**kw) == _lib.EINVAL, what
        assert b"mamdr_exact_metrics" in lib.mamdr_last_error(), what
    with pytest.raises(_lib.MamdrError, match="n_bins 4097 outside 1..4096"):
        _lib.check(call(bins=4097))


# ------------------------------------------------------------------ the host definition
def draws(n, seed, levels=None, rate=0.2):
    rs = np.random.RandomState(seed)
    pred = rs.random_sample(n).astype(F32)
    if levels:
        pred = (np.floor(pred * levels) / levels).astype(F32)
    label = (rs.random_sample(n) < rate * (0.5 + pred)).astype(F32)
    return pred, label


@pytest.mark.parametrize("levels", [None, 3, 8])
@pytest.mark.parametrize("n", [50, 3001, 20000])
def test_metrics_host_against_scikit_learn(n, levels):
    """1e-10 absolute: fp64 rounding at these n is around 1e-16, one mishandled tie moves AUC by at least 1 / (2 P N) >= 5e-9."""
    metrics = pytest.importorskip("sklearn.metrics")
    pred, label = draws(n, 11 + n, levels)
    rep = exact.finish(*exact.metrics_host(pred, label, 10))
    assert rep["valid"] == 1 and rep["P"] + rep["N"] == n and rep["P"] == int(label.sum())
    assert rep["n_runs"] == np.unique(pred).size and rep["n_nan"] == 0
    auc = metrics.roc_auc_score(label, pred.astype(np.float64))
    ap = metrics.average_precision_score(label, pred.astype(np.float64))
    print("n %d levels %s: auc %.17g (sklearn differs by %.2e), ap %.17g (%.2e)"
          % (n, levels, rep["auc"], rep["auc"] - auc, rep["ap"], rep["ap"] - ap))
    assert abs(rep["auc"] - auc) <= 1e-10
    assert abs(rep["ap"] - ap) <= 1e-10


def test_hand_computed():
    # sorted: .1- .2- .2+ .5- .5+ .5+ .9+ -> T = (1+2) + (2+3) + (2+3) + (3+3) = 19 of 2 * 4 * 3
    pred = [.5, .9, .2, .1, .5, .2, .5]
    lab = [1, 1, 0, 0, 1, 1, 0]
    counts, ap_sum, bins, srt = exact.metrics_host(pred, lab, 7, want_sorted=True)
    assert counts.tolist() == [19, 4, 3, 4, 0] and counts.dtype == np.int64
    # per positive (P - cp(rs)) / (n - rs): .2+ 4/6, .5+ 3/4 twice, .9+ 1/1
    assert ap_sum == 4 / 6.0 + 3 / 4.0 + 3 / 4.0 + 1.0
    assert bins[0].tolist() == [1, 2, 0, 3, 0, 0, 1] and bins[1].tolist() == [0, 1, 0, 2, 0, 0, 1]      # a run is one bin
    q = lambda p: int(np.floor(np.float64(F32(p)) * 2.0 ** 32 + 0.5))      # noqa: E731
    assert bins[2].tolist() == [q(.1), 2 * q(.2), 0, 3 * q(.5), 0, 0, q(.9)]
    assert srt.dtype == np.int64 and np.array_equal(srt, np.sort(exact.composites(pred, lab)).astype(np.int64))
    rep = exact.finish(counts, ap_sum, bins)
    assert rep["auc"] == 19 / 24.0 and rep["ap"] == ap_sum / 4 and rep["valid"] == 1
    mean = np.array([q(.1), q(.2), 0, q(.5), 0, 0, q(.9)]) / 2.0 ** 32
    want_ece = (1 * abs(mean[0] - 0) + 2 * abs(mean[1] - .5) + 3 * abs(mean[3] - 2 / 3.0) + 1 * abs(mean[6] - 1)) / 7
    assert abs(rep["ece"] - want_ece) < 1e-15
    assert abs(rep["pcoc"] - (q(.1) + 2 * q(.2) + 3 * q(.5) + q(.9)) / 2.0 ** 32 / 4) < 1e-15
    # NaN lowest and equal to NaN, -0 == +0, values outside [0, 1] clamp in the bins only; labels: anything but 0
    counts, ap_sum, bins = exact.metrics_host([NAN, -np.inf, NAN, -0.0, 0.0, 2.5, -3.0], [2.0, 0, 0, -1.0, 0, 1, 0], 1)
    # sorted: nan- nan+ -inf- -3- 0- 0+ 2.5+: T = (0+1) + (3+4) + (4+4) = 16; five runs; two NaNs
    assert counts.tolist() == [16, 3, 4, 5, 2] and bins.tolist() == [[7], [3], [2 ** 32]]
    # one class only: 0.0 with valid 0 (recommend.ranking_metrics' convention); an empty split
    rep = exact.report_host([.1, .2], [1, 1], 4)
    assert (rep["auc"], rep["valid"], rep["ap"], rep["P"], rep["N"]) == (0.0, 0, 1.0, 2, 0)
    rep = exact.report_host([.1, .2], [0, 0], 4)
    assert (rep["auc"], rep["valid"], rep["ap"], rep["pcoc"]) == (0.0, 0, 0.0, 0.0)
    counts, ap_sum, bins, srt = exact.metrics_host([], [], 3, want_sorted=True)
    assert counts.tolist() == [0] * 5 and ap_sum == 0.0 and bins.tolist() == [[0] * 3] * 3 and srt.size == 0
    assert exact.finish(counts, ap_sum, bins)["ece"] == 0.0
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            exact.metrics_host([.1], [1], bad)
    with pytest.raises(ValueError):
        exact.metrics_host([.1], [1, 0], 2)


@pytest.mark.parametrize("levels", [None, 8])
def test_T_and_P_are_group_auc_hosts(levels):
    pred, label = draws(5000, 3, levels)
    pred[::97] = NAN
    pred[5::89] = -0.0
    counts = exact.metrics_host(pred, label, 5)[0]
    one = gauc.group_auc_host(pred, label, np.zeros(pred.size, np.int32), want_groups=True)
    assert int(one["T"][0]) == counts[0] and int(one["P"][0]) == counts[1]
    assert counts[4] == np.isnan(pred).sum() and counts[2] == pred.size - counts[1]


@pytest.mark.parametrize("n_bins", [1, 10, 64, 4096])
@pytest.mark.parametrize("levels", [None, 3, 50])
def test_bins_hold_every_row_once_and_no_run_straddles(levels, n_bins):
    pred, label = draws(3000, 5, levels)
    counts, _, bins, srt = exact.metrics_host(pred, label, n_bins, want_sorted=True)
    assert bins[0].sum() == 3000 and bins[1].sum() == counts[1]
    assert np.all(bins[1] <= bins[0]) and np.all(bins[2] <= bins[0] * 2 ** 32)
    key = srt >> 1
    edges = np.cumsum(bins[0])[:-1]
    edges = edges[(edges > 0) & (edges < 3000)]
    assert np.all(key[edges] != key[edges - 1])              # every bin boundary is a run boundary
    if levels is None and n_bins == 10:
        assert bins[0].min() >= 295 and bins[0].max() <= 305          # distinct predictions: equal mass up to a tie
    if levels == 3:
        assert np.count_nonzero(bins[0]) <= 3                # three runs: three bins at the most, the others EMPTY


def test_summarise():
    reps = {0: exact.report_host([.1, .9, .5, .3], [0, 1, 1, 0], 2), 1: exact.report_host([.1, .9], [1, 0], 2),
            2: exact.report_host([.2, .4], [1, 1], 2)}
    s = exact.summarise(reps)
    assert s["auc"] == ((1.0 + 0.0) / 2, (4 * 1.0 + 2 * 0.0) / 6)         # domain 2 is not valid: left out of both
    assert s["ap"][0] == (reps[0]["ap"] + reps[1]["ap"]) / 2
    assert exact.summarise({2: reps[2]}) == {"auc": (0.0, 0.0), "ap": (0.0, 0.0), "ece": (0.0, 0.0)}


# ------------------------------------------------------------------ the motivation, pinned
# (logit mean, spread) and the row README.md tables: positive rate, |AUC-500 - exact|
EXPERIMENTS = [((0.0, 1.0), 0.50, 4e-6), ((-3.5, 0.6), 0.034, 2.4e-4), ((-4.55, 0.5), 0.012, 2.1e-3), ((-5.9, 0.42), 0.003, 2.1e-2)]


@pytest.mark.parametrize("case", EXPERIMENTS, ids=lambda c: "rate%g" % c[1])
def test_auc500_is_off_by_the_tabled_amount(case):
    """200,000 rows, logit ~ N(mu, sigma), labels drawn from the prediction; both metrics see the same fp32 predictions,
    AUC-500 from oracle/auc.py in batches of 20,000.  |AUC-500 - exact| lies within 20 % of README.md's row.  One draw is
    one sample: other seeds scatter by a few tens of per cent around the rows (the first row, at the level of the
    thresholds' rounding, even in sign); RandomState(2) is a draw inside all four bands."""
    (mu, sigma), rate, tabled = case
    rs = np.random.RandomState(2)
    logit = rs.normal(mu, sigma, 200000)
    pred = (1 / (1 + np.exp(-logit))).astype(F32)
    label = (rs.random_sample(200000) < pred).astype(F32)
    rep = exact.report_host(pred, label, 20)
    a500 = float(oauc.auc500(label, pred, 20000))
    print("rate %.4f: AUC-500 %.5f exact %.5f difference %.3e (tabled %.1e)" % (label.mean(), a500, rep["auc"], a500 - rep["auc"], tabled))
    assert abs(label.mean() - rate) <= 0.05 * rate
    assert abs(abs(a500 - rep["auc"]) - tabled) <= 0.2 * tabled
    assert rep["ece"] < 5e-3                  # labels drawn from the predictions: calibrated by construction


# ------------------------------------------------------------------ run.py --exact-metrics over a CPU stand-in
OLD_KEYS = {"avg_loss", "avg_auc", "domain_loss", "domain_auc"}
NEW_KEYS = {"domain_auc_exact", "avg_auc_exact", "weighted_auc_exact", "domain_ap", "domain_ece", "domain_pcoc"}
GAUC_KEYS = {"avg_gauc", "weighted_gauc", "domain_gauc", "domain_gauc_users"}


def run_folder(tmp_path, cfg):
    rdir = os.path.join(str(tmp_path / "result"), cfg["model"]["name"], "Taobao", cfg["dataset"]["domain_split_path"])
    runs = os.listdir(rdir)
    assert len(runs) == 1
    return os.path.join(rdir, runs[0])


@pytest.mark.parametrize("name,with_gauc", [("mlp", False), ("mlp_meta_mamdr", True)])
def test_run_exact_flag_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name, with_gauc):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    extra = dict(report_gauc=True) if with_gauc else {}
    cfg = tiny_config(tmp_path, name, epochs=2, report_exact=7, **extra)
    res = cli.main(cfg, ReportingFakeEngine)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}                  # still (loss, auc) per domain
    want_kw = dict(want_exact=7, **({"want_gauc": True} if with_gauc else {}))
    assert ReportingFakeEngine.seen and all(kw == want_kw for kw in ReportingFakeEngine.seen)
    result = result_json(tmp_path, cfg)
    assert set(result) == OLD_KEYS | NEW_KEYS | (GAUC_KEYS if with_gauc else set())
    last = {d: rep for d, split, name, _, rep in ReportingFakeEngine.log if split == "test" and name == "exact"}          # the LAST test evaluation of every domain
    for d in range(3):
        assert result["domain_auc_exact"][str(d)] == last[d]["auc"] and 0.0 < last[d]["auc"] < 1.0
        for key in ("ap", "ece", "pcoc"):
            assert result["domain_" + key][str(d)] == last[d][key]
    assert all(last[d]["valid"] for d in range(3))
    rows = [last[d]["P"] + last[d]["N"] for d in range(3)]
    assert result["avg_auc_exact"] == sum(last[d]["auc"] for d in range(3)) / 3
    assert result["weighted_auc_exact"] == sum(rows[d] * last[d]["auc"] for d in range(3)) / sum(rows)
    folder = run_folder(tmp_path, cfg)
    assert sorted(os.listdir(folder)) == ["config.json.example", "dataset_info.json", "exact_metrics.npz",
                                          "model_parameters.npz", "result.json"]
    with np.load(os.path.join(folder, "exact_metrics.npz")) as z:
        assert sorted(z.files) == ["bin_positives", "bin_pred_sum", "bin_rows", "domains"]
        assert z["domains"].tolist() == [0, 1, 2]
        for i, d in enumerate(z["domains"].tolist()):
            for key in ("bin_rows", "bin_positives", "bin_pred_sum"):
                assert z[key].shape == (3, 7) and np.array_equal(z[key][i], last[d][key]), key
            assert z["bin_rows"][i].sum() == rows[d]
    # the printed lines: the three blocks per domain behind the AUC (and GAUC) block, each with its overall line
    text = capsys.readouterr().out
    tail = text[text.rindex("Overall test Loss:"):]
    num = r"[\d.e-]+"
    for label in ("Exact AUC", "AP", "ECE"):
        assert re.search(r"^%s: \n0: %s\n1: %s\n2: %s\nOverall test %s: %s, Weighted %s: %s$"
                         % (label, num, num, num, label, num, label, num), tail, flags=re.M), (label, tail)
    assert "Overall test Exact AUC: {}, Weighted Exact AUC: {}".format(result["avg_auc_exact"], result["weighted_auc_exact"]) in tail
    assert text.count("Overall val Exact AUC:") >= 1
    if with_gauc:
        assert tail.index("Overall test GAUC:") < tail.index("Exact AUC: ")


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch, capsys):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    cfg = tiny_config(tmp_path, "mlp", epochs=1)
    without = cli.main(cfg, ReportingFakeEngine)
    assert ReportingFakeEngine.seen and all(kw == {} for kw in ReportingFakeEngine.seen)          # evaluate never receives want_exact
    assert set(result_json(tmp_path, cfg)) == OLD_KEYS
    assert sorted(os.listdir(run_folder(tmp_path, cfg))) == ["config.json.example", "dataset_info.json", "model_parameters.npz",
                                                             "result.json"]
    out = capsys.readouterr().out
    assert "Exact AUC" not in out and "ECE" not in out and "AP:" not in out
    # ... and the flag changes neither the returned tuple nor what was saved before: decisions stay on AUC-500
    cfg2 = tiny_config(tmp_path / "b", "mlp", epochs=1, report_exact=20)
    assert cli.main(cfg2, ReportingFakeEngine) == without
    both = result_json(tmp_path / "b", cfg2)
    assert {k: both[k] for k in OLD_KEYS} == result_json(tmp_path, cfg)
    # the command line: --exact-metrics [B] sets train.report_exact, its absence calls main exactly as before
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--exact-metrics"])
    cli.cli(["--config", cfg_path, "--exact-metrics", "64", "--gauc"])
    assert [(len(a), k) for a, k in seen] == [(1, {})] * 3
    assert "report_exact" not in seen[0][0][0]["train"]
    assert seen[1][0][0]["train"]["report_exact"] == 20 and "report_gauc" not in seen[1][0][0]["train"]
    assert seen[2][0][0]["train"]["report_exact"] == 64 and seen[2][0][0]["train"]["report_gauc"] is True
    for bad in ("0", "4097"):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path, "--exact-metrics", bad])


def test_lanes_refuse_report_exact_by_name(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr", report_exact=20, lanes=2)
    with pytest.raises(NotImplementedError, match="train.report_exact"):
        cli.main(cfg, ReportingFakeEngine)
    assert not loaded                    # refused before the data is loaded


def test_documents_carry_the_feature():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--exact-metrics" in readme and "| 0.3 % | 0.59431 | 0.61499 | -2.1e-2 |" in readme
    for word in ("mamdr_exact_metrics", "k_exact_scatter", "k_exact_metrics", "exact_metrics_bench"):
        assert word in design, word
