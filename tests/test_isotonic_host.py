"""Isotonic recalibration and the CORP decomposition, host side (mamdr_amd/isotonic.py): the host definition against an
independent PAV in `fractions.Fraction` and against scikit-learn, the CORP identity, the special values, `apply_host`, the
command line, the refusal under lanes / processes, the report over a CPU stand-in engine, and the C ABI's declarations and
refusals (which need no device).  tests/test_gpu_isotonic.py takes its cases from here."""
import ctypes as C
import json
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import test_gauc_host as gh          # tiny_config, patch_emb_dim
from fake_engine import FakeEngine
from mamdr_amd import _lib, cli, exact, gauc, isotonic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

SPECIALS = (np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 0.5, 0.5, np.nan, 1.0, 1e-45], F32),
            np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 0], F32))

_CACHE = {}


# ------------------------------------------------------------------ the cases (shared with the GPU tests)
def pav_fraction(pred, label):
    """PAV over the runs with exact rational means -> (first_key, rows, positives)."""
    key, rows, pos = isotonic.runs_host(pred, label)
    blocks = []
    for k, r, s in zip(key.tolist(), rows.tolist(), pos.tolist()):
        blocks.append([k, r, s])
        while len(blocks) >= 2 and Fraction(blocks[-2][2], blocks[-2][1]) >= Fraction(blocks[-1][2], blocks[-1][1]):
            b = blocks.pop()
            blocks[-1][1] += b[1]
            blocks[-1][2] += b[2]
    a = np.array(blocks, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint32), a[:, 1], a[:, 2]


def hull_fit(pred, label):
    """the definition's other wording: the strict vertices of the lower hull of Q_0 .. Q_R by one monotone chain."""
    key, rows, pos = isotonic.runs_host(pred, label)
    X = np.concatenate([[0], np.cumsum(rows)]).tolist()
    Y = np.concatenate([[0], np.cumsum(pos)]).tolist()
    st = []
    for j in range(len(X)):
        while len(st) >= 2 and (X[st[-1]] - X[st[-2]]) * (Y[j] - Y[st[-1]]) - (Y[st[-1]] - Y[st[-2]]) * (X[j] - X[st[-1]]) <= 0:
            st.pop()
        st.append(j)
    st = np.array(st)
    return key[st[:-1]], np.diff(np.asarray(X, np.int64)[st]), np.diff(np.asarray(Y, np.int64)[st])


def cases():
    """the 200 seeded random cases (n in 1 .. 399; predictions quantised to 1/4, 1/16, 1/64 and to 2^-20, i.e. unquantised
    for fp32 purposes) and, drawn from the same generator behind them, the two 5,000-row draws of the GPU tests
    -> {"random": [(pred, label)] * 200, "q64": (pred, label), "continuous": (pred, label)}; read-only."""
    if "cases" not in _CACHE:
        rng = np.random.default_rng(0)
        out = {"random": []}
        for _ in range(200):
            n = int(rng.integers(1, 400))
            q = int(rng.choice([4, 16, 64, 1 << 20]))
            logit = rng.normal(-2, 1.5, n)
            p = (1 / (1 + np.exp(-logit))).astype(F32)
            p = (np.round(p * q) / q).astype(F32)
            y = (rng.random(n) < 1 / (1 + np.exp(-logit * rng.choice([1, 0.3, -1])))).astype(F32)
            out["random"].append((p, y))
        for name, q in (("q64", 64), ("continuous", 1 << 20)):
            logit = rng.normal(-2, 1.5, 5000)
            p = (1 / (1 + np.exp(-logit))).astype(F32)
            p = (np.round(p * q) / q).astype(F32)
            out[name] = (p, (rng.random(5000) < 1 / (1 + np.exp(-logit))).astype(F32))
        for pair in out["random"] + [out["q64"], out["continuous"]]:
            for a in pair:
                a.setflags(write=False)
        _CACHE["cases"] = out
    return _CACHE["cases"]


def convex_case():
    """one run per distinct fraction a / b (1 <= b <= 11, 0 <= a <= b) in ascending order: run j at prediction (j + 1) / 44
    with b rows, a of them positive -- strictly increasing rates: every run is its own block."""
    rates = sorted({Fraction(a, b) for b in range(1, 12) for a in range(0, b + 1)})
    p, y = [], []
    for j, f in enumerate(rates):
        p += [F32(j + 1) / F32(len(rates) + 1)] * f.denominator
        y += [1.0] * f.numerator + [0.0] * (f.denominator - f.numerator)
    return np.array(p, F32), np.array(y, F32), len(rates)


def same_fit(got, want):
    for g, w, what in zip(got, want, ("first_key", "rows", "positives")):
        assert np.array_equal(g, w), what


# ------------------------------------------------------------------ the fit
def test_fit_host_equals_the_fraction_pav_and_the_hull():
    for i, (p, y) in enumerate(cases()["random"]):
        counts, fk, rows, pos = isotonic.fit_host(p, y)
        same_fit((fk, rows, pos), pav_fraction(p, y))
        same_fit((fk, rows, pos), hull_fit(p, y))
        n, P = len(p), int((y != 0).sum())
        assert counts.tolist() == [len(fk), len(np.unique(gauc.ordered_key(p))), 0, P], i
        assert rows.sum() == n and pos.sum() == P and fk.dtype == np.uint32 and rows.dtype == pos.dtype == np.int64
        means = [Fraction(int(s), int(r)) for s, r in zip(pos, rows)]
        assert all(a < b for a, b in zip(means, means[1:])), i           # strictly increasing
        assert np.all(fk[1:] > fk[:-1])


def test_fitted_values_match_scikit_learn_on_the_fitted_rows():
    sk = pytest.importorskip("sklearn.isotonic")
    for i, (p, y) in enumerate(cases()["random"]):
        _, fk, rows, pos = isotonic.fit_host(p, y)
        ir = sk.IsotonicRegression(out_of_bounds="clip").fit(p.astype(np.float64), y.astype(np.float64))
        got = isotonic.apply_host(fk, rows, pos, p)
        assert got.dtype == F32 and np.abs(got - ir.predict(p.astype(np.float64))).max() <= 1e-6, i


def test_corp_identity():
    for i, (p, y) in enumerate(cases()["random"]):
        _, fk, rows, pos = isotonic.fit_host(p, y)
        brier, _ = isotonic.score_sums_host(p, y)
        S = brier / len(p)
        c = isotonic.corp(rows, pos, S)
        assert abs(S - (c["mcb"] - c["dsc"] + c["unc"])) <= 1e-15, i
        assert c["mcb"] >= -1e-15 and c["dsc"] >= -1e-15, (i, c)
    assert isotonic.corp(np.zeros(0, np.int64), np.zeros(0, np.int64), 0.0) == {"mcb": 0.0, "dsc": 0.0, "unc": 0.0}


def test_specials():
    p, y = SPECIALS
    counts, fk, rows, pos = isotonic.fit_host(p, y)
    assert rows.tolist() == [6, 2, 2] and pos.tolist() == [2, 1, 2]
    assert counts.tolist() == [3, 7, 2, 5]                      # runs: NaN, -inf, +-0, 1e-45, 0.5, 1, +inf
    same_fit((fk, rows, pos), pav_fraction(p, y))
    got = isotonic.apply_host(fk, rows, pos, p)
    want = np.array([1 / 3, 1 / 3, 1 / 3, 1, 1 / 3, .5, .5, 1 / 3, 1, 1 / 3], np.float64).astype(F32)
    assert got.tobytes() == want.tobytes()
    t = isotonic.table(counts, fk, rows, pos)
    assert t["n"] == 10 and t["n_nan"] == 2 and np.isnan(t["first_pred"][0]) and t["first_pred"][1:].tolist() == [0.5, 1.0]


def test_small_and_degenerate_fits():
    for p, y, want in (([0.3], [1], ([1], [1])), ([0.3], [0], ([1], [0])), ([0.3, 0.3], [1, 0], ([2], [1])),
                       ([.1, .2, .3, .4], [0, 0, 0, 0], ([4], [0])), ([.1, .2, .3, .4], [1, 1, 1, 1], ([4], [4])),
                       ([.1, .2, .3, .4], [1, 1, 0, 0], ([4], [2])), ([.1, .2, .3, .4], [0, 1, 0, 1], ([1, 2, 1], [0, 1, 1]))):
        counts, fk, rows, pos = isotonic.fit_host(np.array(p, F32), np.array(y, F32))
        assert (rows.tolist(), pos.tolist()) == want and counts[0] == len(rows)
    counts, fk, rows, pos = isotonic.fit_host(np.zeros(0, F32), np.zeros(0, F32))
    assert counts.tolist() == [0, 0, 0, 0] and fk.size == rows.size == pos.size == 0


def test_the_convex_case_keeps_every_run():
    p, y, n_runs = convex_case()
    counts, fk, rows, pos = isotonic.fit_host(p, y)
    assert len(p) == 328 and n_runs == 43 and counts.tolist() == [43, 43, 0, int(y.sum())]
    for tile in (4, 8, 64):
        assert isotonic.level_counts_host(p, y, tile) == [44] * (isotonic.levels(328, tile) + 1)       # nothing shrinks


def test_levels_are_fixed_by_n_and_tile():
    assert isotonic.levels(0, 4) == 0 and isotonic.levels(3, 4) == 0 and isotonic.levels(4, 4) == 1
    assert isotonic.levels(5000, 4) == 11 and isotonic.levels(5000, 8) == 5 and isotonic.levels(5000, 64) == 2
    assert isotonic.levels(4 * 10 ** 6, 64) == 4 and isotonic.levels(2 ** 31 - 1, 4) <= isotonic.MAX_LEVELS
    p, y = cases()["continuous"]
    alive = isotonic.level_counts_host(p, y, 8)
    assert len(alive) == 6 and alive[0] == isotonic.fit_host(p, y)[0][1] + 1 and alive[-1] < alive[0] // 8
    assert all(a >= b for a, b in zip(alive, alive[1:])) and alive[-1] >= isotonic.fit_host(p, y)[0][0] + 1


# ------------------------------------------------------------------ apply, sums
def test_apply_host_below_at_between_above_and_nan():
    fk = gauc.ordered_key(np.array([0.25, 0.5, 0.75], F32))
    rows, pos = np.array([4, 4, 2], np.int64), np.array([1, 2, 2], np.int64)
    x = np.array([-np.inf, -1.0, 0.0, 0.2499, 0.25, 0.3, np.nextafter(F32(0.5), F32(0)), 0.5, 0.74, 0.75, 2.0, np.inf, np.nan], F32)
    want = np.array([.25, .25, .25, .25, .25, .25, .25, .5, .5, 1, 1, 1, .25], F32)
    assert isotonic.apply_host(fk, rows, pos, x).tobytes() == want.tobytes()
    assert isotonic.apply_host(fk, rows, pos, np.zeros(0, F32)).shape == (0,)
    with pytest.raises(ValueError):
        isotonic.apply_host(fk[:0], rows[:0], pos[:0], x)
    assert isotonic.values([3], [1]).tobytes() == F32(np.float64(1) / np.float64(3)).tobytes()


def test_score_sums_host():
    p = np.array([0.0, 1.0, 0.25, 0.75, 2.0, -1.0], F32)
    y = np.array([0, 1, 1, 0, 1, 0], F32)
    brier, ll = isotonic.score_sums_host(p, y)
    assert brier == 0.75 ** 2 * 2 + 1.0 + 1.0
    want = -2 * math.log(1 - 1e-7) - 2 * math.log(0.25) - math.log(1 - 1e-7) - math.log(1 - 1e-7)
    assert abs(ll - want) <= 1e-15 * abs(want)
    worst = isotonic.score_sums_host(np.array([0.0, 1.0], F32), np.array([1, 0], F32))[1]
    assert abs(worst - (-math.log(1e-7) - math.log(1.0 - (1.0 - 1e-7)))) <= 1e-14      # (1 - q is formed in fp64, as defined)
    assert all(math.isnan(v) for v in isotonic.score_sums_host(np.array([0.5, np.nan], F32), np.array([1, 0], F32)))
    assert isotonic.score_sums_host(np.zeros(0, F32), np.zeros(0, F32)) == (0.0, 0.0)
    with pytest.raises(ValueError):
        isotonic.score_sums_host(p, y[:3])


# ------------------------------------------------------------------ the command line
def test_cli_flag_sets_train_isotonic(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--isotonic"])
    cli.cli(["--config", cfg_path, "--isotonic", "4096", "--isotonic-out", "x.npz"])
    assert "isotonic" not in seen[0][0][0]["train"] and "isotonic_out" not in seen[0][0][0]["train"]
    assert seen[1][1] == {} and seen[1][0][0]["train"]["isotonic"] == 20 and "isotonic_out" not in seen[1][0][0]["train"]
    assert seen[2][0][0]["train"]["isotonic"] == 4096 and seen[2][0][0]["train"]["isotonic_out"] == "x.npz"
    for bad in ("0", "4097", "-1"):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path, "--isotonic", bad])


@pytest.mark.parametrize("how", ["lanes", "processes"])
def test_lanes_and_processes_refuse_isotonic_by_name(tmp_path, monkeypatch, how):
    gh.patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    if how == "lanes":
        cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", isotonic=20, lanes=2)
    else:
        cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", isotonic=20)
        monkeypatch.setattr(cli, "init_distributed", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"train\.isotonic \(run\.py --isotonic\).*one process and train\.lanes = 1"):
        cli.main(cfg, FakeEngine)
    assert not loaded                    # refused before the data is loaded


# ------------------------------------------------------------------ the report over a CPU stand-in engine
class IsotonicFakeEngine(FakeEngine):
    """FakeEngine with what BaseModel.isotonic_eval asks of an engine, through the host definitions; `fits` records the
    live weights of every fit."""
    fits = []

    def predict_device(self, domain, split):
        return np.asarray(self.oracle.evaluate(self.data[(domain, split)], self.batch_size)[1], F32)

    def isotonic_fit(self, preds, labels):
        type(self).fits.append(self.weights.numpy().copy())
        return isotonic.table(*isotonic.fit_host(preds, labels))

    def isotonic_apply(self, fit, preds):
        return isotonic.apply_host(fit["first_key"], fit["rows"], fit["positives"], preds)

    def score_sums(self, preds, labels):
        return isotonic.score_sums_host(preds, labels)

    def exact_metrics(self, preds, labels, n_bins):
        return exact.report_host(preds, labels, n_bins)


def test_report_end_to_end_on_the_stand_in(tmp_path, monkeypatch, capsys):
    """cli.main with train.isotonic on a MAMDR run: the report is made under every domain's own merged weights, which are
    put back; result.json and isotonic.npz carry what the issue lists; a run without the key gains nothing."""
    gh.patch_emb_dim(monkeypatch)
    IsotonicFakeEngine.fits = []
    built = []
    cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", isotonic=8)
    cli.main(cfg, IsotonicFakeEngine, on_model=built.append)
    model = built[0]
    eng = model.model
    rdir = [os.path.join(model.result_path, f) for f in os.listdir(model.result_path) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    domains = sorted(model.dataset.test_dataset)
    per_domain = ["domain_brier", "domain_brier_isotonic", "domain_logloss", "domain_logloss_isotonic", "domain_ece_isotonic",
                  "domain_pcoc_isotonic", "domain_mcb", "domain_dsc", "domain_unc", "domain_isotonic_blocks"]
    for key in per_domain:
        assert set(result[key]) == {str(d) for d in domains}, key
    assert "avg_mcb" in result and "weighted_mcb" in result
    live, keep = eng.weights.numpy().copy(), eng.get_weights().clone()
    assert len(IsotonicFakeEngine.fits) == 2 * len(domains)
    with np.load(os.path.join(model.result_path, "isotonic.npz")) as z:
        assert z["domains"].tolist() == domains and int(z["n_bins"]) == 8
        for i, d in enumerate(domains):
            # the fit ran under merge(best theta, best phi_d) ...
            merged = eng.new_vector(meta=True)
            eng.merge(merged, model.best_shared_weights, model.best_domain_weights[d], cfg["train"]["merged_method"])
            eng.assign_meta(merged)
            assert np.array_equal(eng.weights.numpy(), IsotonicFakeEngine.fits[2 * i])
            val_p, test_p = eng.predict_device(d, "val"), eng.predict_device(d, "test")
            eng.set_weights(keep)
            val_y, test_y = eng.data[(d, "val")]["label"], eng.data[(d, "test")]["label"]
            counts, fk, rows, pos = isotonic.fit_host(val_p, val_y)
            assert np.array_equal(z["val_first_key_%d" % d], fk) and np.array_equal(z["val_rows_%d" % d], rows)
            assert np.array_equal(z["val_positives_%d" % d], pos)
            assert z["val_first_pred_%d" % d].tobytes() == exact.prediction_of_key(fk).tobytes()
            t_counts, t_fk, t_rows, t_pos = isotonic.fit_host(test_p, test_y)
            assert np.array_equal(z["test_rows_%d" % d], t_rows) and np.array_equal(z["test_positives_%d" % d], t_pos)
            assert z["counts_%d" % d].tolist() == [counts.tolist() + [len(val_y)], t_counts.tolist() + [len(test_y)]]
            n = len(test_y)
            brier, ll = isotonic.score_sums_host(test_p, test_y)
            b2, ll2 = isotonic.score_sums_host(isotonic.apply_host(fk, rows, pos, test_p), test_y)
            s = str(d)
            assert result["domain_brier"][s] == brier / n and result["domain_logloss"][s] == ll / n
            assert result["domain_brier_isotonic"][s] == b2 / n and result["domain_logloss_isotonic"][s] == ll2 / n
            assert result["domain_isotonic_blocks"][s] == len(fk)
            mcb, dsc, unc = result["domain_mcb"][s], result["domain_dsc"][s], result["domain_unc"][s]
            assert abs(brier / n - (mcb - dsc + unc)) <= 1e-15 and mcb >= -1e-15 and dsc >= -1e-15
            assert z["mcb"][i] == mcb and z["brier"][i] == brier / n
        info = model.dataset.dataset_info
        total = sum(info[d]["n_test"] for d in domains)
        assert abs(result["avg_mcb"] - z["mcb"].mean()) <= 1e-15
        assert abs(result["weighted_mcb"] - sum(info[d]["n_test"] * z["mcb"][i] for i, d in enumerate(domains)) / total) <= 1e-15
    assert np.array_equal(eng.weights.numpy(), live)
    text = capsys.readouterr().out
    assert "Isotonic recalibration" in text and text.count(" MCB ") == len(domains) and "isotonic.npz" in text
    # without the key: no new key in result.json, no file
    cfg2 = gh.tiny_config(tmp_path / "plain", "mlp_meta_mamdr")
    built2 = []
    cli.main(cfg2, FakeEngine, on_model=built2.append)
    rdir2 = os.path.join(built2[0].result_path, os.listdir(built2[0].result_path)[0])
    with open(os.path.join(rdir2, "result.json")) as f:
        assert sorted(json.load(f)) == ["avg_auc", "avg_loss", "domain_auc", "domain_loss"]
    assert not os.path.exists(os.path.join(built2[0].result_path, "isotonic.npz"))


def test_report_writes_where_it_is_told_and_checks_the_bins(tmp_path):
    class Model(object):
        result_path = str(tmp_path / "result")

        class dataset(object):
            test_dataset = {3: None}

        def isotonic_eval(self, d, n_bins):
            p, y = cases()["q64"]
            t = isotonic.table(*isotonic.fit_host(p, y))
            rep = exact.report_host(p, y, n_bins)
            return isotonic.finish(t, t, isotonic.score_sums_host(p, y), isotonic.score_sums_host(p, y), rep, rep)
    out = str(tmp_path / "elsewhere" / "i.npz")
    path, reports = isotonic.report(Model(), 4, out)
    assert path == out and os.path.exists(out) and reports[3]["n_blocks"] == reports[3]["n_blocks_test"]
    s = isotonic.summarise(reports)
    assert s["mcb"] == (reports[3]["mcb"], reports[3]["mcb"]) and set(s) == set(isotonic.SUMMARY_KEYS)
    assert isotonic.summarise({}) == {k: (0.0, 0.0) for k in isotonic.SUMMARY_KEYS}
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            isotonic.report(Model(), bad, out)


def test_the_module_is_not_imported_without_the_flag():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import mamdr_amd.cli, mamdr_amd.engine, mamdr_amd.model_zoo; "
            "assert 'mamdr_amd.isotonic' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ------------------------------------------------------------------ C ABI
DECLARED = {
    "mamdr_isotonic_fit": ["const float* d_pred", "const float* d_label", "int64_t n", "int64_t* d_counts", "uint32_t* d_first_key",
                           "int64_t* d_rows", "int64_t* d_positives", "void* stream"],
    "mamdr_isotonic_fit_bounded": ["const float* d_pred", "const float* d_label", "int64_t n", "int64_t* d_counts",
                                   "uint32_t* d_first_key", "int64_t* d_rows", "int64_t* d_positives", "int32_t tile_points",
                                   "void* stream"],
    "mamdr_isotonic_apply": ["const uint32_t* d_first_key", "const int64_t* d_rows", "const int64_t* d_positives",
                             "int64_t n_blocks", "const float* d_pred", "int64_t n", "float* d_out", "void* stream"],
    "mamdr_score_sums": ["const float* d_pred", "const float* d_label", "int64_t n", "double* d_out", "void* stream"],
}


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    ctype = lambda p: vp if "*" in p else {"int64_t": i64, "int32_t": i32}[p.split()[0]]      # noqa: E731
    lib = _lib.load()
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, bare)
        assert m, "%s is not declared in include/mamdr_hip.h" % name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
        assert _lib.SIGNATURES[name] == (C.c_int, [ctype(p) for p in params])
        assert hasattr(lib, name)
    assert header.index("int mamdr_auc_bootstrap_bounded") < header.index("int mamdr_isotonic_fit(") < header.index("int mamdr_gram(")
    doc = header[:header.index("int mamdr_isotonic_fit(")].rsplit("/*", 1)[1]
    for word in ("NO REFERENCE COUNTERPART", "STRICT", "<= 0 in int64", "mean_left >= mean_right", "1e-7", "Added within ABI 19",
                 "about 33 bytes per row", "one lane"):
        assert word in doc, word
    assert isotonic.MIN_TILE == int(re.search(r"#define\s+MAMDR_ISOTONIC_MIN_TILE\s+(\d+)", header).group(1))
    kernels = open(os.path.join(ROOT, "mamdr_amd", "csrc", "mamdr_kernels.h")).read()
    for c_name, value in (("ISO_POINT_TILE", isotonic.POINT_TILE), ("ISO_SCAN_TILE", isotonic.SCAN_TILE),
                          ("ISO_HULL_TILE", isotonic.HULL_TILE), ("ISO_MIN_TILE", isotonic.MIN_TILE),
                          ("ISO_MAX_LEVELS", isotonic.MAX_LEVELS), ("ISO_APPLY_TILE", isotonic.APPLY_TILE),
                          ("ISO_APPLY_LDS", isotonic.APPLY_LDS), ("ISO_SCORE_TILE", isotonic.SCORE_TILE)):
        assert int(re.search(r"constexpr int %s = (\d+);" % c_name, kernels).group(1)) == value, c_name
    assert _lib.ABI_VERSION == 19
    from mamdr_amd import build
    assert "isotonic_kernels.hip" in [s for s, _ in build.SOURCES]


def test_refusals_need_no_device():
    """every MAMDR_EINVAL comes before any HIP call: a host address stands in for the device pointers -- nothing is
    launched, nothing dereferenced."""
    lib = _lib.load()
    f, odd, s = C.c_void_p(4096), C.c_void_p(4098), None
    fit, bounded, apply, sums = lib.mamdr_isotonic_fit, lib.mamdr_isotonic_fit_bounded, lib.mamdr_isotonic_apply, lib.mamdr_score_sums
    for what, code in {"n < 0": fit(f, f, -1, f, f, f, f, s), "n = 2^31": fit(f, f, 2 ** 31, f, f, f, f, s),
                       "null counts": fit(f, f, 8, None, f, f, f, s), "null pred": fit(None, f, 8, f, f, f, f, s),
                       "null label": fit(f, None, 8, f, f, f, f, s), "null first_key": fit(f, f, 8, f, None, f, f, s),
                       "null rows": fit(f, f, 8, f, f, None, f, s), "null positives": fit(f, f, 8, f, f, f, None, s),
                       "misaligned pred": fit(odd, f, 8, f, f, f, f, s), "misaligned counts": fit(f, f, 8, C.c_void_p(4100), f, f, f, s),
                       "misaligned rows": fit(f, f, 8, f, f, C.c_void_p(4100), f, s),
                       "tile 3": bounded(f, f, 8, f, f, f, f, isotonic.MIN_TILE - 1, s), "tile 0": bounded(f, f, 8, f, f, f, f, 0, s),
                       "tile < 0": bounded(f, f, 8, f, f, f, f, -64, s), "tile 3, n = 0": bounded(f, f, 0, f, f, f, f, 3, s)}.items():
        assert code == _lib.EINVAL and b"mamdr_isotonic_fit" in lib.mamdr_last_error(), what
    for what, code in {"no blocks": apply(f, f, f, 0, f, 8, f, s), "blocks < 0": apply(f, f, f, -1, f, 8, f, s),
                       "blocks < 0, n = 0": apply(f, f, f, -1, f, 0, f, s), "n < 0": apply(f, f, f, 3, f, -1, f, s),
                       "n = 2^31": apply(f, f, f, 3, f, 2 ** 31, f, s), "null first_key": apply(None, f, f, 3, f, 8, f, s),
                       "null rows": apply(f, None, f, 3, f, 8, f, s), "null positives": apply(f, f, None, 3, f, 8, f, s),
                       "null pred": apply(f, f, f, 3, None, 8, f, s), "null out": apply(f, f, f, 3, f, 8, None, s),
                       "misaligned out": apply(f, f, f, 3, f, 8, odd, s), "misaligned rows": apply(f, C.c_void_p(4100), f, 3, f, 8, f, s)}.items():
        assert code == _lib.EINVAL and b"mamdr_isotonic_apply" in lib.mamdr_last_error(), what
    for what, code in {"n < 0": sums(f, f, -1, f, s), "n = 2^31": sums(f, f, 2 ** 31, f, s), "null out": sums(f, f, 8, None, s),
                       "null pred": sums(None, f, 8, f, s), "null label": sums(f, None, 8, f, s),
                       "misaligned out": sums(f, f, 8, C.c_void_p(4100), s), "misaligned label": sums(f, odd, 8, f, s)}.items():
        assert code == _lib.EINVAL and b"mamdr_score_sums" in lib.mamdr_last_error(), what
    assert apply(None, None, None, 0, None, 0, None, s) == _lib.OK          # n = 0: nothing to do, no device call
