"""Bootstrap intervals of the exact AUC, host side (no GPU): the threshold table against `decimal` and the header, the hash
against oracle/rng.py, `bootstrap.replicates_host` against exact.metrics_host and a double loop over pairs, `finish` /
`paired`, the C ABI's declaration, binding and device-free refusals, the command line, and `run.py --auc-ci` end to end over
a CPU stand-in of the engine whose `evaluate` honours `want_ci` through `replicates_host`."""
import ctypes as C
import decimal
import os
import re

import numpy as np
import pytest

from fake_engine import ReportingFakeEngine
from mamdr_amd import _lib, bootstrap, cli, exact, gauc
from oracle import rng as orng
from test_gauc_host import patch_emb_dim, result_json, tiny_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
NAN = float("nan")


def header_text():
    return open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()


# ------------------------------------------------------------------ the table and the hash
def test_thresholds_recomputed_and_in_the_header():
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        e1, fact, cdf, want = decimal.Decimal(-1).exp(), 1, decimal.Decimal(0), []
        pmf = []
        for k in range(40):
            fact *= max(k, 1)
            pmf.append(e1 / fact)
            cdf += pmf[-1]
            want.append(int(cdf * 2 ** 32))               # (positive: int() is the floor)
            if want[-1] >= 2 ** 32 - 1:
                break
        assert want[-1] == 2 ** 32 - 1 and want[-2] < 2 ** 32 - 1
        assert tuple(want) == bootstrap.THR == bootstrap.thresholds() == bootstrap.thresholds(50)
        assert bootstrap.WMAX == len(want) == 13
        # the table's steps are the probabilities to 32 bits: P(w = k) = (THR[k] - THR[k - 1]) / 2^32, each floor loses < 1
        steps = np.diff(np.concatenate([[0], want]))
        for k, step in enumerate(steps.tolist()):
            assert abs(step - pmf[k] * 2 ** 32) < 1, k
        assert steps.sum() == 2 ** 32 - 1                  # the one draw 0xffffffff is all that reaches WMAX
    header = header_text()
    m = re.search(r"#define\s+MAMDR_BOOT_THR\s+\{([^}]*)\}", header)
    assert m, "MAMDR_BOOT_THR is not defined in include/mamdr_hip.h"
    literals = [int(x) for x in re.findall(r"(\d+)u", m.group(1).replace("\\", " "))]
    assert tuple(literals) == bootstrap.THR
    assert re.search(r"#define\s+MAMDR_BOOT_WMAX\s+%d\b" % bootstrap.WMAX, header)
    assert bootstrap.poisson1(np.array([0, want[0] - 1, want[0], want[1], 2 ** 32 - 2, 2 ** 32 - 1], np.uint32)).tolist() \
        == [0, 0, 1, 2, 12, 13]


def test_mix64_is_splitmix64s_finaliser():
    for state in (0, 1, 1024, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1):
        advanced, out = orng.splitmix64(state)
        assert bootstrap.mix64(advanced) == out
        assert int(bootstrap.mix64(np.array([advanced], np.uint64))[0]) == out
    assert bootstrap.GOLDEN == (orng.splitmix64(0)[0])
    # u32: the two-level hash, by hand
    seed, b, x = 77, 5, 123456
    hb = bootstrap.mix64((seed + bootstrap.GOLDEN * b) % 2 ** 64)
    assert int(bootstrap.u32(seed, b, np.array([x]))[0]) == bootstrap.mix64(hb ^ x) >> 32
    # a negative unit goes through the (uint32) cast
    assert bootstrap.units_of(np.array([-1, 5], np.int32), 2).tolist() == [2 ** 32 - 1, 5]
    assert int(bootstrap.u32(seed, b, bootstrap.units_of(np.array([-1]), 1))[0]) == bootstrap.mix64(hb ^ (2 ** 32 - 1)) >> 32


def test_weights_look_like_poisson_1():
    """a crude sanity check: over 10^6 (b, unit) pairs the mean lies within 5e-3 of 1 (5 standard errors of 1e-3) and the
    variance within 1e-2 of 1 (the variance's standard error is sqrt(3 / 10^6) = 1.7e-3)."""
    units = np.arange(10000, dtype=np.uint32) * np.uint32(7919)
    w = np.concatenate([bootstrap.weights(3, b, units) for b in range(1, 101)])
    assert w.shape == (10 ** 6,) and w.min() == 0 and w.max() <= bootstrap.WMAX
    print("mean %.6f variance %.6f max %d" % (w.mean(), w.var(), w.max()))
    assert abs(w.mean() - 1.0) <= 5e-3 and abs(w.var() - 1.0) <= 1e-2
    assert np.array_equal(bootstrap.weights(3, 0, units), np.ones(10000, np.int64))
    # one weight per unit and replicate: equal units, equal weights; another replicate or seed, other weights
    assert np.array_equal(bootstrap.weights(3, 4, units[[5, 5, 9, 5]])[[0, 1, 3]], np.repeat(bootstrap.weights(3, 4, units[5:6]), 3))
    assert not np.array_equal(bootstrap.weights(3, 4, units), bootstrap.weights(3, 5, units))
    assert not np.array_equal(bootstrap.weights(3, 4, units), bootstrap.weights(4, 4, units))


# ------------------------------------------------------------------ the host definition
def draws(n, seed, levels=None, rate=0.3):
    rs = np.random.RandomState(seed)
    pred = rs.random_sample(n).astype(F32)
    if levels:
        pred = (np.floor(pred * levels) / levels).astype(F32)
    label = (rs.random_sample(n) < rate * (0.5 + pred)).astype(F32)
    return pred, label, rs.randint(0, max(n // 4, 1), n).astype(np.int32)


def pair_loop(pred, label, w):
    """2 * #{s_p > s_n} + #{s_p == s_n} with every pair counted w_p * w_n times, as a double loop in python integers."""
    key = gauc.ordered_key(pred).tolist()
    pos = [i for i in range(len(key)) if label[i] != 0]
    neg = [i for i in range(len(key)) if label[i] == 0]
    t = 0
    for p in pos:
        for q in neg:
            t += int(w[p]) * int(w[q]) * (2 if key[p] > key[q] else (1 if key[p] == key[q] else 0))
    return t, sum(int(w[p]) for p in pos), sum(int(w[q]) for q in neg)


@pytest.mark.parametrize("levels", [None, 3])
@pytest.mark.parametrize("with_unit", [False, True])
def test_replicates_host_against_a_double_loop(levels, with_unit):
    pred, label, uid = draws(200, 21, levels)
    pred[::37] = NAN
    unit = uid if with_unit else None
    T, P, N = bootstrap.replicates_host(pred, label, 5, seed=9, unit=unit)
    assert T.dtype == np.uint64 and P.dtype == np.int64 and N.dtype == np.int64 and T.shape == P.shape == N.shape == (6,)
    units = bootstrap.units_of(unit, 200)
    for b in range(6):
        assert (int(T[b]), int(P[b]), int(N[b])) == pair_loop(pred, label, bootstrap.weights(9, b, units)), b
    assert len(set(T.tolist())) > 1


@pytest.mark.parametrize("levels", [None, 8])
def test_slot_0_is_metrics_hosts(levels):
    pred, label, uid = draws(5000, 3, levels)
    pred[::97] = NAN
    pred[5::89] = -0.0
    pred[7::113] = np.inf
    pred[11::127] = -np.inf
    counts = exact.metrics_host(pred, label, 5)[0]
    for unit in (None, uid):
        T, P, N = bootstrap.replicates_host(pred, label, 2, seed=1, unit=unit)
        assert [int(T[0]), int(P[0]), int(N[0])] == counts[:3].tolist()
    rep = bootstrap.finish(T, P, N)
    assert rep["auc"] == exact.finish(*exact.metrics_host(pred, label, 5))["auc"] and rep["valid"] == 1


def test_special_values_follow_the_keys_rules():
    # sorted: nan- nan+ -inf- -3- 0- 0+ 2.5+ (exact's hand-computed case); NaN == NaN and -0 == +0 tie, NaN < -inf
    pred = np.array([NAN, -np.inf, NAN, -0.0, 0.0, 2.5, -3.0], F32)
    label = np.array([2.0, 0, 0, -1.0, 0, 1, 0], F32)
    T, P, N = bootstrap.replicates_host(pred, label, 40, seed=5)
    assert (int(T[0]), int(P[0]), int(N[0])) == (16, 3, 4)
    for b in range(41):
        assert (int(T[b]), int(P[b]), int(N[b])) == pair_loop(pred, label, bootstrap.weights(5, b, np.arange(7, dtype=np.uint32)))
    # all-equal predictions: every pair ties, AUC_b is exactly 1/2 for every valid b
    label = (np.arange(300) % 3 == 0).astype(F32)
    T, P, N = bootstrap.replicates_host(np.full(300, 0.25, F32), label, 30, seed=2)
    assert np.array_equal(T.astype(np.int64), P * N)
    assert bootstrap.finish(T, P, N)["replicates"].tolist() == [0.5] * 31
    # an empty split, one class only
    T, P, N = bootstrap.replicates_host([], [], 3, seed=0)
    assert T.tolist() == P.tolist() == N.tolist() == [0] * 4
    T, P, N = bootstrap.replicates_host([.1, .2, .3], [1, 1, 1], 6, seed=0)
    assert not T.any() and not N.any() and P[0] == 3
    rep = bootstrap.finish(T, P, N)
    assert (rep["auc"], rep["valid"], rep["n_valid"], rep["se"], rep["ci_lo"], rep["ci_hi"]) == (0.0, 0, 0, 0.0, 0.0, 0.0)
    assert np.isnan(rep["replicates"]).all()
    for bad in (dict(n_rep=-1), dict(n_rep=65536)):
        with pytest.raises(ValueError):
            bootstrap.replicates_host([.1], [1], seed=0, **bad)
    with pytest.raises(ValueError):
        bootstrap.replicates_host([.1], [1, 0], 2, seed=0)
    with pytest.raises(ValueError):
        bootstrap.replicates_host([.1, .2], [1, 0], 2, seed=0, unit=[1])


def test_a_row_permutation():
    """with a unit column the replicates are a function of the (value, unit) multiset; without, slot 0 alone is."""
    pred, label, uid = draws(3000, 8, levels=16)
    p = np.random.RandomState(1).permutation(3000)
    a = bootstrap.replicates_host(pred, label, 8, seed=4, unit=uid)
    b = bootstrap.replicates_host(pred[p], label[p], 8, seed=4, unit=uid[p])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a = bootstrap.replicates_host(pred, label, 8, seed=4)
    b = bootstrap.replicates_host(pred[p], label[p], 8, seed=4)
    assert all(x[0] == y[0] for x, y in zip(a, b)) and not np.array_equal(a[0][1:], b[0][1:])


# ------------------------------------------------------------------ finish / paired
def test_finish_and_paired_by_hand():
    # slots: the estimate 3/4; replicates 1/2, 1 (= 8 / (2 * 2 * 2)), invalid (N = 0), 1/4, invalid (P = 0), 3/4
    T = np.array([6, 4, 8, 0, 2, 0, 6], np.uint64)
    P = np.array([2, 2, 2, 3, 2, 0, 2], np.int64)
    N = np.array([2, 2, 2, 0, 2, 3, 2], np.int64)
    rep = bootstrap.finish(T, P, N, level=0.5)
    assert rep["auc"] == 0.75 and rep["valid"] == 1 and rep["n_rep"] == 6 and rep["n_valid"] == 4 and rep["level"] == 0.5
    assert np.array_equal(np.isnan(rep["replicates"]), [False, False, False, True, False, True, False])
    drawn = [0.5, 1.0, 0.25, 0.75]
    assert rep["replicates"][[1, 2, 4, 6]].tolist() == drawn
    assert rep["se"] == float(np.std(drawn, ddof=1))
    # percentiles 25 and 75 of (.25 .5 .75 1.) by linear interpolation: positions 0.75 and 2.25 -> .4375 and .8125
    assert (rep["ci_lo"], rep["ci_hi"]) == (0.4375, 0.8125)
    assert rep["T"].dtype == np.uint64 and rep["P"].tolist() == P.tolist() and rep["N"].tolist() == N.tolist()
    wide = bootstrap.finish(T, P, N)
    # percentiles 2.5 and 97.5: positions 0.075 and 2.925 -> .26875 and .98125 (the level's own rounding moves them by 1e-16)
    assert wide["level"] == 0.95 and abs(wide["ci_lo"] - 0.26875) < 1e-12 and abs(wide["ci_hi"] - 0.98125) < 1e-12
    assert wide["ci_lo"] <= rep["ci_lo"] and rep["ci_hi"] <= wide["ci_hi"]
    # fewer than two valid replicates: zeros, n_valid tells why; an invalid estimate: 0.0 with valid = 0
    one = bootstrap.finish(T[[0, 1, 3]], P[[0, 1, 3]], N[[0, 1, 3]])
    assert (one["n_rep"], one["n_valid"], one["se"], one["ci_lo"], one["ci_hi"], one["auc"]) == (2, 1, 0.0, 0.0, 0.0, 0.75)
    none = bootstrap.finish(T[[3]], P[[3]], N[[3]])
    assert (none["n_rep"], none["n_valid"], none["auc"], none["valid"]) == (0, 0, 0.0, 0)
    with pytest.raises(ValueError):
        bootstrap.finish(T, P[:3], N)
    with pytest.raises(ValueError):
        bootstrap.finish(T, P, N, level=1.0)
    # paired: differences over the replicates valid in both
    other = bootstrap.finish(np.array([4, 4, 0, 2, 8, 0, 2], np.uint64), np.array([2, 2, 0, 2, 2, 0, 2], np.int64),
                             np.array([2, 2, 2, 2, 2, 3, 2], np.int64))
    cmp = bootstrap.paired(rep, other, level=0.5)
    assert cmp["diff"] == 0.25 and cmp["valid"] == 1 and cmp["n_rep"] == 6 and cmp["n_valid"] == 3
    assert np.array_equal(np.isnan(cmp["replicates"]), [False, False, True, True, False, True, False])
    diffs = [0.0, -0.75, 0.5]
    assert cmp["replicates"][[1, 4, 6]].tolist() == diffs and cmp["se"] == float(np.std(diffs, ddof=1))
    assert (cmp["ci_lo"], cmp["ci_hi"]) == tuple(np.percentile(diffs, [25, 75]).tolist())
    same = bootstrap.paired(rep["replicates"], rep["replicates"])
    assert same["diff"] == 0.0 and same["se"] == 0.0 and same["n_valid"] == 4 and (same["ci_lo"], same["ci_hi"]) == (0.0, 0.0)
    with pytest.raises(ValueError):
        bootstrap.paired(rep, one)
    assert bootstrap.summarise({0: rep, 3: one}) == {
        "domain_auc_ci_lo": {0: 0.4375, 3: 0.0}, "domain_auc_ci_hi": {0: 0.8125, 3: 0.0},
        "domain_auc_se": {0: rep["se"], 3: 0.0}, "domain_auc_ci_valid": {0: 4, 3: 1}}


def test_two_models_on_one_split_are_paired():
    """one label / unit / seed, two prediction vectors: every row has the same weights, so P and N are identical arrays, and
    the difference's interval is far narrower than either AUC's."""
    pred, label, uid = draws(4000, 13)
    rs = np.random.RandomState(0)
    worse = (pred + 0.05 * rs.standard_normal(4000)).astype(F32)
    a = bootstrap.finish(*bootstrap.replicates_host(pred, label, 200, seed=6, unit=uid))
    b = bootstrap.finish(*bootstrap.replicates_host(worse, label, 200, seed=6, unit=uid))
    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["N"], b["N"]) and not np.array_equal(a["T"], b["T"])
    cmp = bootstrap.paired(a, b)
    print("AUC %.4f +- %.4f against %.4f +- %.4f: difference %.4f +- %.4f [%.4f, %.4f]"
          % (a["auc"], a["se"], b["auc"], b["se"], cmp["diff"], cmp["se"], cmp["ci_lo"], cmp["ci_hi"]))
    assert cmp["n_valid"] == 200 and cmp["diff"] == a["auc"] - b["auc"] and 0 < cmp["se"] < a["se"]
    assert a["ci_lo"] < a["auc"] < a["ci_hi"]            # (no law, but at 4,000 rows and 200 replicates anything else is a bug)
    other_seed = bootstrap.replicates_host(pred, label, 200, seed=7, unit=uid)
    assert not np.array_equal(other_seed[1], a["P"]) and other_seed[1][0] == a["P"][0]


# ------------------------------------------------------------------ C ABI
PARAMS = ["const float* d_pred", "const float* d_label", "const int32_t* d_unit", "int64_t n", "int32_t n_rep",
          "uint64_t seed", "uint64_t* d_T", "int64_t* d_P", "int64_t* d_N"]


def test_auc_bootstrap_is_declared_and_bound():
    header = header_text()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, extra in (("mamdr_auc_bootstrap", []), ("mamdr_auc_bootstrap_bounded", ["int64_t part_words"])):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, bare)
        assert m, "%s is not declared in include/mamdr_hip.h" % name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == PARAMS + extra + ["void* stream"]
    assert header.index("int mamdr_exact_metrics") < header.index("int mamdr_auc_bootstrap(") < header.index("int mamdr_gram(")
    doc = header[:header.index("int mamdr_auc_bootstrap(")].rsplit("/*", 1)[1]
    flat = lambda s: " ".join(s.replace(" * ", " ").replace("`", "").split())      # noqa: E731 (the comment's line starts)
    assert "NO REFERENCE COUNTERPART" in doc and "Added within ABI 19" in doc
    for phrase in ("NaN is lowest and equals NaN, -0 equals +0", "w(b, i) = poisson1(u32(b, unit(i)))",
                   "Replicate 0 is the unweighted statistic: w(0, .) = 1", "0 <= n < 2^27", "0 <= n_rep <= 65,535",
                   "n = 0 writes zeros", "hipMallocAsync / hipFreeAsync", "reported, not hidden",
                   "no floating-point arithmetic on the device at all", "not on grid, tiling or chunking"):
        assert phrase in flat(doc), phrase
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    assert _lib.SIGNATURES["mamdr_auc_bootstrap"] == (C.c_int, [vp, vp, vp, i64, i32, u64, vp, vp, vp, vp])
    assert _lib.SIGNATURES["mamdr_auc_bootstrap_bounded"] == (C.c_int, [vp, vp, vp, i64, i32, u64, vp, vp, vp, i64, vp])
    assert _lib.ABI_VERSION == 19 and re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    assert _lib.load().mamdr_abi_version() == 19


def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "mamdr_amd", "csrc", "mamdr_kernels.h")).read()
    for name in ("TILE", "GROUP"):
        m = re.search(r"constexpr int BOOT_%s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(bootstrap, name), name
    m = re.search(r"constexpr int64_t BOOT_PART_WORDS = 1 << (\d+);", text)
    assert m and 1 << int(m.group(1)) == bootstrap.PART_WORDS
    from mamdr_amd import build
    assert "bootstrap_kernels.hip" in dict(build.SOURCES)


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    x = C.c_void_p(64)            # never dereferenced: every case below is refused before any device call

    def call(pred=x, label=x, unit=None, n=8, n_rep=3, T=x, P=x, N=x, words=None):
        if words is None:
            return lib.mamdr_auc_bootstrap(pred, label, unit, n, n_rep, 0, T, P, N, None)
        return lib.mamdr_auc_bootstrap_bounded(pred, label, unit, n, n_rep, 0, T, P, N, words, None)
    cases = {"null T": dict(T=None), "null P": dict(P=None), "null N": dict(N=None), "null pred": dict(pred=None),
             "null label": dict(label=None), "n < 0": dict(n=-1), "n = 2^27": dict(n=2 ** 27), "n_rep < 0": dict(n_rep=-1),
             "n_rep = 65,536": dict(n_rep=65536), "misaligned pred": dict(pred=C.c_void_p(66)),
             "misaligned label": dict(label=C.c_void_p(65)), "misaligned unit": dict(unit=C.c_void_p(66)),
             "misaligned T": dict(T=C.c_void_p(68)), "misaligned P": dict(P=C.c_void_p(68)),
             "misaligned N": dict(N=C.c_void_p(68)), "no workspace": dict(words=0), "null T, bounded": dict(T=None, words=64)}
    for what, kw in cases.items():
        assert call(**kw) == _lib.EINVAL, what
        assert b"mamdr_auc_bootstrap" in lib.mamdr_last_error(), what
    with pytest.raises(_lib.MamdrError, match="n_rep 65536 outside 0..65535"):
        _lib.check(call(n_rep=65536))


# ------------------------------------------------------------------ run.py --auc-ci over a CPU stand-in
OLD_KEYS = {"avg_loss", "avg_auc", "domain_loss", "domain_auc"}
CI_KEYS = {"domain_auc_ci_lo", "domain_auc_ci_hi", "domain_auc_se", "domain_auc_ci_valid"}
EXACT_KEYS = {"domain_auc_exact", "avg_auc_exact", "weighted_auc_exact", "domain_ap", "domain_ece", "domain_pcoc"}
GAUC_KEYS = {"avg_gauc", "weighted_gauc", "domain_gauc", "domain_gauc_users"}


def run_folder(tmp_path, cfg):
    rdir = os.path.join(str(tmp_path / "result"), cfg["model"]["name"], "Taobao", cfg["dataset"]["domain_split_path"])
    runs = os.listdir(rdir)
    assert len(runs) == 1
    return os.path.join(rdir, runs[0])


@pytest.mark.parametrize("name,others,unit", [("mlp", False, "row"), ("mlp_meta_mamdr", True, None)])
def test_run_auc_ci_on_a_cpu_stand_in(tmp_path, monkeypatch, capsys, name, others, unit):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    extra = dict(report_gauc=True, report_exact=7) if others else {}
    if unit:
        extra.update(auc_ci_unit=unit, auc_ci_seed=11)
    cfg = tiny_config(tmp_path, name, epochs=2, report_auc_ci=40, **extra)
    built = []
    res = cli.main(cfg, ReportingFakeEngine, on_model=built.append)
    assert len(res) == 4 and set(res[3]) == {0, 1, 2}                  # still (loss, auc) per domain
    want_kw = dict(want_ci=(40, 11, "row") if unit else (40, 0, "user"), **({"want_gauc": True, "want_exact": 7} if others else {}))
    assert ReportingFakeEngine.seen and all(kw == want_kw for kw in ReportingFakeEngine.seen)
    result = result_json(tmp_path, cfg)
    assert set(result) == OLD_KEYS | CI_KEYS | ((GAUC_KEYS | EXACT_KEYS) if others else set())
    last = {d: rep for d, split, name, _, rep in ReportingFakeEngine.log if split == "test" and name == "ci"}          # the LAST test evaluation of every domain
    for d in range(3):
        rep = last[d]
        assert built[0].ci_reports[("test", d)] is rep
        assert result["domain_auc_ci_lo"][str(d)] == rep["ci_lo"] and result["domain_auc_ci_hi"][str(d)] == rep["ci_hi"]
        assert result["domain_auc_se"][str(d)] == rep["se"] and result["domain_auc_ci_valid"][str(d)] == rep["n_valid"]
        assert 0.0 <= rep["ci_lo"] <= rep["ci_hi"] <= 1.0 and rep["se"] > 0 and rep["n_valid"] >= 38
        if others:
            assert result["domain_auc_exact"][str(d)] == rep["auc"]
            assert isinstance(built[0].exact_reports[("test", d)], dict) and "gauc" in built[0].gauc_reports[("test", d)]
    folder = run_folder(tmp_path, cfg)
    assert "auc_bootstrap.npz" in os.listdir(folder)
    with np.load(os.path.join(folder, "auc_bootstrap.npz")) as z:
        assert sorted(z.files) == sorted(["n_rep", "seed", "unit"] + ["%s_%d" % (k, d) for k in ("replicates", "T", "P", "N")
                                                                      for d in range(3)])
        assert int(z["n_rep"]) == 40 and int(z["seed"]) == (11 if unit else 0) and str(z["unit"]) == (unit or "user")
        for d in range(3):
            assert z["replicates_%d" % d].shape == (41,) and z["T_%d" % d].dtype == np.uint64
            for k in ("T", "P", "N"):
                assert np.array_equal(z["%s_%d" % (k, d)], last[d][k]), (k, d)
            assert np.array_equal(z["replicates_%d" % d], last[d]["replicates"], equal_nan=True)
            assert z["replicates_%d" % d][0] == last[d]["auc"]
            # the arrays are what `paired` takes
            assert bootstrap.paired(z["replicates_%d" % d], z["replicates_%d" % d])["n_valid"] == last[d]["n_valid"]
    text = capsys.readouterr().out
    tail = text[text.rindex("Overall test Loss:"):]
    assert "Exact AUC, 40 bootstrap replicates by %s (seed %d)" % (unit or "user", 11 if unit else 0) in tail
    assert "0: {} [{}, {}] {}, {}".format(last[0]["auc"], last[0]["ci_lo"], last[0]["ci_hi"], last[0]["se"], last[0]["n_valid"]) in tail
    assert text.count("bootstrap replicates by") >= 2                   # the validations report it as well


def test_without_the_flag_nothing_changes(tmp_path, monkeypatch, capsys):
    patch_emb_dim(monkeypatch)
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    cfg = tiny_config(tmp_path, "mlp", epochs=1)
    without = cli.main(cfg, ReportingFakeEngine)
    assert ReportingFakeEngine.seen and all(kw == {} for kw in ReportingFakeEngine.seen)          # evaluate never receives want_ci
    assert set(result_json(tmp_path, cfg)) == OLD_KEYS
    assert "auc_bootstrap.npz" not in os.listdir(run_folder(tmp_path, cfg))
    assert "bootstrap" not in capsys.readouterr().out
    # ... and the flag changes neither the returned tuple nor what was saved before: decisions stay on AUC-500
    cfg2 = tiny_config(tmp_path / "b", "mlp", epochs=1, report_auc_ci=20)
    assert cli.main(cfg2, ReportingFakeEngine) == without
    both = result_json(tmp_path / "b", cfg2)
    assert {k: both[k] for k in OLD_KEYS} == result_json(tmp_path, cfg)
    for bad in (dict(report_auc_ci=65536), dict(report_auc_ci=5, auc_ci_unit="item")):
        with pytest.raises(ValueError, match="auc_ci"):
            cli.main(tiny_config(tmp_path / "c", "mlp", epochs=1, **bad), ReportingFakeEngine)


def test_the_command_line(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--auc-ci"])
    cli.cli(["--config", cfg_path, "--auc-ci", "200", "--auc-ci-unit", "row", "--auc-ci-seed", "9", "--exact-metrics"])
    assert [(len(a), k) for a, k in seen] == [(1, {})] * 3             # main is called as before
    train = [a[0]["train"] for a, _ in seen]
    assert not any(k in train[0] for k in ("report_auc_ci", "auc_ci_unit", "auc_ci_seed"))
    assert (train[1]["report_auc_ci"], train[1]["auc_ci_unit"], train[1]["auc_ci_seed"]) == (1000, "user", 0)
    assert "report_exact" not in train[1]
    assert (train[2]["report_auc_ci"], train[2]["auc_ci_unit"], train[2]["auc_ci_seed"], train[2]["report_exact"]) == (200, "row", 9, 20)
    for bad in (["--auc-ci", "0"], ["--auc-ci", "65536"], ["--auc-ci-unit", "row"], ["--auc-ci-seed", "3"],
                ["--auc-ci", "10", "--auc-ci-unit", "item"]):
        with pytest.raises(SystemExit):
            cli.cli(["--config", cfg_path] + bad)
    assert len(seen) == 3


def test_lanes_refuse_report_auc_ci_by_name(tmp_path, monkeypatch):
    patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr", report_auc_ci=100, lanes=2)
    with pytest.raises(NotImplementedError, match="train.report_auc_ci"):
        cli.main(cfg, ReportingFakeEngine)
    assert not loaded                    # refused before the data is loaded


def test_documents_carry_the_feature():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "--auc-ci" in readme
    for word in ("mamdr_auc_bootstrap", "k_boot_parts", "k_boot_carry", "k_boot_T", "Poisson", "auc_bootstrap.txt"):
        assert word in design, word
