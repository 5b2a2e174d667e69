"""Bootstrap replicates of the exact AUC's integers on the device (mamdr_auc_bootstrap, DeviceEngine.auc_bootstrap /
evaluate(want_ci=...)).

Every comparison is exact integer equality of (T, P, N), all n_rep + 1 slots, with bootstrap.replicates_host (a stable
np.argsort and np.cumsum: another algorithm).  Sizes: around one wave, around the sorted-row tile bootstrap.TILE, several
tiles with a ragged end, n = 0.  Replicate counts: around the replicate group bootstrap.GROUP, and a workspace bound
(mamdr_auc_bootstrap_bounded) small enough to run the replicates in several chunks.  A host reference is computed once per
case and shared.
"""
import ctypes as C
import copy
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import bootstrap, exact      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, GROUP = bootstrap.TILE, bootstrap.GROUP
MID = 3 * TILE + 5
SIZES = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, MID]

_CACHE = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def device_call(pred, label, n_rep, seed, unit=None, part_words=None):
    """the stateless export on torch's current stream -> (T uint64, P int64, N int64) as numpy; every output starts as -1."""
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred = torch.from_numpy(np.array(pred, dtype=F32)).to(dev)
    d_label = torch.from_numpy(np.array(label, dtype=F32)).to(dev)
    d_unit = torch.from_numpy(np.array(unit, dtype=np.int32)).to(dev) if unit is not None else None
    n = int(d_pred.numel())
    T, P, N = [torch.full((n_rep + 1,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
    args = (ptr(d_pred), ptr(d_label), ptr(d_unit), n, n_rep, seed, ptr(T), ptr(P), ptr(N))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if part_words is None:
        L.check(lib.mamdr_auc_bootstrap(*args, stream))
    else:
        L.check(lib.mamdr_auc_bootstrap_bounded(*args, part_words, stream))
    return T.cpu().numpy().view(np.uint64), P.cpu().numpy(), N.cpu().numpy()


def host(name, pred, label, n_rep, seed, unit=None):
    """bootstrap.replicates_host of a named case: computed once, never modified."""
    key = (name, n_rep, seed, unit is not None)
    if key not in _CACHE:
        ref = bootstrap.replicates_host(pred, label, n_rep, seed, unit)
        for a in ref:
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def check(name, pred, label, n_rep, seed, unit=None, **kw):
    """device == host on every word -> the device's outputs."""
    want = host(name, pred, label, n_rep, seed, unit)
    got = device_call(pred, label, n_rep, seed, unit, **kw)
    for what, g, w in zip("TPN", got, want):
        assert g.shape == (n_rep + 1,) and np.array_equal(g, w), (name, what, np.flatnonzero(g != w)[:10], g[:4], w[:4])
    return got


def mixed(n, seed=0):
    """continuous predictions, one row in four quantised to 8 levels (tie runs), CTR-like labels drawn from them, a uid column
    with repeats."""
    key = ("mixed", n, seed)
    if key not in _CACHE:
        rs = np.random.RandomState(2000 + seed)
        pred = rs.random_sample(n).astype(F32)
        coarse = rs.random_sample(n) < 0.25
        pred[coarse] = (np.floor(pred[coarse] * 8) / 8).astype(F32)
        label = (rs.random_sample(n) < 0.05 + 0.3 * pred).astype(F32)
        uid = rs.randint(0, max(n // 5, 1), n).astype(np.int32)
        for a in (pred, label, uid):
            a.setflags(write=False)
        _CACHE[key] = (pred, label, uid)
    return _CACHE[key]


# ------------------------------------------------------------------ sizes and replicate counts
@pytest.mark.parametrize("n", SIZES)
def test_every_size(n):
    need_gpu()
    pred, label, uid = mixed(n)
    T, P, N = check("mixed%d" % n, pred, label, 3, 5)
    assert P[0] + N[0] == n and P[0] == int((label != 0).sum())
    check("mixed%d" % n, pred, label, 3, 5, unit=uid)


@pytest.mark.parametrize("n_rep", [0, 1, 3, GROUP - 1, GROUP, GROUP + 1, 3 * GROUP + 2])
def test_every_replicate_count(n_rep):
    """n_rep + 1 slots: below, at and beyond one workgroup's replicate group."""
    need_gpu()
    pred, label, uid = mixed(MID)
    check("mixed%d" % MID, pred, label, n_rep, 9, unit=uid)


@pytest.mark.parametrize("part_words", [1, 3 * 4 * GROUP, 3 * 4 * 2 * GROUP + 7])
def test_replicates_in_chunks(part_words):
    """MID rows are 4 tiles, 12 words of partials per replicate: bounds of nothing (one group at a time is the least), of
    exactly one group and of two groups and a bit run 70 + 1 slots in 5, 5 and 3 chunks; the words do not depend on it."""
    need_gpu()
    pred, label, uid = mixed(MID)
    bounded = check("mixed%d" % MID, pred, label, 70, 4, unit=uid, part_words=part_words)
    whole = check("mixed%d" % MID, pred, label, 70, 4, unit=uid)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(bounded, whole))


# ------------------------------------------------------------------ data
def data_case(name):
    rs = np.random.RandomState(17)
    n = MID
    label = (rs.random_sample(n) < 0.3).astype(F32)
    distinct = (0.25 + 0.5 * rs.permutation(n) / F32(n)).astype(F32)            # n different values in [0.25, 0.75)
    if name == "continuous":
        return distinct, label
    if name == "3 values":                                 # runs of about a tile: each crosses tile borders
        return (rs.randint(0, 3, n) / F32(4)).astype(F32), label
    if name == "all equal":                                # one run over every tile: the carried run start
        return np.full(n, 0.3, F32), label
    if name == "run ends on a tile border":                # the lowest TILE rows tie, the others are distinct
        pred = distinct.copy()
        pred[rs.permutation(n)[:TILE]] = 0.125
        return pred, label
    if name == "run from mid tile to a border":            # 500 distinct rows, a run up to position 2 * TILE, distinct rows
        pred = distinct.copy()
        rows = rs.permutation(n)
        pred[rows[:500]] = (0.01 + 0.1 * np.arange(500) / F32(500)).astype(F32)
        pred[rows[500:2 * TILE]] = 0.2
        return pred, label
    if name == "specials":
        tiny = np.float32(1e-45)
        pool = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1e-39, -1e-39, -2.5, -0.25, 1.0, 1.5, 7e37,
                         0.25, 0.75, np.nextafter(F32(0.75), F32(1))], F32)
        return rs.choice(pool, n), label
    if name == "all positive":
        return distinct, np.ones(n, F32)
    if name == "all negative":
        return distinct, np.zeros(n, F32)
    if name == "one positive":
        label = np.zeros(n, F32)
        label[n // 3] = 2.0
        return distinct, label
    raise KeyError(name)


DATA = ["continuous", "3 values", "all equal", "run ends on a tile border", "run from mid tile to a border", "specials",
        "all positive", "all negative", "one positive"]


@pytest.mark.parametrize("name", DATA)
def test_every_kind_of_data(name):
    need_gpu()
    pred, label = data_case(name)
    uid = mixed(MID)[2]
    n_rep = 60 if name == "one positive" else 5
    T, P, N = check(name, pred, label, n_rep, 3)
    check(name, pred, label, n_rep, 3, unit=uid)
    rep = bootstrap.finish(T, P, N)
    if name == "all equal":
        assert np.array_equal(T.astype(np.int64), P * N)                        # every pair ties: AUC_b exactly 1/2
        assert rep["replicates"].tolist() == [0.5] * (n_rep + 1)
    if name == "all positive":
        assert not T.any() and not N.any() and P[0] == MID and rep["n_valid"] == 0 and rep["valid"] == 0
    if name == "all negative":
        assert not T.any() and not P.any() and N[0] == MID and rep["n_valid"] == 0
    if name == "one positive":
        # the positive's weight is 0 in about e^-1 of the replicates: they are flagged, not dropped
        invalid = np.flatnonzero(P[1:] == 0)
        assert 5 <= invalid.size <= 40 and rep["n_rep"] == 60 and rep["n_valid"] == 60 - invalid.size
        assert np.isnan(rep["replicates"][1:][invalid]).all() and not T[1:][invalid].any()
        assert rep["valid"] == 1 and P[0] == 1
    if name == "specials":
        assert exact.metrics_host(pred, label, 4)[0][:3].tolist() == [int(T[0]), int(P[0]), int(N[0])]


def test_units():
    """every row of a unit gets one weight: P_b + N_b is the units' weights times their row counts; negative ids go through
    the (uint32) cast."""
    need_gpu()
    pred, label, _ = mixed(MID)
    rs = np.random.RandomState(3)
    uid = rs.randint(0, 20, MID).astype(np.int32)
    T, P, N = check("heavy repeats", pred, label, 6, 8, unit=uid)
    rows = np.bincount(uid, minlength=20)
    for b in range(7):
        assert P[b] + N[b] == int((bootstrap.weights(8, b, np.arange(20, dtype=np.uint32)) * rows).sum()), b
    negative = (uid - 10).astype(np.int32)
    assert negative.min() < 0
    shifted = check("negative ids", pred, label, 6, 8, unit=negative)
    assert not np.array_equal(shifted[1][1:], P[1:]) and shifted[1][0] == P[0]


def test_same_bytes_other_seeds_and_pairing():
    need_gpu()
    pred, label, uid = mixed(MID, seed=1)
    first = check("det", pred, label, 20, 12, unit=uid)
    again = device_call(pred, label, 20, 12, unit=uid)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    other = device_call(pred, label, 20, 13, unit=uid)
    assert all(a[0] == b[0] for a, b in zip(first, other))                      # slot 0 knows no seed
    assert not np.array_equal(first[0][1:], other[0][1:]) and not np.array_equal(first[1][1:], other[1][1:])
    # a seed beyond 2^63 passes as the 64-bit word it is
    check("det", pred, label, 4, 2 ** 64 - 3, unit=uid)
    # pairing: another prediction vector, the same labels / units / seed -> the same weights: identical P and N
    worse = (pred + 0.1 * np.random.RandomState(0).standard_normal(MID)).astype(F32)
    paired = check("det worse", worse, label, 20, 12, unit=uid)
    assert paired[1].tobytes() == first[1].tobytes() and paired[2].tobytes() == first[2].tobytes()
    assert not np.array_equal(paired[0], first[0])
    a, b = bootstrap.finish(*first), bootstrap.finish(*paired)
    cmp = bootstrap.paired(a, b)
    assert cmp["n_valid"] == 20 and cmp["diff"] == a["auc"] - b["auc"] and cmp["se"] > 0
    # a row permutation with the uid column permuted alike: the same words; without units slot 0 alone
    p = np.random.RandomState(4).permutation(MID)
    moved = device_call(pred[p], label[p], 20, 12, unit=uid[p])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, moved))
    rows_a, rows_b = device_call(pred, label, 20, 12), device_call(pred[p], label[p], 20, 12)
    assert all(a[0] == b[0] for a, b in zip(rows_a, rows_b)) and not np.array_equal(rows_a[0][1:], rows_b[0][1:])


@pytest.mark.parametrize("name", ["3 values", "specials", "run ends on a tile border"])
def test_the_shared_sort_still_serves_exact_metrics(name):
    """mamdr_exact_metrics, d_sorted_out included, against exact.metrics_host (tests/test_gpu_exact.py is the main guard)."""
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    pred, label = data_case(name)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred, d_label = torch.from_numpy(pred.copy()).to(dev), torch.from_numpy(label.copy()).to(dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    ap = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    bins = torch.full((3, 10), -1, dtype=torch.int64, device=dev)
    out = torch.full((MID,), -1, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    L.check(lib.mamdr_exact_metrics(p(d_pred), p(d_label), MID, 10, p(counts), p(ap), p(bins), p(out),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    want = exact.metrics_host(pred, label, 10, want_sorted=True)
    assert counts.cpu().numpy().tolist() == want[0].tolist()
    assert np.array_equal(bins.cpu().numpy(), want[2]) and np.array_equal(out.cpu().numpy(), want[3])
    assert abs(ap.item() - want[1]) <= MID * 2.0 ** -52 * want[1]
    T, P, N = device_call(pred, label, 0, 0)
    assert [int(T[0]), int(P[0]), int(N[0])] == want[0][:3].tolist()


def test_bad_arguments_launch_nothing():
    """EINVAL with the outputs untouched (they keep their -1 fill)."""
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.zeros(8, dtype=torch.float32, device=dev)
    u = torch.zeros(8, dtype=torch.int32, device=dev)
    T, P, N = [torch.full((4,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, args in {"n < 0": (p(x), p(x), None, -1, 3, 0, p(T), p(P), p(N)),
                       "n = 2^27": (p(x), p(x), None, 2 ** 27, 3, 0, p(T), p(P), p(N)),
                       "n_rep < 0": (p(x), p(x), None, 8, -1, 0, p(T), p(P), p(N)),
                       "n_rep = 65,536": (p(x), p(x), None, 8, 65536, 0, p(T), p(P), p(N)),
                       "null pred": (None, p(x), None, 8, 3, 0, p(T), p(P), p(N)),
                       "null T": (p(x), p(x), None, 8, 3, 0, None, p(P), p(N)),
                       "null P": (p(x), p(x), None, 8, 3, 0, p(T), None, p(N)),
                       "null N": (p(x), p(x), None, 8, 3, 0, p(T), p(P), None),
                       "misaligned label": (p(x), p(x, 2), None, 4, 3, 0, p(T), p(P), p(N)),
                       "misaligned unit": (p(x), p(x), p(u, 1), 4, 3, 0, p(T), p(P), p(N)),
                       "misaligned T": (p(x), p(x), None, 8, 2, 0, p(T, 4), p(P), p(N))}.items():
        assert lib.mamdr_auc_bootstrap(*args, s) == L.EINVAL, what
    assert lib.mamdr_auc_bootstrap_bounded(p(x), p(x), None, 8, 3, 0, p(T), p(P), p(N), 0, s) == L.EINVAL
    torch.cuda.synchronize()
    assert all(t.tolist() == [-1] * 4 for t in (T, P, N))


# ------------------------------------------------------------------ the engine
def same(rep, want):
    assert set(rep) == set(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert rep[k].dtype == want[k].dtype and np.array_equal(rep[k], want[k], equal_nan=k == "replicates"), k
        else:
            assert rep[k] == want[k], k


def test_engine_auc_bootstrap_and_evaluate_with_ci():
    need_gpu()
    from test_gpu_exact import make_engine
    eng, g = make_engine("tower")
    for d in (0, 7):
        cols = g["data"]["test"][d]
        plain = eng.evaluate(d, "test", want_preds=True)
        with_ci = eng.evaluate(d, "test", want_preds=True, want_ci=(12, 5, "user"))
        every = eng.evaluate(d, "test", want_gauc=True, want_exact=10, want_ci=(12, 5, "row"))
        assert len(plain) == 4 and len(with_ci) == 5 and len(every) == 5
        assert plain[:2] == with_ci[:2] == every[:2] and plain[3].tobytes() == with_ci[3].tobytes()
        assert "gauc" in every[2] and "ece" in every[3] and "replicates" in every[4]          # GAUC's, exact's, then the CI's
        for rep, unit in ((with_ci[4], cols["uid"]), (every[4], None)):
            same(rep, bootstrap.finish(*bootstrap.replicates_host(plain[3], cols["label"], 12, 5, unit)))
        # slot 0 is mamdr_exact_metrics' T, P, N, and the estimate is exact.finish's AUC
        preds = torch.from_numpy(plain[3]).to(eng.device)
        labels = eng.data[(d, "test")]["label"]
        ex = eng.exact_metrics(preds, labels, 10, want_sorted=True)
        srt = ex["sorted"]
        positive = (srt & 1).astype(bool)
        direct = eng.auc_bootstrap(preds, labels, 12, seed=5, unit=eng.data[(d, "test")]["uid"])
        same(direct, with_ci[4])
        assert (int(direct["P"][0]), int(direct["N"][0])) == (ex["P"], ex["N"]) == (int(positive.sum()), int((~positive).sum()))
        assert direct["auc"] == ex["auc"] == every[3]["auc"] and np.array_equal(direct["T"], with_ci[4]["T"])
        assert int(direct["T"][0]) == exact.metrics_host(plain[3], cols["label"], 10)[0][0]
        print("domain %d: %d rows, exact AUC %.5f, by user se %.5f [%.5f, %.5f], by row se %.5f"
              % (d, len(cols["label"]), direct["auc"], direct["se"], direct["ci_lo"], direct["ci_hi"], every[4]["se"]))
    # the launcher's workspace bound (what the chunking test drives through the C call) through the engine
    T, P, N = eng._bootstrap_launch(preds, labels, 40, 5, part_words=1)
    whole = eng._bootstrap_launch(preds, labels, 40, 5)
    assert torch.equal(T, whole[0]) and torch.equal(P, whole[1]) and torch.equal(N, whole[2])
    with pytest.raises(ValueError):
        eng.evaluate(0, "test", want_ci=(12, 5, "item"))
    with pytest.raises(ValueError):
        eng.auc_bootstrap(preds, labels, 65536)
    with pytest.raises(ValueError):
        eng.auc_bootstrap(preds, labels[:-1], 4)
    with pytest.raises(ValueError):
        eng.auc_bootstrap(preds, labels, 4, unit=labels)
    eng.close()


# ------------------------------------------------------------------ end to end
def test_run_config_with_auc_ci(tmp_path, monkeypatch, capsys):
    """run.py's command line on the shipped Taobao-10 config (sized as tests/test_gpu_recommend.py's
    test_run_config_with_recommend sizes its run) with --exact-metrics 20 --auc-ci 200.  No quality bar, and no
    ci_lo <= AUC <= ci_hi either: a percentile interval need not contain the point estimate."""
    need_gpu()
    from mamdr_amd import cli, engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    path = str(tmp_path / "config.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    built, real_main = [], cli.main
    monkeypatch.setattr(cli, "main", lambda config, **kw: real_main(config, on_model=built.append, **kw))
    res = cli.cli(["--config", path, "--exact-metrics", "20", "--auc-ci", "200"])
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    assert isinstance(model.model, engine.TowerEngine)
    assert (model.train_config["report_auc_ci"], model.train_config["auc_ci_unit"], model.train_config["auc_ci_seed"]) == (200, "user", 0)
    rdir = os.path.join(model.result_path, os.listdir(model.result_path)[0])
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    domains = {str(d) for d in range(10)}
    for key in ("domain_auc_ci_lo", "domain_auc_ci_hi", "domain_auc_se", "domain_auc_ci_valid", "domain_auc_exact"):
        assert set(result[key]) == domains, key
    for d in domains:
        lo, hi = result["domain_auc_ci_lo"][d], result["domain_auc_ci_hi"][d]
        assert 0.0 <= lo <= hi <= 1.0 and result["domain_auc_se"][d] >= 0.0 and 0 <= result["domain_auc_ci_valid"][d] <= 200
        print("domain %s: exact AUC %.5f, interval [%.5f, %.5f], se %.5f, %d valid"
              % (d, result["domain_auc_exact"][d], lo, hi, result["domain_auc_se"][d], result["domain_auc_ci_valid"][d]))
    with np.load(os.path.join(rdir, "auc_bootstrap.npz")) as z:
        assert int(z["n_rep"]) == 200 and int(z["seed"]) == 0 and str(z["unit"]) == "user"
        saved = {k: z[k] for k in z.files}
    for d in range(10):
        assert saved["replicates_%d" % d].shape == (201,)
        assert saved["replicates_%d" % d][0] == result["domain_auc_exact"][str(d)]
        # a re-evaluation under the weights the test evaluation scored the domain with
        cols = model.dataset.test_dataset[d]["data"]
        with model._best_of_domain(d):
            preds = model.model.evaluate(d, "test", want_preds=True)[3]
        T, P, N = bootstrap.replicates_host(preds, cols["label"], 200, 0, cols["uid"])
        for k, want in (("T", T), ("P", P), ("N", N)):
            assert np.array_equal(saved["%s_%d" % (k, d)], want), (k, d)
        assert np.array_equal(saved["replicates_%d" % d], bootstrap.aucs(T, P, N), equal_nan=True)
    assert "Exact AUC, 200 bootstrap replicates by user (seed 0)" in capsys.readouterr().out
