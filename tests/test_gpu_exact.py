"""Exact AUC, average precision and calibration bins on the device (mamdr_exact_metrics, DeviceEngine.exact_metrics /
evaluate(want_exact=B)).

Every integer output -- T, P, N, n_runs, n_nan, the three bin arrays, the sorted composites -- is held to `==` against
exact.metrics_host (np.sort and np.cumsum: another algorithm).  The AP sum is held to a relative n * 2^-52: both sides form
each positive's term by the same correctly rounded division of the same two integers, so they differ in the order of the sum
alone, and any two orders of n non-negative terms are within (n - 1) * 2^-53 of the exact sum each (the bound gauc.py states
for its tree).

Sizes: the fixed list; every tile constant of the chain (exact.SORT_TILE, SCAN_TILE, METRIC_TILE) at -1, +0, +1; the sizes
at which a scan takes another path -- the histograms' scan leaves one tile behind 2 sort tiles, the runs' scan behind
SCAN_TILE metric tiles, the histograms' scan needs a third level behind SCAN_TILE^2 / 256 sort tiles, which is also the
smallest n that puts more than one workgroup into every launch of the chain bar the single-workgroup top of each scan --;
n = 0.  A host reference is computed once per (data, n_bins) and shared.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import exact      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32

FIXED = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 65537, 2 ** 20 + 3]
ONE_SCAN_TILE_OF_HISTOGRAMS = exact.SCAN_TILE // 2 ** exact.RADIX_BITS * exact.SORT_TILE        # 4,096: 2 sort tiles
ONE_SCAN_TILE_OF_RUNS = exact.SCAN_TILE * exact.METRIC_TILE                                      # 524,288
TWO_SCAN_LEVELS_OF_HISTOGRAMS = exact.SCAN_TILE ** 2 // 2 ** exact.RADIX_BITS * exact.SORT_TILE  # 2,097,152
EDGES = [exact.SORT_TILE, exact.SCAN_TILE, exact.METRIC_TILE, ONE_SCAN_TILE_OF_HISTOGRAMS, ONE_SCAN_TILE_OF_RUNS,
         TWO_SCAN_LEVELS_OF_HISTOGRAMS]
SIZES = sorted(set(FIXED + [e + d for e in EDGES for d in (-1, 0, 1)]))
MID = 3 * exact.SORT_TILE + 5 * 64 + 7          # 6,471 rows: 4 sort tiles, 7 metric tiles, a ragged last wave round

_CACHE = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def device_call(pred, label, n_bins, want_sorted=True, keep=None):
    """the stateless export on torch's current stream -> (counts, ap_sum, bins, sorted composites or None) as numpy; every
    output starts as -1 / NaN.  keep: a list that receives the two input tensors (the untouched-inputs test)."""
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred = torch.from_numpy(np.array(pred, dtype=F32)).to(dev)
    d_label = torch.from_numpy(np.array(label, dtype=F32)).to(dev)
    n = int(d_pred.numel())
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    ap = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    bins = torch.full((3, n_bins), -1, dtype=torch.int64, device=dev)
    out = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev) if want_sorted else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
    L.check(lib.mamdr_exact_metrics(ptr(d_pred), ptr(d_label), n, n_bins, ptr(counts), ptr(ap), ptr(bins), ptr(out),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    res = (counts.cpu().numpy(), float(ap.cpu().numpy()[0]), bins.cpu().numpy(), out.cpu().numpy()[:n] if want_sorted else None)
    if keep is not None:
        keep.extend([d_pred, d_label])
    return res


def host(name, pred, label, n_bins):
    """exact.metrics_host(want_sorted) of a named case: computed once, never modified."""
    key = (name, n_bins)
    if key not in _CACHE:
        ref = exact.metrics_host(pred, label, n_bins, want_sorted=True)
        for a in (ref[0], ref[2], ref[3]):
            a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def check(name, pred, label, n_bins, **kw):
    """device == host on every integer, the AP sum within n * 2^-52 relative -> the device's outputs."""
    want = host(name, pred, label, n_bins)
    got = device_call(pred, label, n_bins, **kw)
    n = len(pred)
    assert np.array_equal(got[3], want[3]), (name, np.flatnonzero(got[3] != want[3])[:10])
    assert got[0].tolist() == want[0].tolist(), (name, dict(zip(exact.COUNTS, zip(got[0].tolist(), want[0].tolist()))))
    for row, what in enumerate(("rows", "positives", "Q32 sums")):
        assert np.array_equal(got[2][row], want[2][row]), (name, what, np.flatnonzero(got[2][row] != want[2][row])[:10])
    print("%s: n %d, AP sum device %.17g host %.17g, relative difference %.3e, bound %.3e"
          % (name, n, got[1], want[1], abs(got[1] - want[1]) / want[1] if want[1] else 0.0, n * 2.0 ** -52))
    assert abs(got[1] - want[1]) <= n * 2.0 ** -52 * want[1]
    return got


def mixed(n, seed=0):
    """continuous predictions, one row in four quantised to 8 levels (long tie runs), CTR-like labels drawn from them."""
    key = ("mixed", n, seed)
    if key not in _CACHE:
        rs = np.random.RandomState(1000 + seed)
        pred = rs.random_sample(n).astype(F32)
        coarse = rs.random_sample(n) < 0.25
        pred[coarse] = (np.floor(pred[coarse] * 8) / 8).astype(F32)
        label = (rs.random_sample(n) < 0.05 + 0.3 * pred).astype(F32)
        pred.setflags(write=False)
        label.setflags(write=False)
        _CACHE[key] = (pred, label)
    return _CACHE[key]


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", SIZES)
def test_every_size(n):
    need_gpu()
    pred, label = mixed(n)
    got = check("mixed%d" % n, pred, label, 10)
    assert got[0][1] + got[0][2] == n and got[2][0].sum() == n


def test_empty_split():
    need_gpu()
    counts, ap, bins, out = device_call(np.zeros(0, F32), np.zeros(0, F32), 10)
    assert counts.tolist() == [0] * 5 and ap == 0.0 and not bins.any() and out.size == 0
    assert exact.finish(counts, ap, bins)["valid"] == 0


# ------------------------------------------------------------------ data
def keys_case(bits, n=MID, seed=0):
    """predictions whose ordered keys differ from 0xbf000000 (0.5) in the given key bits only."""
    rs = np.random.RandomState(50 + seed)
    key = np.full(n, 0xbf000000, np.uint32)
    for b in bits:
        key ^= (rs.randint(0, 2, n).astype(np.uint32) << np.uint32(b))
    pred = exact.prediction_of_key(key).copy()
    assert not np.isnan(pred).any() and np.array_equal(exact.gauc.ordered_key(pred), key)
    return pred, (rs.random_sample(n) < 0.3).astype(F32)


def data_case(name):
    rs = np.random.RandomState(7)
    n = MID
    label = (rs.random_sample(n) < 0.3).astype(F32)
    distinct = (rs.permutation(n) / F32(n)).astype(F32)              # n different values in [0, 1)
    if name == "all equal":
        return np.full(n, 0.3, F32), label
    if name == "all distinct":
        return distinct, label
    if name in ("2 values", "8 values"):
        return (rs.randint(0, int(name[0]), n) / F32(8)).astype(F32), label
    if name == "ascending":
        return np.sort(distinct), label
    if name == "descending":
        return np.sort(distinct)[::-1].copy(), label
    if name == "all positive":
        return distinct, np.ones(n, F32)
    if name == "all negative":
        return distinct, np.zeros(n, F32)
    if name == "labels 2 and -1":
        return distinct, rs.choice(np.array([0.0, 2.0, -1.0], F32), n)
    if name == "specials":
        tiny = np.float32(1e-45)
        pool = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1e-39, -1e-39, -2.5, -0.25, 1.0, 1.5, 7e37,
                         0.25, 0.75, np.nextafter(F32(0.75), F32(1))], F32)
        return rs.choice(pool, n), label
    # the composite's digits are 8 bits wide and the key starts at composite bit 1: key bits (6, 7), (14, 15), (22, 23) and
    # (30, 31) sit on either side of a digit boundary, key bit 0 is the lowest, key bit 31 the last pass's only bit
    bits = {"lowest key bit": (0,), "top key bit": (31,), "digits 0|1": (6, 7), "digits 1|2": (14, 15), "digits 2|3": (22, 23),
            "digits 3|4": (30, 31)}[name]
    return keys_case(bits)


DATA = ["all equal", "all distinct", "2 values", "8 values", "lowest key bit", "top key bit", "digits 0|1", "digits 1|2",
        "digits 2|3", "digits 3|4", "ascending", "descending", "all positive", "all negative", "labels 2 and -1", "specials"]


@pytest.mark.parametrize("name", DATA)
def test_every_kind_of_data(name):
    need_gpu()
    pred, label = data_case(name)
    counts = check(name, pred, label, 10)[0]
    T, P, N, n_runs, n_nan = counts.tolist()
    if name == "all equal":
        assert T == P * N and n_runs == 1                      # every pair ties: AUC exactly 1/2
    if name in ("all distinct", "ascending", "descending"):
        assert n_runs == MID
    if name in ("2 values", "8 values"):
        assert n_runs == int(name[0])
    if name == "all positive":
        assert (T, P, N) == (0, MID, 0)
    if name == "all negative":
        assert (T, P, N) == (0, 0, MID)
    if name == "labels 2 and -1":
        assert P == int((label != 0).sum()) and P > MID // 2
    if name == "specials":
        assert n_nan == int(np.isnan(pred).sum()) and n_nan > 0 and n_runs == 16      # -nan == nan, -0 == +0
    if name in ("lowest key bit", "top key bit"):
        assert n_runs == 2
    if name.startswith("digits"):
        assert n_runs == 4


@pytest.mark.parametrize("n_bins", [1, 10, 4096])
@pytest.mark.parametrize("n", [1000, 3000, 70001])
def test_bin_counts(n, n_bins):
    """1,000 and 3,000 rows: n_bins = 4,096 > n, a tile's bins spread beyond its LDS slots, in one metric tile and in three;
    70,001 rows: 69 metric tiles."""
    need_gpu()
    pred, label = mixed(n, seed=1)
    bins = check("bins%d" % n, pred, label, n_bins)[2]
    assert bins[0].sum() == n and bins[0].shape == (n_bins,)


def test_quantised_predictions_leave_bins_empty():
    need_gpu()
    pred, label = data_case("8 values")
    bins = check("8 values", pred, label, 64)[2]
    assert np.count_nonzero(bins[0]) <= 8 and bins[0].sum() == MID


def test_the_optional_output_and_the_inputs():
    """without d_sorted_out the same outputs; the two input tensors are bitwise what they were."""
    need_gpu()
    pred, label = data_case("specials")
    kept = []
    with_out = device_call(pred, label, 10, want_sorted=True, keep=kept)
    torch.cuda.synchronize()
    assert kept[0].cpu().numpy().tobytes() == np.asarray(pred, F32).tobytes()
    assert kept[1].cpu().numpy().tobytes() == np.asarray(label, F32).tobytes()
    without = device_call(pred, label, 10, want_sorted=False)
    assert without[3] is None and without[0].tolist() == with_out[0].tolist() and np.array_equal(without[2], with_out[2])
    assert np.float64(without[1]).tobytes() == np.float64(with_out[1]).tobytes()


@pytest.mark.parametrize("n", [MID, ONE_SCAN_TILE_OF_RUNS + 1])
def test_bits_under_a_row_permutation_and_between_runs(n):
    need_gpu()
    pred, label = mixed(n, seed=2)
    first = check("perm%d" % n, pred, label, 10)
    p = np.random.RandomState(4).permutation(n)
    for again in (device_call(pred, label, 10), device_call(pred[p], label[p], 10)):
        assert again[0].tobytes() == first[0].tobytes() and again[2].tobytes() == first[2].tobytes()
        assert again[3].tobytes() == first[3].tobytes()
        assert np.float64(again[1]).tobytes() == np.float64(first[1]).tobytes()         # AP: the same bits


def test_bad_arguments_launch_nothing():
    """EINVAL with the outputs untouched (they keep their -1 fill)."""
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.zeros(8, dtype=torch.float32, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    ap = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    bins = torch.full((3, 4), -1, dtype=torch.int64, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, args in {"n < 0": (p(x), p(x), -1, 4, p(counts), p(ap), p(bins), None),
                       "n = 2^31": (p(x), p(x), 2 ** 31, 4, p(counts), p(ap), p(bins), None),
                       "no bins": (p(x), p(x), 8, 0, p(counts), p(ap), p(bins), None),
                       "4,097 bins": (p(x), p(x), 8, 4097, p(counts), p(ap), p(bins), None),
                       "null pred": (None, p(x), 8, 4, p(counts), p(ap), p(bins), None),
                       "null counts": (p(x), p(x), 8, 4, None, p(ap), p(bins), None),
                       "misaligned label": (p(x), p(x, 2), 4, 4, p(counts), p(ap), p(bins), None),
                       "misaligned bins": (p(x), p(x), 8, 4, p(counts), p(ap), p(bins, 4), None)}.items():
        assert lib.mamdr_exact_metrics(*args, s) == L.EINVAL, what
    torch.cuda.synchronize()
    assert counts.tolist() == [-1] * 5 and ap.item() == -1.0 and bool((bins == -1).all())


# ------------------------------------------------------------------ the engines
def gen(emb_dim):
    if ("g", emb_dim) not in _CACHE:
        from mamdr_amd import synthetic
        _CACHE[("g", emb_dim)] = synthetic.generate("taobao10", batch_size=256, seed=7, scale=0.05, emb_dim=emb_dim)
    return _CACHE[("g", emb_dim)]


def make_engine(which):
    """the step engine's mlp, or the generic-layer engine's 64-wide mlp as tests/test_gpu_rank.py builds it; frozen tables,
    every test split bound, random weights."""
    from mamdr_amd import engine, graph_engine
    if which == "tower":
        g = gen(128)
        eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 256, dropout=0.5, emb_trainable=False, tower="mlp")
    else:
        g = gen(64)
        assert (g["n_user"], g["n_item"], g["n_domain"]) == (1188, 346, 10)
        eng = graph_engine.GraphEngine("mlp", 1188, 346, 10, 256, (128, 64), (), emb_dim=64)
    eng.bind_table("user_emb", g["tables"]["user_emb"])
    eng.bind_table("item_emb", g["tables"]["item_emb"])
    for d in range(g["n_domain"]):
        c = g["data"]["test"][d]
        eng.bind_domain_data(d, "test", c["uid"], c["pid"], c["domain"], c["label"])
    rs = np.random.RandomState(7)
    named = {n: (rs.standard_normal(cnt) * (0.0 if n in ("user_emb", "item_emb") else 0.08)).astype(F32)
             for n, (off, cnt) in eng.segments.items()}
    eng.set_weights(eng.pack(named))
    return eng, g


def same_report(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("which", ["tower", "graph"])
def test_engine_evaluate_with_exact(which):
    need_gpu()
    eng, g = make_engine(which)
    for d in (0, 4, 9):
        cols = g["data"]["test"][d]
        plain = eng.evaluate(d, "test", want_preds=True)
        both = eng.evaluate(d, "test", want_preds=True, want_exact=10)
        only = eng.evaluate(d, "test", want_exact=10)
        every = eng.evaluate(d, "test", want_preds=True, want_gauc=True, want_exact=10)
        assert len(plain) == 4 and len(both) == 5 and len(only) == 3 and len(every) == 6
        # loss, AUC-500, histogram and predictions: the bits of a call without the key
        assert plain[0] == both[0] == only[0] == every[0] and plain[1] == both[1] == only[1] == every[1]
        assert np.array_equal(plain[2], both[2]) and plain[3].tobytes() == both[3].tobytes() == every[3].tobytes()
        assert eng.evaluate(d, "test") == plain[:2] and eng.evaluate(d, "test", want_exact=0) == plain[:2]
        rep = both[4]
        same_report(only[2], rep)
        same_report(every[5], rep)                               # after GAUC's report
        assert every[4] == eng.evaluate(d, "test", want_gauc=True)[2] and "gauc" in every[4]
        counts, ap_sum, bins, srt = exact.metrics_host(both[3], cols["label"], 10, want_sorted=True)
        want = exact.finish(counts, ap_sum, bins)
        n = len(cols["label"])
        for k in ("auc", "valid", "P", "N", "n_runs", "n_nan", "ece", "pcoc"):
            assert rep[k] == want[k], k                          # integers and what finish() makes of integers
        for k in ("bin_rows", "bin_positives", "bin_pred_q32", "bin_pred_sum"):
            assert np.array_equal(rep[k], want[k]), k
        assert abs(rep["ap"] - want["ap"]) <= n * 2.0 ** -52 * want["ap"]
        print("%s engine, domain %d: %d rows, AUC-500 %.6f exact %.6f AP %.6f ECE %.4f PCOC %.3f"
              % (which, d, n, both[1], rep["auc"], rep["ap"], rep["ece"], rep["pcoc"]))
        # the direct form on device tensors
        direct = eng.exact_metrics(torch.from_numpy(both[3]).to(eng.device), eng.data[(d, "test")]["label"], 10, want_sorted=True)
        assert np.array_equal(direct.pop("sorted"), srt)
        same_report(direct, rep)
    with pytest.raises(ValueError):
        eng.evaluate(0, "test", want_exact=4097)
    with pytest.raises(ValueError):
        eng.exact_metrics(torch.zeros(4, device=eng.device), torch.zeros(5, device=eng.device), 10)
    eng.close()


# ------------------------------------------------------------------ end to end
def test_run_config_with_exact_metrics(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 config (sized as tests/test_gpu_gauc.py sizes its run) with
    train.report_exact.  No quality bar: the saved figures are those of the printed summary and of a valid report."""
    need_gpu()
    import copy
    import json
    import os
    from mamdr_amd import cli, engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5, report_exact=16,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    assert isinstance(model.model, engine.TowerEngine)
    rdir = os.path.join(model.result_path, os.listdir(model.result_path)[0])
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    domains = {str(d) for d in range(10)}
    for key in ("domain_auc_exact", "domain_ap", "domain_ece", "domain_pcoc"):
        assert set(result[key]) == domains, key
    assert all(0.0 < v < 1.0 for v in result["domain_auc_exact"].values())
    assert 0.0 < result["avg_auc_exact"] < 1.0 and 0.0 < result["weighted_auc_exact"] < 1.0
    with np.load(os.path.join(rdir, "exact_metrics.npz")) as z:
        assert z["bin_rows"].shape == (10, 16) and z["domains"].tolist() == list(range(10))
        info = model.dataset.dataset_info
        assert z["bin_rows"].sum(axis=1).tolist() == [info[d]["n_test"] for d in range(10)]
    # the remembered reports are the test evaluations' own
    for d in range(10):
        rep = model.exact_reports[("test", d)]
        assert rep["valid"] == 1 and result["domain_auc_exact"][str(d)] == rep["auc"] and result["domain_ap"][str(d)] == rep["ap"]
    text = capsys.readouterr().out
    assert "Overall test Exact AUC: {}, Weighted Exact AUC: {}".format(result["avg_auc_exact"], result["weighted_auc_exact"]) in text
    print(text[text.rindex("Exact AUC: \n"):])
