"""The isotonic fit, its application and the score sums on the device (mamdr_isotonic_fit(_bounded), mamdr_isotonic_apply,
mamdr_score_sums; DeviceEngine.isotonic_fit / isotonic_apply / score_sums; run.py --isotonic).

Every integer output of the fit -- the four counts and the block table -- is held to `==` against isotonic.fit_host (np.sort
and a stack of pooled blocks: another algorithm), the applied values to the bits of isotonic.apply_host.  Each fit case runs
through mamdr_isotonic_fit and through mamdr_isotonic_fit_bounded at tile_points = isotonic.MIN_TILE, 8 and 64, and under a
row permutation: identical bytes.  The score sums are held to a relative 1e-12 against isotonic.score_sums_host (math.fsum):
both sums have non-negative terms, each computed in fp64 to a few ulp (2^-50), and a tree of depth <= 32 adds <= 33 * 2^-53;
together < 3e-15, so 1e-12 leaves more than 300 x.

Sizes are at most 5,000 rows; the host references are computed once per case and shared (tests/test_isotonic_host.py holds
the cases)."""
import copy
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_exact as ex          # noqa: E402  (the small engines)
import test_isotonic_host as ih      # noqa: E402  (the cases)
from mamdr_amd import isotonic       # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (None, isotonic.MIN_TILE, 8, 64)         # None: mamdr_isotonic_fit

_CACHE = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_fit(pred, label, tile=None):
    """the stateless export on torch's current stream -> (counts [4], first_key uint32 [n_blocks], rows, positives, and the
    untouched tails of the three arrays); every output starts as -1."""
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred = torch.from_numpy(np.array(pred, dtype=F32)).to(dev)
    d_label = torch.from_numpy(np.array(label, dtype=F32)).to(dev)
    n = int(d_pred.numel())
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    fk = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    rows, pos = [torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev) for _ in range(2)]
    args = (ptr(d_pred), ptr(d_label), n, ptr(counts), ptr(fk), ptr(rows), ptr(pos))
    if tile is None:
        L.check(lib.mamdr_isotonic_fit(*args, stream()))
    else:
        L.check(lib.mamdr_isotonic_fit_bounded(*args, tile, stream()))
    counts, fk, rows, pos = counts.cpu().numpy(), fk.cpu().numpy().view(np.uint32), rows.cpu().numpy(), pos.cpu().numpy()
    nb = int(counts[0])
    assert 0 <= nb <= n
    assert np.all(fk[nb:] == 0xffffffff) and np.all(rows[nb:] == -1) and np.all(pos[nb:] == -1)      # nothing behind the table
    return counts, fk[:nb], rows[:nb], pos[:nb]


def fit_case(name):
    """(pred, label) of a named case and its host fit: computed once, never modified."""
    if name not in _CACHE:
        half = np.arange(1, 41, dtype=F32) / F32(64)
        if name in ("q64", "continuous"):
            p, y = ih.cases()[name]
        elif name == "convex":
            p, y, _ = ih.convex_case()
        elif name == "specials":
            p, y = ih.SPECIALS
        else:
            p, y = {"n1 positive": ([0.3], [1]), "n1 negative": ([0.3], [0]), "n2 tied": ([0.7, 0.7], [1, 0]),
                    "all equal": ([0.25] * 300, ([1, 0, 0] * 100)), "all negative": (half, np.zeros(40)),
                    "all positive": (half, np.ones(40)), "anti-monotone": (half, (np.arange(40) < 20))}[name]
        p, y = np.array(p, dtype=F32), np.array(y, dtype=F32)
        ref = isotonic.fit_host(p, y)
        for a in (p, y) + ref:
            a.setflags(write=False)
        _CACHE[name] = (p, y, ref)
    return _CACHE[name]


FIT_CASES = ["n1 positive", "n1 negative", "n2 tied", "all equal", "all negative", "all positive", "anti-monotone", "specials",
             "convex", "q64", "continuous"]


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_equals_the_host_definition_under_every_tile(name):
    need_gpu()
    p, y, want = fit_case(name)
    first = None
    for tile in TILES:
        got = device_fit(p, y, tile)
        for g, w, what in zip(got, want, ("counts", "first_key", "rows", "positives")):
            assert np.array_equal(g, w), (name, tile, what, g[:10], w[:10])
        if first is None:
            first = got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first)), (name, tile)
    counts, fk, rows, pos = first
    n_blocks, n_runs, n_nan, P = counts.tolist()
    print("%s: %d rows, %d runs, %d blocks; levels at tile 4 / 8 / 64: %s" % (
        name, len(p), n_runs, n_blocks, [isotonic.levels(len(p), t) for t in (4, 8, 64)]))
    assert rows.sum() == len(p) and pos.sum() == P == int((y != 0).sum()) and n_nan == int(np.isnan(p).sum())
    if name in ("n1 positive", "n1 negative", "n2 tied", "all equal", "all negative", "all positive", "anti-monotone"):
        assert n_blocks == 1
    if name == "specials":
        assert rows.tolist() == [6, 2, 2] and pos.tolist() == [2, 1, 2] and n_nan == 2
    if name == "convex":
        assert (len(p), n_runs, n_blocks) == (328, 43, 43)          # nothing may be dropped at any level
    if name == "q64":
        assert n_runs <= 65 and n_blocks < n_runs
    if name == "continuous":
        # a block that covers more than 60 tiles of 8 points: blocks cross many tile borders, several levels run
        run_key = isotonic.runs_host(p, y)[0]
        start = np.searchsorted(run_key, fk)
        assert n_runs > 4900 and np.diff(np.concatenate([start, [n_runs]])).max() > 60 * 8 and isotonic.levels(len(p), 8) >= 3


@pytest.mark.parametrize("name", ["specials", "q64", "continuous"])
def test_fit_bits_under_a_row_permutation(name):
    need_gpu()
    p, y, want = fit_case(name)
    perm = np.random.RandomState(4).permutation(len(p))
    for tile in (None, isotonic.MIN_TILE):
        got = device_fit(p[perm], y[perm], tile)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (name, tile)


def second_draw():
    """5,000 predictions of another seed, the specials among them."""
    rng = np.random.default_rng(11)
    x = (1 / (1 + np.exp(-rng.normal(-2, 1.5, 5000)))).astype(F32)
    x[::97] = np.resize(ih.SPECIALS[0], len(x[::97]))
    x[1::2] = (np.round(x[1::2] * 64) / 64).astype(F32)           # every other row on the q64 grid: rows AT thresholds
    return x


@pytest.mark.parametrize("name", ["q64", "continuous", "specials", "n1 positive"])
def test_apply_is_bit_equal_to_apply_host(name):
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    _, _, (counts, fk, rows, pos) = fit_case(name)
    x = second_draw()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(np.array(a).view(t)).to(dev)      # noqa: E731
    d_fk, d_rows, d_pos, d_x = up(fk, np.int32), up(rows, np.int64), up(pos, np.int64), up(x, F32)
    out = torch.full((len(x),), -7.0, dtype=torch.float32, device=dev)
    L.check(lib.mamdr_isotonic_apply(ptr(d_fk), ptr(d_rows), ptr(d_pos), len(fk), ptr(d_x), len(x), ptr(out), stream()))
    want = isotonic.apply_host(fk, rows, pos, x)
    got = out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (name, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10])
    assert d_x.cpu().numpy().tobytes() == x.tobytes()
    L.check(lib.mamdr_isotonic_apply(ptr(d_fk), ptr(d_rows), ptr(d_pos), len(fk), None, 0, None, stream()))      # n = 0


def test_apply_beyond_the_lds_table():
    """more blocks than k_iso_apply stages in LDS: 4,500 strictly increasing block means, searched in global memory."""
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    nb = isotonic.APPLY_LDS + 404
    fk = isotonic.gauc.ordered_key((np.arange(nb) / F32(nb)).astype(F32))
    rows, pos = np.full(nb, nb, np.int64), np.arange(nb, dtype=np.int64)
    x = second_draw()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(np.array(a).view(t)).to(dev)      # noqa: E731
    d_fk, d_rows, d_pos, d_x = up(fk, np.int32), up(rows, np.int64), up(pos, np.int64), up(x, F32)
    out = torch.full((len(x),), -7.0, dtype=torch.float32, device=dev)
    L.check(lib.mamdr_isotonic_apply(ptr(d_fk), ptr(d_rows), ptr(d_pos), nb, ptr(d_x), len(x), ptr(out), stream()))
    assert out.cpu().numpy().tobytes() == isotonic.apply_host(fk, rows, pos, x).tobytes()


def device_sums(pred, label):
    from mamdr_amd import _lib as L
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred, d_label = torch.from_numpy(np.array(pred, dtype=F32)).to(dev), torch.from_numpy(np.array(label, dtype=F32)).to(dev)
    out = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    L.check(L.load().mamdr_score_sums(ptr(d_pred), ptr(d_label), len(pred), ptr(out), stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["n1 positive", "n2 tied", "all equal", "q64", "continuous"])
def test_score_sums(name):
    need_gpu()
    p, y, _ = fit_case(name)
    if name == "continuous":         # saturated rows: both clamps, on either label
        p = p.copy()
        p[:8] = [0.0, 0.0, 1.0, 1.0, -3.0, 7.0, 1e-9, 1 - 1e-9]
    want = isotonic.score_sums_host(p, y)
    got = device_sums(p, y)
    again = device_sums(p, y)
    for g, w, what in zip(got, want, ("Brier", "log loss")):
        print("%s: %s sum device %.17g host %.17g, relative difference %.3e" % (name, what, g, w, abs(g - w) / w if w else 0.0))
        assert abs(g - w) <= 1e-12 * w
    assert got.tobytes() == again.tobytes()


def test_score_sums_with_a_nan_row_and_of_nothing():
    need_gpu()
    p, y, _ = fit_case("q64")
    p = p.copy()
    p[1234] = np.nan
    assert np.isnan(device_sums(p, y)).all()
    assert device_sums(np.zeros(0, F32), np.zeros(0, F32)).tolist() == [0.0, 0.0]


def test_empty_split_and_bad_arguments_launch_nothing():
    """n = 0 writes zero counts; every MAMDR_EINVAL leaves the outputs untouched (they keep their -1 fill); the engine's
    own refusals come before the library is called."""
    need_gpu()
    from mamdr_amd import _lib as L
    lib = L.load()
    counts, fk, rows, pos = device_fit(np.zeros(0, F32), np.zeros(0, F32))
    assert counts.tolist() == [0, 0, 0, 0] and fk.size == rows.size == pos.size == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.full((8,), 0.5, dtype=torch.float32, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    fk = torch.full((8,), -1, dtype=torch.int32, device=dev)
    rows, pos = [torch.full((8,), -1, dtype=torch.int64, device=dev) for _ in range(2)]
    out = torch.full((8,), -1.0, dtype=torch.float32, device=dev)
    sums = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731
    s = stream()
    fit, bounded, apply, score = lib.mamdr_isotonic_fit, lib.mamdr_isotonic_fit_bounded, lib.mamdr_isotonic_apply, lib.mamdr_score_sums
    for what, code in {"n < 0": fit(p(x), p(x), -1, p(counts), p(fk), p(rows), p(pos), s),
                       "n = 2^31": fit(p(x), p(x), 2 ** 31, p(counts), p(fk), p(rows), p(pos), s),
                       "null pred": fit(None, p(x), 8, p(counts), p(fk), p(rows), p(pos), s),
                       "null counts": fit(p(x), p(x), 8, None, p(fk), p(rows), p(pos), s),
                       "null rows": fit(p(x), p(x), 8, p(counts), p(fk), None, p(pos), s),
                       "misaligned label": fit(p(x), p(x, 2), 4, p(counts), p(fk), p(rows), p(pos), s),
                       "misaligned positives": fit(p(x), p(x), 4, p(counts), p(fk), p(rows), p(pos, 4), s),
                       "tile below the minimum": bounded(p(x), p(x), 8, p(counts), p(fk), p(rows), p(pos), isotonic.MIN_TILE - 1, s),
                       "apply without blocks": apply(p(fk), p(rows), p(pos), 0, p(x), 8, p(out), s),
                       "apply with -1 blocks": apply(p(fk), p(rows), p(pos), -1, p(x), 8, p(out), s),
                       "apply, null out": apply(p(fk), p(rows), p(pos), 2, p(x), 8, None, s),
                       "apply, misaligned rows": apply(p(fk), p(rows, 4), p(pos), 2, p(x), 4, p(out), s),
                       "sums, n < 0": score(p(x), p(x), -1, p(sums), s), "sums, null out": score(p(x), p(x), 8, None, s),
                       "sums, misaligned out": score(p(x), p(x), 8, p(sums, 4), s)}.items():
        assert code == L.EINVAL, what
    torch.cuda.synchronize()
    assert counts.tolist() == [-1] * 4 and bool((fk == -1).all()) and bool((rows == -1).all()) and bool((pos == -1).all())
    assert bool((out == -1).all()) and bool((sums == -1).all())
    # the engine refuses on the host, before the library is called
    eng, _ = ex.make_engine("tower")
    launched = []
    real = {n: getattr(eng.lib, n) for n in ("mamdr_isotonic_fit", "mamdr_isotonic_fit_bounded", "mamdr_isotonic_apply", "mamdr_score_sums")}
    try:
        for n in real:
            setattr(eng.lib, n, lambda *a: launched.append(a) or 0)
        y5 = torch.zeros(5, device=eng.device)
        with pytest.raises(ValueError):
            eng.isotonic_fit(x, y5)
        with pytest.raises(ValueError):
            eng.isotonic_fit(x, x, tile_points=isotonic.MIN_TILE - 1)
        with pytest.raises(ValueError):
            eng.isotonic_fit(x.double(), x.double())
        with pytest.raises(ValueError):
            eng.score_sums(x, y5)
        with pytest.raises(ValueError):
            eng.isotonic_apply(isotonic.table(*isotonic.fit_host(np.zeros(0, F32), np.zeros(0, F32))), x)
        with pytest.raises(ValueError):
            eng.isotonic_apply(isotonic.table(*isotonic.fit_host([0.5], [1])), x.double())
    finally:
        for n, fn in real.items():
            setattr(eng.lib, n, fn)
    assert not launched
    eng.close()


# ------------------------------------------------------------------ the engines
def engine_digest(eng, which):
    if which == "tower":
        import test_gpu_recommend as base
        return base.state_digest(eng)
    return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (eng.weights, eng.adam_m, eng.adam_v)]


@pytest.mark.parametrize("which", ["tower", "graph"])
def test_engine_fit_apply_sums_and_isotonic_eval(which):
    need_gpu()
    from mamdr_amd.model_zoo.base_model import BaseModel
    eng, g = ex.make_engine(which)
    for d in (0, 4, 9):
        c = g["data"]["val"][d]
        eng.bind_domain_data(d, "val", c["uid"], c["pid"], c["domain"], c["label"])
    before = engine_digest(eng, which)
    for d in (0, 4, 9):
        host = {s: eng.evaluate(d, s, want_preds=True)[3] for s in ("val", "test")}
        label = {s: np.asarray(g["data"][s][d]["label"], F32) for s in ("val", "test")}
        dev_p = {s: eng.predict_device(d, s) for s in ("val", "test")}
        for s in ("val", "test"):
            assert dev_p[s].device == eng.device and dev_p[s].cpu().numpy().tobytes() == host[s].tobytes()
        fits = {}
        for s in ("val", "test"):
            want = isotonic.table(*isotonic.fit_host(host[s], label[s]))
            fits[s] = eng.isotonic_fit(dev_p[s], eng.data[(d, s)]["label"])
            small = eng.isotonic_fit(dev_p[s], eng.data[(d, s)]["label"], tile_points=isotonic.MIN_TILE)
            for got in (fits[s], small):
                assert set(got) == set(want)
                for k in want:
                    assert (got[k].tobytes() == want[k].tobytes()) if isinstance(want[k], np.ndarray) else got[k] == want[k], (d, s, k)
        fitted = eng.isotonic_apply(fits["val"], dev_p["test"])
        want_fitted = isotonic.apply_host(fits["val"]["first_key"], fits["val"]["rows"], fits["val"]["positives"], host["test"])
        assert fitted.cpu().numpy().tobytes() == want_fitted.tobytes()
        for p_dev, p_host in ((dev_p["test"], host["test"]), (fitted, want_fitted)):
            got, want = eng.score_sums(p_dev, eng.data[(d, "test")]["label"]), isotonic.score_sums_host(p_host, label["test"])
            assert all(abs(a - b) <= 1e-12 * b for a, b in zip(got, want)), (d, got, want)
        rep = BaseModel.isotonic_eval(type("M", (), {"model": eng})(), d, 10)
        n = len(label["test"])
        brier = isotonic.score_sums_host(host["test"], label["test"])[0] / n
        assert abs(rep["brier"] - brier) <= 1e-12 * brier and rep["n"] == n and rep["n_blocks"] == fits["val"]["n_blocks"]
        assert abs(rep["brier"] - (rep["mcb"] - rep["dsc"] + rep["unc"])) <= 1e-12 and rep["mcb"] >= -1e-12 and rep["dsc"] >= -1e-12
        assert rep["ece"] == eng.exact_metrics(dev_p["test"], eng.data[(d, "test")]["label"], 10)["ece"]
        print("%s engine, domain %d: %d rows, %d val blocks; Brier %.6f -> %.6f, ECE %.4f -> %.4f, MCB %.6f DSC %.6f UNC %.6f"
              % (which, d, n, rep["n_blocks"], rep["brier"], rep["brier_isotonic"], rep["ece"], rep["ece_isotonic"],
                 rep["mcb"], rep["dsc"], rep["unc"]))
    assert engine_digest(eng, which) == before
    eng.close()


# ------------------------------------------------------------------ end to end
def test_run_config_with_isotonic(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 MAMDR config (sized as tests/test_gpu_rank.py sizes its run) with
    train.isotonic: isotonic.npz and every result.json key exist; per domain the CORP identity, domain_brier and the val
    table are those of the host definition on that domain's predictions under its own merged weights.  No quality bar:
    the recalibrated Brier may be worse on a tiny split; both are printed."""
    need_gpu()
    from mamdr_amd import cli, engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5, isotonic=20,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    eng = model.model
    assert isinstance(eng, engine.TowerEngine)
    rdir = [os.path.join(model.result_path, f) for f in os.listdir(model.result_path) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    domains = [str(d) for d in range(10)]
    for key in ("domain_brier", "domain_brier_isotonic", "domain_logloss", "domain_logloss_isotonic", "domain_ece_isotonic",
                "domain_pcoc_isotonic", "domain_mcb", "domain_dsc", "domain_unc", "domain_isotonic_blocks"):
        assert sorted(result[key]) == sorted(domains), key
    assert "avg_mcb" in result and "weighted_mcb" in result
    digest = lambda: hashlib.sha256(eng.weights.cpu().numpy().tobytes()).hexdigest()      # noqa: E731
    before = digest()
    keep = eng.get_weights().clone()
    with np.load(os.path.join(model.result_path, "isotonic.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and int(z["n_bins"]) == 20
        for d in range(10):
            merged = eng.new_vector(meta=True)
            eng.merge(merged, model.best_shared_weights, model.best_domain_weights[d], cfg["train"]["merged_method"])
            eng.assign_meta(merged)
            val_p, test_p = eng.evaluate(d, "val", want_preds=True)[3], eng.evaluate(d, "test", want_preds=True)[3]
            eng.set_weights(keep)
            val_y = np.asarray(model.dataset.val_dataset[d]["data"]["label"], F32)
            test_y = np.asarray(model.dataset.test_dataset[d]["data"]["label"], F32)
            counts, fk, rows, pos = isotonic.fit_host(val_p, val_y)
            assert np.array_equal(z["val_first_key_%d" % d], fk) and np.array_equal(z["val_rows_%d" % d], rows)
            assert np.array_equal(z["val_positives_%d" % d], pos) and z["counts_%d" % d][0].tolist() == counts.tolist() + [len(val_y)]
            assert z["val_first_pred_%d" % d].tobytes() == isotonic.exact.prediction_of_key(fk).tobytes()
            t = isotonic.fit_host(test_p, test_y)
            assert np.array_equal(z["test_rows_%d" % d], t[2]) and np.array_equal(z["test_positives_%d" % d], t[3])
            s = str(d)
            brier = isotonic.score_sums_host(test_p, test_y)[0] / len(test_y)
            assert abs(result["domain_brier"][s] - brier) <= 1e-12 * brier
            mcb, dsc, unc = result["domain_mcb"][s], result["domain_dsc"][s], result["domain_unc"][s]
            assert abs(result["domain_brier"][s] - (mcb - dsc + unc)) <= 1e-12 and mcb >= -1e-12 and dsc >= -1e-12
            assert result["domain_isotonic_blocks"][s] == len(fk)
            print("domain %d: Brier %.6f, recalibrated %.6f" % (d, result["domain_brier"][s], result["domain_brier_isotonic"][s]))
    assert digest() == before
    before_eval = digest()
    model.isotonic_eval(3, 20)
    assert digest() == before_eval                 # the live flat vector is put back, bit for bit
    text = capsys.readouterr().out
    assert "Isotonic recalibration" in text and text.count(" MCB ") == 10
    print(text[text.index("Isotonic recalibration"):])
