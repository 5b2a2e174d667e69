"""Domain-conflict report, host side (no GPU): `conflict.cosines` / `summary` on hand-made Gram matrices, `conflict.report`
over a small numpy stand-in of the engine, `run.py --conflict`, the lanes / multi-process refusal and the C ABI's
declaration and binding of mamdr_gram / mamdr_gram_work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gauc_host as gh          # tiny_config, patch_emb_dim
from fake_engine import FakeEngine
from mamdr_amd import _lib, cli, conflict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ cosines / summary
def test_orthogonal_pair():
    cos = conflict.cosines(np.array([[4.0, 0.0], [0.0, 9.0]]))
    assert cos.tolist() == [[1.0, 0.0], [0.0, 1.0]]
    m = conflict.summary(cos)
    assert m == {"conflict_rate": 0.0, "mean_cosine": 0.0, "min_cosine": 0.0, "min_pair": (0, 1), "n_pairs": 1}


def test_opposite_pair_conflicts():
    v = np.array([[1.0, 2.0, -3.0], [-2.0, -4.0, 6.0]])
    cos = conflict.cosines(v @ v.T)
    assert cos.tolist() == [[1.0, -1.0], [-1.0, 1.0]]
    m = conflict.summary(cos)
    assert m["conflict_rate"] == 1.0 and m["mean_cosine"] == -1.0 and m["min_cosine"] == -1.0 and m["min_pair"] == (0, 1)


def test_zero_vector_is_nan_and_leaves_the_pairs():
    v = np.array([[3.0, 4.0], [0.0, 0.0], [-4.0, 3.0], [-3.0, -4.0]])
    cos = conflict.cosines(v @ v.T)
    assert np.all(np.isnan(cos[1])) and np.all(np.isnan(cos[:, 1]))          # off the diagonal and on it
    live = [0, 2, 3]
    assert np.array_equal(cos[np.ix_(live, live)], np.array([[1.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 1.0]]))
    m = conflict.summary(cos)
    assert m["n_pairs"] == 3 and m["conflict_rate"] == 1.0 / 3 and m["min_cosine"] == -1.0 and m["min_pair"] == (0, 3)
    assert m["mean_cosine"] == -1.0 / 3


def test_one_domain_has_no_pairs():
    cos = conflict.cosines(np.array([[2.5]]))
    assert cos.tolist() == [[1.0]]
    m = conflict.summary(cos)
    assert m["n_pairs"] == 0 and m["conflict_rate"] == 0.0 and np.isnan(m["mean_cosine"]) and m["min_pair"] is None


def test_cosines_are_symmetric_with_a_unit_diagonal():
    rs = np.random.RandomState(0)
    v = rs.standard_normal((7, 50)) * np.exp(rs.uniform(-20, 20, (7, 1)))
    g = np.stack([v @ v.T, (v[:, :9] @ v[:, :9].T)])
    cos = conflict.cosines(g)
    assert cos.shape == (2, 7, 7)
    assert np.array_equal(cos, np.swapaxes(cos, 1, 2)) and np.all(np.diagonal(cos, axis1=1, axis2=2) == 1.0)
    assert np.all(np.abs(cos) <= 1.0 + 1e-12)


# ------------------------------------------------------------------ report over a numpy stand-in
class StandInEngine(object):
    """what conflict.measure asks of an engine, in numpy: three tensors in a flat vector of 23 floats, the meta range
    [4, 19); domain d's batch gradients are integer vectors, so every sum and product below is exact."""
    n_params, meta_off, n_meta = 23, 4, 15
    segments = {"emb": (0, 8), "W": (8, 12), "b": (20, 3)}
    passes = {0: 5, 1: 2, 2: 0, 3: 7}                       # batches of a whole pass; domain 2 has no rows

    def __init__(self):
        rs = np.random.RandomState(4)
        self.mean = {d: rs.randint(-6, 7, self.n_params).astype(np.float32) for d in self.passes}
        self.mean[3][8:20] = -self.mean[0][8:20]            # tensor W: domains 0 and 3 are opposite
        self.calls = []

    def domain_gradients(self, domains, n_batches=None, out=None):
        self.calls.append((list(domains), n_batches))
        steps = np.array([self.passes[d] if n_batches is None else min(n_batches, self.passes[d]) for d in domains], np.int64)
        return np.stack([self.mean[d] * np.float32(s) for d, s in zip(domains, steps)]), steps

    def gram(self, vecs, ranges):
        v = np.asarray(vecs, np.float64)
        return np.stack([v[:, o:o + c] @ v[:, o:o + c].T for o, c in ranges])


class StandInModel(object):
    def __init__(self, tmp_path):
        self.model = StandInEngine()
        self.result_path = str(tmp_path / "result")

    def domain_conflict(self, n_batches=None):
        return conflict.measure(self.model, [0, 1, 2, 3], n_batches)


@pytest.mark.parametrize("n_batches,steps", [(3, [3, 2, 0, 3]), (0, [5, 2, 0, 7])])
def test_report_on_a_numpy_stand_in(tmp_path, capsys, n_batches, steps):
    model = StandInModel(tmp_path)
    eng = model.model
    path, res = conflict.report(model, n_batches)
    assert path == os.path.join(model.result_path, "domain_conflict.npz") and os.path.exists(path)
    assert eng.calls == [([0, 1, 2, 3], n_batches or None)]             # 0 means whole passes
    names = ["all", "meta", "emb", "W", "b"]
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["domains", "steps", "ranges", "offsets", "counts", "gram", "cosine", "norm",
                                          "conflict_rate", "mean_cosine"])
        assert z["domains"].tolist() == [0, 1, 2, 3] and z["steps"].tolist() == steps
        assert z["ranges"].tolist() == names
        assert z["offsets"].tolist() == [0, 4, 0, 8, 20] and z["counts"].tolist() == [23, 15, 8, 12, 3]
        assert z["gram"].shape == z["cosine"].shape == (5, 4, 4) and z["gram"].dtype == z["cosine"].dtype == np.float64
        assert z["norm"].shape == (5, 4) and z["conflict_rate"].shape == z["mean_cosine"].shape == (5,)
        mean = np.stack([eng.mean[d] if s else np.zeros(23, np.float32) for d, s in zip(range(4), steps)]).astype(np.float64)
        for r, (o, c) in enumerate(zip(z["offsets"], z["counts"])):
            want = mean[:, o:o + c] @ mean[:, o:o + c].T
            assert np.array_equal(z["gram"][r], want), names[r]         # the summed gradients' Gram over steps_i * steps_j
            assert np.array_equal(z["norm"][r], np.sqrt(np.diag(want)))
            cos = z["cosine"][r]
            assert np.array_equal(cos, cos.T, equal_nan=True)
            live = z["norm"][r] > 0
            assert np.all(np.diag(cos)[live] == 1.0) and np.all(np.isnan(cos[~live])) and not live[2]
            m = conflict.summary(cos)
            assert z["conflict_rate"][r] == m["conflict_rate"] and z["mean_cosine"][r] == m["mean_cosine"]
            assert m["n_pairs"] == 3                                     # domain 2 has no gradient: out of every pair
        assert z["cosine"][3][0, 3] == -1.0 and z["conflict_rate"][3] >= 1.0 / 3
    head = conflict.headline(res)
    assert sorted(head) == ["conflict_rate_all", "conflict_rate_meta", "mean_cosine_all", "mean_cosine_meta"]
    assert head["conflict_rate_meta"] == res["conflict_rate"][1] and head["mean_cosine_all"] == res["mean_cosine"][0]
    text = capsys.readouterr().out
    assert "Domain conflict" in text and text.count("ConflictRate") == 5 and "domain_conflict.npz" in text
    for name in names:
        assert ("\n%s: ConflictRate" % name) in text


def test_report_writes_where_it_is_told(tmp_path):
    out = str(tmp_path / "elsewhere" / "c.npz")
    path, _ = conflict.report(StandInModel(tmp_path), 2, out)
    assert path == out and os.path.exists(out)


# ------------------------------------------------------------------ the command line
def test_cli_flag_sets_train_conflict(monkeypatch):
    seen = []
    monkeypatch.setattr(cli, "main", lambda *a, **k: seen.append((a, k)))
    cfg_path = os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")
    cli.cli(["--config", cfg_path])
    cli.cli(["--config", cfg_path, "--conflict"])
    cli.cli(["--config", cfg_path, "--conflict", "0"])
    cli.cli(["--config", cfg_path, "--conflict", "3", "--conflict-out", "x.npz", "--recommend", "10"])
    assert "conflict" not in seen[0][0][0]["train"] and "conflict_out" not in seen[0][0][0]["train"]
    assert seen[1][1] == {} and seen[1][0][0]["train"]["conflict"] == 8 == conflict.DEFAULT_BATCHES
    assert seen[2][0][0]["train"]["conflict"] == 0
    assert seen[3][1] == {"recommend": 10, "recommend_out": None}
    assert seen[3][0][0]["train"]["conflict"] == 3 and seen[3][0][0]["train"]["conflict_out"] == "x.npz"
    with pytest.raises(SystemExit):
        cli.cli(["--config", cfg_path, "--conflict", "-1"])


@pytest.mark.parametrize("how", ["lanes", "processes"])
@pytest.mark.parametrize("n", [8, 0])
def test_lanes_and_processes_refuse_conflict_by_name(tmp_path, monkeypatch, how, n):
    gh.patch_emb_dim(monkeypatch)
    loaded = []
    from mamdr_amd import utils
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    if how == "lanes":
        cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", conflict=n, lanes=2)
    else:
        cfg = gh.tiny_config(tmp_path, "mlp_meta_mamdr", conflict=n)
        monkeypatch.setattr(cli, "init_distributed", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match=r"train\.conflict"):
        cli.main(cfg, FakeEngine)
    assert not loaded                    # refused before the data is loaded


# ------------------------------------------------------------------ C ABI
def test_gram_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+mamdr_gram\s*\(([^;]*)\)\s*;", bare)
    assert m, "mamdr_gram is not declared in include/mamdr_hip.h"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "const float* d_vecs", "int64_t stride", "int32_t n_vec", "int64_t n_cols", "const int64_t* h_off",
        "const int64_t* h_count", "int32_t n_range", "double* d_work", "int64_t work_doubles", "double* d_out", "void* stream"]
    m = re.search(r"\bint64_t\s+mamdr_gram_work\s*\(([^;]*)\)\s*;", bare)
    assert m, "mamdr_gram_work is not declared in include/mamdr_hip.h"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "int32_t n_vec", "const int64_t* h_off", "const int64_t* h_count", "int32_t n_range"]
    doc = header[:header.index("int64_t mamdr_gram_work")].rsplit("/*", 1)[1]
    assert "NO REFERENCE COUNTERPART" in doc and "ascending slab order" in doc and "No floating-point atomics" in doc
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_gram_work"] == (i64, [i32, vp, vp, i32])
    assert _lib.SIGNATURES["mamdr_gram"] == (C.c_int, [vp, i64, i32, i64, vp, vp, i32, vp, i64, vp, vp])
    assert _lib.GRAM_SLAB == int(re.search(r"#define\s+MAMDR_GRAM_SLAB\s+(\d+)", header).group(1))
    assert _lib.GRAM_MAX_VEC == int(re.search(r"#define\s+MAMDR_GRAM_MAX_VEC\s+(\d+)", header).group(1)) == 32
    assert _lib.ABI_VERSION == 19 and re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)
    lib = _lib.load()
    assert hasattr(lib, "mamdr_gram") and hasattr(lib, "mamdr_gram_work")


def test_gram_work_and_refusals_need_no_device():
    """the workspace size is host arithmetic, and every refusal comes before any HIP call."""
    lib = _lib.load()
    S = _lib.GRAM_SLAB
    arr = lambda *v: (C.c_int64 * len(v))(*v)      # noqa: E731
    assert lib.mamdr_gram_work(5, arr(0, 3, 1), arr(0, S, 2 * S + 7), 3) == (0 + 1 + 3) * 25
    assert lib.mamdr_gram_work(32, arr(7), arr(S + 1), 1) == 2 * 1024
    assert lib.mamdr_gram_work(1, None, None, 0) == 0
    for n_vec in (0, 33):
        assert lib.mamdr_gram_work(n_vec, arr(0), arr(4), 1) == _lib.EINVAL
        assert b"n_vec" in lib.mamdr_last_error()
    assert lib.mamdr_gram_work(2, arr(0), arr(-1), 1) == _lib.EINVAL and b"h_count" in lib.mamdr_last_error()
    assert lib.mamdr_gram_work(2, arr(-1), arr(1), 1) == _lib.EINVAL and b"h_off" in lib.mamdr_last_error()
    # mamdr_gram: a host address stands in for the device pointers -- nothing is launched, nothing dereferenced
    fake = C.c_void_p(4096)
    assert lib.mamdr_gram(fake, 10, 0, 10, arr(0), arr(4), 1, fake, 1 << 20, fake, None) == _lib.EINVAL
    assert b"n_vec" in lib.mamdr_last_error()
    assert lib.mamdr_gram(fake, 10, 2, 10, arr(8), arr(3), 1, fake, 1 << 20, fake, None) == _lib.EINVAL
    assert b"range 0" in lib.mamdr_last_error()
    assert lib.mamdr_gram(fake, 9, 2, 10, arr(0), arr(3), 1, fake, 1 << 20, fake, None) == _lib.EINVAL
    assert b"stride" in lib.mamdr_last_error()
    assert lib.mamdr_gram(fake, 10, 2, 10, arr(0), arr(3), 1, fake, 3, fake, None) == _lib.EINVAL
    assert b"work_doubles" in lib.mamdr_last_error()
    assert lib.mamdr_gram(fake, 10, 2, 10, arr(0), arr(3), 1, fake, 4, C.c_void_p(4100), None) == _lib.EINVAL
    assert b"d_out" in lib.mamdr_last_error()
    assert lib.mamdr_gram(None, 10, 2, 10, arr(0), arr(3), 1, fake, 4, fake, None) == _lib.EINVAL
    assert b"d_vecs" in lib.mamdr_last_error()
