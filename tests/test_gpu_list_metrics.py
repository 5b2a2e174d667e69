"""What top-K lists are made of, on the device: mamdr_id_counts against np.bincount, mamdr_list_similarity against the float64
host definition on the same fp32 rows (mamdr_amd/list_metrics.py), and `list_metrics.report` / `run.py --list-metrics` end to
end on the small Taobao-shaped problem of tests/test_gpu_recommend.py (synthetic "taobao10", seed 7, scale 0.05: 1,188 users,
346 items, 10 domains).

The similarity's bar is derived, not tuned: |sim_sum - host| <= pairs * (2 E + 8) * 2^-24 (list_metrics.error_bound: the
fp32 fma chain of E terms, the two IEEE square roots and the two IEEE divisions).  One process, nothing that provokes a fault,
no sanitizer, no assembly scan.
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import _lib                      # noqa: E402
from mamdr_amd import list_metrics as lm        # noqa: E402
from test_gpu_recommend import gen, state_digest        # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def id_counts(ids, n_bins, label=None):
    """mamdr_id_counts through ctypes -> uint32 [n_bins]; the output starts as garbage: the call zeroes it."""
    lib = _lib.load()
    n = int(ids.size)
    d_ids = dev(ids.astype(np.int32)) if n else None
    d_label = dev(label.astype(F32)) if (label is not None and n) else None
    out = torch.full((n_bins,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.mamdr_id_counts(ptr(d_ids), ptr(d_label), n, n_bins, ptr(out), stream()))
    return out.cpu().numpy().view(np.uint32)


def list_similarity(ids, d_rows):
    """mamdr_list_similarity through ctypes -> (sim_sum float64 [Q], pairs int32 [Q])."""
    lib = _lib.load()
    ids = np.ascontiguousarray(ids, np.int32)
    Q, K = ids.shape
    d_ids = dev(ids)
    sim = torch.full((Q,), float("nan"), dtype=torch.float64, device="cuda")
    pairs = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.mamdr_list_similarity(ptr(d_ids), Q, K, ptr(d_rows), int(d_rows.shape[0]), int(d_rows.shape[1]), ptr(sim),
                                         ptr(pairs), stream()))
    return sim.cpu().numpy(), pairs.cpu().numpy()


# ------------------------------------------------------------------ mamdr_id_counts
def test_id_counts_equal_bincount():
    need_gpu()
    rs = np.random.RandomState(3)
    for n in (0, 1, 63, 64, 65, 100003):
        for n_bins in (1, 7, 4097):
            ids = rs.randint(0, n_bins, n).astype(np.int64)
            # ids that count nowhere, mixed in: -1, n_bins and INT32_MAX
            foreign = rs.rand(n) < 0.15
            ids[foreign] = rs.choice([-1, n_bins, INT32_MAX], int(foreign.sum()))
            valid = ids[(ids >= 0) & (ids < n_bins)]
            want = np.bincount(valid, minlength=n_bins).astype(np.uint32)
            got = id_counts(ids, n_bins)
            assert got.tobytes() == want.tobytes(), (n, n_bins)
            assert got.tobytes() == lm.id_counts_host(ids, n_bins).astype(np.uint32).tobytes()
            # with a label column: -0.0 equals 0, 0.5 does not
            label = rs.choice(np.array([0.0, -0.0, 0.5, 1.0], F32), n)
            keep = (ids >= 0) & (ids < n_bins) & (label != 0)
            want = np.bincount(ids[keep], minlength=n_bins).astype(np.uint32)
            got = id_counts(ids, n_bins, label)
            assert got.tobytes() == want.tobytes(), (n, n_bins, "label")
            assert id_counts(ids, n_bins, label).tobytes() == got.tobytes()        # two runs, the same bytes


def test_id_counts_worst_contention_and_2d_input():
    need_gpu()
    got = id_counts(np.full(100003, 5, np.int64), 7)
    assert got.tolist() == [0, 0, 0, 0, 0, 100003, 0]
    assert id_counts(np.full(100003, 5, np.int64), 7).tobytes() == got.tobytes()
    lists = np.array([[3, 1, -1], [3, -1, -1], [0, 3, 1]], np.int32)
    assert id_counts(lists.ravel(), 4).tolist() == [1, 2, 0, 3]


# ------------------------------------------------------------------ mamdr_list_similarity: exact cases
def one_hot_table(E):
    """48 signed power-of-two multiples of one-hot rows over 8 distinct columns, and row 48 all zeros: every cosine is
    exactly 0 or +-1."""
    rows = np.zeros((49, E), F32)
    for r in range(48):
        rows[r, (r % 8) * (E // 8) + 1] = (-1.0) ** (r // 3) * 2.0 ** (r % 5 - 2)
    return rows


EXACT_LISTS = [
    [0, 8, 16, 24, 3, 11, 1, 9],            # shared columns: +-1 among 0 / 8 / 16 / 24, 3 / 11 and 1 / 9
    [-1, -1, -1, -1, -1, -1, -1, -1],       # all padding
    [5, -1, 13, -1, -1, 21, 5, -1],         # padding in the middle, a duplicate
    [5, 49, 13, INT32_MAX, 21, 49, 5, 49],  # an id of n_rows (and a huge one) is padding
    [7, 7, 7, 7, 7, 7, 7, 7],               # duplicates only: 28 pairs of cosine 1
    [48, 0, 48, 8, 16, 48, 24, 32],         # the zero row: its pairs are exactly 0
    [40, -1, -1, -1, -1, -1, -1, -1],       # one valid entry: no pair
    [2, 10, 18, 26, 34, 42, 47, 39],
]


@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_list_similarity_exact_cases(E):
    need_gpu()
    rows = one_hot_table(E)
    d_rows = dev(rows)
    base = np.array(EXACT_LISTS, np.int32)
    seen = set()
    for K in (1, 8, 32, 33, 128):                   # both kernel variants; K = 1: pairs 0, sim_sum 0
        ids = np.full((base.shape[0], K), -1, np.int32)
        ids[:, :min(K, 8)] = base[:, :min(K, 8)]
        if K > 8:                                   # the tail: more entries behind a run of padding
            ids[:, K - 3:] = base[:, :3]
        want_sim, want_pairs = lm.list_similarity_host(ids, rows)
        sim, pairs = list_similarity(ids, d_rows)
        assert np.all(want_sim == np.round(want_sim))
        assert pairs.tobytes() == want_pairs.tobytes(), (E, K)
        assert sim.tobytes() == (want_sim + 0.0).tobytes(), (E, K, sim, want_sim)
        if K == 1:
            assert not pairs.any() and not sim.any()
        seen.update(sim.tolist())
    assert len(seen) > 4 and min(seen) < 0 < max(seen)      # the cases are not all zeros


# ------------------------------------------------------------------ mamdr_list_similarity: random cases
def random_table(E, n_rows=300, seed=0):
    rs = np.random.RandomState(100 + E + seed)
    return (rs.standard_normal((n_rows, E)) * 10.0 ** rs.uniform(-3, 3, (n_rows, 1))).astype(F32)


def ragged_lists(rs, Q, K, n_rows, scatter):
    """Q lists of K entries with valid lengths 0 .. K: list 0 is full and starts with one id twice (a pair of cosine 1: at
    least one list of every case carries a mean cosine far above the bound); the others draw their length, and their ids
    with replacement from a pool of min(L, 16) rows.  Padding (-1, n_rows, INT32_MAX) at the tail, or scattered."""
    ids = np.empty((Q, K), np.int32)
    for q in range(Q):
        L = K if q == 0 else rs.randint(0, K + 1)
        pool = rs.choice(n_rows, max(1, min(L, 16)), replace=False)
        vals = rs.choice(pool, L)
        if q == 0:
            vals[1] = vals[0]
        row = rs.choice(np.array([-1, n_rows, INT32_MAX], np.int64), K)
        where = np.sort(rs.choice(K, L, replace=False)) if scatter else np.arange(L)
        row[where] = vals
        ids[q] = row
    return ids


@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_list_similarity_within_the_derived_bound(E):
    need_gpu()
    rows = random_table(E)
    d_rows = dev(rows)
    bound = lm.error_bound(E)
    assert bound == (2 * E + 8) * 2.0 ** -24
    rs = np.random.RandomState(E)
    worst = 0.0
    for case, K in enumerate((2, 3, 16, 17, 32, 33, 64, 65, 100, 128)):
        for Q in (1, 5, 257):
            ids = ragged_lists(rs, Q, K, rows.shape[0], scatter=bool((case + Q) % 2))
            want_sim, want_pairs = lm.list_similarity_host(ids, rows)
            sim, pairs = list_similarity(ids, d_rows)
            assert pairs.tobytes() == want_pairs.tobytes(), (E, K, Q)
            err = np.abs(sim - want_sim)
            has = want_pairs > 0
            ratio = float((err[has] / (want_pairs[has] * bound)).max())
            worst = max(worst, ratio)
            print("E %3d K %3d Q %3d: worst |sim_sum - host| / (pairs * bound) = %.4f" % (E, K, Q, ratio))
            assert np.all(err <= want_pairs * bound), (E, K, Q, ratio)
            assert np.all(sim[~has] == 0.0)
            # the bound is useful: a kernel that returns zeros cannot pass
            assert float(np.abs(want_sim[has] / want_pairs[has]).max()) > 100.0 * bound, (E, K, Q)
    print("E %d: worst ratio to the bound %.4f" % (E, worst))


# ------------------------------------------------------------------ position and neighbours
def test_a_list_is_the_same_bits_wherever_it_sits():
    need_gpu()
    E, K = 64, 48
    rows = random_table(E, seed=1)
    d_rows = dev(rows)
    rs = np.random.RandomState(17)
    mine = ragged_lists(rs, 64, K, rows.shape[0], scatter=True)
    alone = list_similarity(mine, d_rows)
    again = list_similarity(mine, d_rows)
    assert alone[0].tobytes() == again[0].tobytes() and alone[1].tobytes() == again[1].tobytes()
    rev = list_similarity(mine[::-1], d_rows)
    assert rev[0][::-1].tobytes() == alone[0].tobytes() and rev[1][::-1].tobytes() == alone[1].tobytes()
    others = ragged_lists(rs, 200, K, rows.shape[0], scatter=False)
    where = np.sort(rs.choice(264, 64, replace=False))
    mixed = np.empty((264, K), np.int32)
    mixed[where] = mine
    mixed[np.setdiff1d(np.arange(264), where)] = others
    emb = list_similarity(mixed, d_rows)
    assert emb[0][where].tobytes() == alone[0].tobytes() and emb[1][where].tobytes() == alone[1].tobytes()
    assert alone[1].max() == K * (K - 1) // 2 and np.abs(alone[0]).max() > 0
    # the valid entries alone decide: the same entries with their padding elsewhere, in a shorter or a longer call
    short = ragged_lists(rs, 40, 20, rows.shape[0], scatter=False)
    a = list_similarity(short, d_rows)
    for K2 in (32, 33, 128):
        wide = np.full((40, K2), -1, np.int32)
        for q in range(40):
            valid = short[q][(short[q] >= 0) & (short[q] < rows.shape[0])]
            wide[q, np.sort(rs.choice(K2, valid.size, replace=False))] = valid
        b = list_similarity(wide, d_rows)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), K2


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    need_gpu()
    lib = _lib.load()
    d_rows = dev(random_table(32, n_rows=8))
    d_wide = dev(np.zeros((8, 96), F32))
    ids = dev(np.zeros((4, 128), np.int32))
    sim = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    pairs = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    call = lambda n_list, k, rows, n_rows, emb: lib.mamdr_list_similarity(    # noqa: E731
        ptr(ids), n_list, k, rows, n_rows, emb, ptr(sim), ptr(pairs), stream())
    for args, word in (((4, 0, ptr(d_rows), 8, 32), b"k 0"), ((4, 129, ptr(d_rows), 8, 32), b"k 129"),
                       ((4, 2, ptr(d_wide), 8, 96), b"emb_dim 96"), ((0, 2, ptr(d_rows), 8, 32), b"n_list"),
                       ((4, 2, C.c_void_p(d_rows.data_ptr() + 4), 7, 32), b"aligned"), ((4, 2, ptr(d_rows), 0, 32), b"n_rows")):
        assert call(*args) == _lib.EINVAL, word
        assert word in lib.mamdr_last_error(), lib.mamdr_last_error()
    torch.cuda.synchronize()
    assert sim.cpu().tolist() == [7.0] * 4 and pairs.cpu().tolist() == [7] * 4         # nothing was written
    assert lib.mamdr_id_counts(ptr(ids), None, 4, 0, ptr(pairs), stream()) == _lib.EINVAL
    assert lib.mamdr_id_counts(C.c_void_p(ids.data_ptr() + 2), None, 4, 4, ptr(pairs), stream()) == _lib.EINVAL
    assert pairs.cpu().tolist() == [7] * 4


# ------------------------------------------------------------------ end to end
def small_config(tmp_path, name, trainable):
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name)
    cfg["train"].update(epoch=1, patience=1, sample_num=2, meta_learning_rate=0.5, emb_trainable=trainable,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.05, synthetic_seed=7)        # test_gpu_recommend.gen()'s problem
    return cfg


@pytest.mark.parametrize("name,trainable", [("mlp", False), ("deepfm", True)], ids=["mlp-frozen", "deepfm-trainable"])
def test_report_equals_the_host_route(tmp_path, capsys, name, trainable):
    need_gpu()
    from mamdr_amd import cli, engine
    from mamdr_amd.utils import MultiDomainDataset
    cfg = small_config(tmp_path, name, trainable)
    model = cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    eng = model.model
    g = gen()
    assert isinstance(eng, engine.TowerEngine) and (eng.n_user, eng.n_item, eng.n_domain) == (g["n_user"], g["n_item"], 10)
    assert eng.emb_trainable == trainable
    # a few Adam steps first: with trainable tables the rows no batch touched are advanced lazily, and item_rows() must hand
    # out current ones
    d_big = max(range(10), key=lambda i: eng.n_rows(i, "train"))
    eng.train_steps(d_big, n_steps=3, lr=1e-2)
    before = state_digest(eng)
    view = eng.item_rows()
    assert view.shape == (346, 128) and view.is_cuda and view.data_ptr() % 16 == 0
    rows = view.cpu().numpy().copy()
    if trainable:
        assert rows.tobytes() == eng.unpack(eng.get_weights())["item_emb"].tobytes()
        assert view.data_ptr() == eng._weights.data_ptr() + 4 * eng.segments["item_emb"][0]        # a view, not a copy
    else:
        assert view.data_ptr() == eng.tables["item_emb"].data_ptr()
    out = str(tmp_path / "lm.npz")
    path, reports = lm.report(model, 10, out)
    assert path == out and sorted(reports) == list(range(10))
    assert state_digest(eng) == before                      # weights, Adam slots, counters: the report reads state only
    bound = lm.error_bound(128)
    ds = model.dataset
    with np.load(out) as z:
        assert z["domains"].tolist() == list(range(10)) and int(z["k"]) == 10
        for d in range(10):
            r = model.list_eval(d, 10)
            ids = r["ids"]
            assert ids.tobytes() == model.recommend(d, 10)["ids"].tobytes()
            tr = ds.train_dataset[d]["data"]
            expo = lm.id_counts_host(ids, 346)
            pop = lm.id_counts_host(tr["pid"], 346, tr["label"])
            assert r["exposure"].tolist() == expo.tolist() and r["popularity"].tolist() == pop.tolist()
            sim, pairs = lm.list_similarity_host(ids, rows)
            assert r["pairs"].tolist() == pairs.tolist()
            assert np.all(np.abs(r["sim_sum"] - sim) <= pairs * bound)
            cat = np.unique(np.concatenate([s[d]["data"]["pid"] for s in (ds.train_dataset, ds.val_dataset, ds.test_dataset)]))
            assert np.array_equal(z["catalogue_%d" % d], cat)
            assert np.array_equal(z["exposure_%d" % d], expo[cat]) and np.array_equal(z["popularity_%d" % d], pop[cat])
            assert np.array_equal(z["pairs_%d" % d], pairs) and z["sim_sum_%d" % d].tobytes() == r["sim_sum"].tobytes()
            n_lists = int((ids >= 0).any(axis=1).sum())
            want = lm.summarise(expo, pop, cat, 10, sim, pairs, n_lists=n_lists)
            got = reports[d]
            for key in lm.FIGURES[:-1] + ("n_ild", "n_lists", "n_items", "n_shown"):
                assert got[key] == want[key], (d, key)              # integers in, the same float64 out
                if key in z.files:
                    assert z[key][d] == want[key]
            assert abs(got["ild"] - want["ild"]) <= bound and z["ild"][d] == got["ild"]
            assert got["n_ild"] > 0 and 0.0 < got["coverage"] <= 1.0
    assert state_digest(eng) == before
    text = capsys.readouterr().out
    assert "List metrics top-10" in text and text.count("Coverage@10") == 10
    print(text[text.index("List metrics top-10"):])
    eng.close()


def test_run_config_with_list_metrics(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 MAMDR config, shrunk, with train.list_metrics: the .npz and the result.json
    keys exist, and every domain's lists were scored -- and its item table read -- under that domain's own merged weights,
    with the live flat vector put back afterwards."""
    need_gpu()
    from mamdr_amd import cli, engine
    cfg = small_config(tmp_path, "mlp_meta_mamdr", False)
    cfg["train"].update(list_metrics=10)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    eng = model.model
    assert isinstance(eng, engine.TowerEngine)
    rdir = [os.path.join(model.result_path, f) for f in os.listdir(model.result_path) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    for key in lm.FIGURES:
        assert sorted(result["domain_" + key]) == sorted(str(d) for d in range(10)), key
    for key in lm.AVERAGED:
        assert np.isfinite(result["avg_" + key])
    before = state_digest(eng)
    keep = eng.get_weights().clone()
    rows = eng.item_rows().cpu().numpy()
    with np.load(os.path.join(model.result_path, "list_metrics_top10.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and int(z["k"]) == 10
        for d in range(10):
            merged = eng.new_vector(meta=True)
            eng.merge(merged, model.best_shared_weights, model.best_domain_weights[d], cfg["train"]["merged_method"])
            eng.assign_meta(merged)
            ids = model.base_model.recommend(d, 10)["ids"]            # the domain's own weights, installed by hand
            eng.set_weights(keep)
            cat = z["catalogue_%d" % d]
            assert np.array_equal(z["exposure_%d" % d], lm.id_counts_host(ids, 346)[cat])
            sim, pairs = lm.list_similarity_host(ids, rows)
            assert np.array_equal(z["pairs_%d" % d], pairs)
            assert np.all(np.abs(z["sim_sum_%d" % d] - sim) <= pairs * lm.error_bound(128))
            assert result["domain_coverage"][str(d)] == float(z["coverage"][d])
        assert result["avg_ild"] == pytest.approx(float(np.mean(z["ild"])))
    assert state_digest(eng) == before
    model.list_eval(3, 10)
    assert state_digest(eng) == before                 # the live flat vector is put back, bit for bit
    text = capsys.readouterr().out
    assert "List metrics top-10" in text and text.count("Coverage@10") == 10
    print(text[text.index("List metrics top-10"):])
