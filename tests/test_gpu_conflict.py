"""Domain-conflict report on the device: mamdr_gram (FlatVectorOps.gram) against numpy, `domain_gradients` against the
manual accumulate route on tests/test_gpu_recommend.py's problem (1,188 users, 346 items, 10 domains, batch 256), its state
contract on twin engines, and run.py --conflict end to end.

S = _lib.GRAM_SLAB columns per slab; every range length around it is covered, at every offset modulo 4.

Bound 2 (random data): |G - G_ref| <= 2 * n * 2^-53 * (|V| @ |V|^T) elementwise against numpy's fp64 Gram -- the standard
bound n * u * sum |a_k b_k| of a sum of n exact products under any order of additions (u = 2^-53), doubled for numpy's own
error of the same kind.
"""
import copy
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_recommend as base           # noqa: E402  (the problem, the mlp / deepfm engines, their digest)
import test_gpu_recommend_star as sbase     # noqa: E402  (the Star engine and its digest)

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def ops():
    """FlatVectorOps without an engine behind it: the library, the current stream."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import _lib
    from mamdr_amd.engine import FlatVectorOps
    o = FlatVectorOps()
    o.lib, o.stream = _lib.load(), torch.cuda.current_stream()
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def slab():
    from mamdr_amd import _lib
    return _lib.GRAM_SLAB


# ---------------------------------------------------------------------------------------------------------------- 1
def integer_ranges():
    S = slab()
    ranges = [(o, n) for n in (1, 3, 4, 5, S - 1, S, S + 1, 2 * S + 7) for o in (0, 1, 2, 3)]
    n_cols = 3 + 2 * S + 7
    ranges += [(5, 0), (0, n_cols)]                                     # an empty one, "all"
    part = [(0, 5), (5, S), (5 + S, n_cols - 5 - S)]                    # a partition of "all"
    return n_cols, ranges, part


@pytest.mark.parametrize("n_vec", [1, 2, 5, 30, 32])
def test_exact_on_integers(n_vec):
    o = ops()
    n_cols, ranges, part = integer_ranges()
    V = np.random.RandomState(n_vec).randint(-8, 9, (n_vec, n_cols)).astype(F32)
    got = o.gram(dev(V), ranges + part).cpu().numpy()
    assert got.shape == (len(ranges) + 3, n_vec, n_vec) and got.dtype == np.float64
    Vi = V.astype(np.int64)
    for r, (off, cnt) in enumerate(ranges + part):
        want = Vi[:, off:off + cnt] @ Vi[:, off:off + cnt].T
        assert got[r].tobytes() == want.astype(np.float64).tobytes(), (n_vec, off, cnt)
        assert got[r].tobytes() == np.ascontiguousarray(got[r].T).tobytes()
    assert not got[len(ranges) - 2].any()                               # the empty range: zeros
    assert np.array_equal(got[len(ranges) - 1], got[len(ranges):].sum(axis=0))      # "all" = the partition's sum, exactly


# ---------------------------------------------------------------------------------------------------------------- 2
def test_random_data_within_the_summation_bound():
    o = ops()
    S = slab()
    n, D = 2 * S + 7, 30
    rs = np.random.RandomState(2)
    V = (rs.standard_normal((D, n)) * np.exp(rs.uniform(-12, 12, (D, n)))).astype(F32)      # mixed magnitudes
    got = o.gram(dev(V), [(0, n)]).cpu().numpy()[0]
    V64 = V.astype(np.float64)
    ref = V64 @ V64.T
    bound = 2 * n * U * (np.abs(V64) @ np.abs(V64).T)
    err = np.abs(got - ref)
    print("worst |G - G_ref| / bound = %.3e (bound 2 n u |V| |V|^T, n = %d)" % ((err / bound).max(), n))
    assert np.all(err <= bound)
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("D", [5, 30])
def test_layout_independence(D):
    o = ops()
    S = slab()
    n = S + 77
    rs = np.random.RandomState(3)
    V = (rs.standard_normal((D, n)) * np.exp(rs.uniform(-6, 6, (D, n)))).astype(F32)
    ranges = [(0, n), (3, S + 1), (S - 5, 40), (1, 2)]
    tight = dev(V)
    first = o.gram(tight, ranges).cpu().numpy()
    assert first.tobytes() == o.gram(tight, ranges).cpu().numpy().tobytes()             # repeated
    stride = n + 5
    for shift in (0, 1):                                                                 # a wider stride; the block one float on
        buf = torch.full((D * stride + 8,), 7.0, dtype=torch.float32, device="cuda")
        view = buf[shift:shift + D * stride].view(D, stride)[:, :n]
        view.copy_(tight)
        assert view.data_ptr() % 16 == 4 * shift and view.stride(0) == stride
        assert o.gram(view, ranges).cpu().numpy().tobytes() == first.tobytes(), shift
    for r, rng in enumerate(ranges):                                                     # alone = inside the overlapping request
        assert o.gram(tight, [rng]).cpu().numpy()[0].tobytes() == first[r].tobytes(), rng
    # one nan poisons exactly its vector's row and column of the ranges that hold it
    row, col = D - 1, 10
    W = V.copy()
    W[row, col] = np.nan
    got = o.gram(dev(W), ranges).cpu().numpy()
    for r, (off, cnt) in enumerate(ranges):
        bad = np.isnan(got[r])
        want = np.zeros((D, D), bool)
        if off <= col < off + cnt:
            want[row, :] = want[:, row] = True
        assert np.array_equal(bad, want), (off, cnt)
        assert got[r][~want].tobytes() == first[r][~want].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_refusals():
    o = ops()
    from mamdr_amd import _lib
    lib = o.lib
    S = slab()
    n = S + 9
    V = dev(np.ones((2, n), F32))
    out = torch.full((2 * 4 + 1,), -7.0, dtype=torch.float64, device="cuda")
    work = torch.zeros(2 * 4 + 1, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    arr = lambda *v: (C.c_int64 * len(v))(*v)    # noqa: E731
    assert lib.mamdr_gram_work(2, arr(0), arr(n), 1) == 8
    call = lambda n_vec=2, off=0, cnt=n, w=work, wd=8, dst=None: lib.mamdr_gram(      # noqa: E731
        p(V), n, n_vec, n, arr(off), arr(cnt), 1, p(w), wd, dst if dst is not None else p(out), None)
    for kw, word in ((dict(n_vec=0), b"n_vec"), (dict(n_vec=33), b"n_vec"), (dict(off=10, cnt=n - 9), b"range 0"),
                     (dict(cnt=-1), b"h_count"), (dict(wd=7), b"work_doubles"),
                     (dict(dst=C.c_void_p(out.data_ptr() + 4)), b"d_out")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.mamdr_last_error(), (kw, lib.mamdr_last_error())
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7.0] * 9                              # untouched: nothing was launched
    assert call() == _lib.OK
    assert out.cpu().tolist() == [float(n)] * 4 + [-7.0] * 5
    with pytest.raises(ValueError):
        o.gram(V, [(0, n + 1)])
    with pytest.raises(ValueError):
        o.gram(dev(np.ones((33, 4), F32)), [(0, 4)])


# ---------------------------------------------------------------------------------------------------------------- 5
N_STEPS = 3
DOMAINS = (4, 0, 9)


def make_graph_engine(bind):
    """GraphEngine mlp (hidden [128, 64]), frozen tables, random weights (tests/test_gpu_gauc.py's recipe)."""
    from mamdr_amd import graph_engine
    g = base.gen()
    eng = graph_engine.GraphEngine("mlp", g["n_user"], g["n_item"], g["n_domain"], 256, (128, 64), (), dropout=0.5)
    eng.bind_table("user_emb", g["tables"]["user_emb"])
    eng.bind_table("item_emb", g["tables"]["item_emb"])
    for d in bind:
        c = g["data"]["train"][d]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    rs = np.random.RandomState(7)
    named = {n: (rs.standard_normal(cnt) * 0.08).astype(F32) for n, (off, cnt) in eng.segments.items()}
    eng.set_weights(eng.pack(named))
    return eng


def make(which, bind):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if which == "mlp-frozen":
        return base.make_engine("mlp", False, bind=bind)[0]
    if which == "deepfm-trainable":
        return base.make_engine("deepfm", True, bind=bind)[0]
    if which == "star":
        return sbase.make_star_engine(True, bind=bind)[0]
    return make_graph_engine(bind)


def manual_rows(eng, domains, n_steps):
    """the route domain_gradients stands for: a zeroed vector, bind_accumulator, accumulate steps."""
    rows = []
    for d in domains:
        total = -(-eng.n_rows(d, "train") // eng.batch_size)
        acc = eng.new_vector()
        eng.bind_accumulator(acc)
        eng.train_steps(d, optimizer="accumulate", n_steps=total if n_steps is None else min(n_steps, total))
        rows.append(acc.cpu().numpy())
    return np.stack(rows)


@pytest.mark.parametrize("which", ["mlp-frozen", "deepfm-trainable", "star", "graph-mlp"])
def test_domain_gradients_are_the_accumulate_steps(which):
    eng = make(which, DOMAINS)
    want = manual_rows(eng, DOMAINS, N_STEPS)
    rows, steps = eng.domain_gradients(DOMAINS, N_STEPS)
    passes = [-(-eng.n_rows(d, "train") // 256) for d in DOMAINS]
    assert tuple(rows.shape) == (3, eng.n_params) and rows.dtype == torch.float32
    assert steps.tolist() == [min(N_STEPS, n) for n in passes] and max(steps) == N_STEPS        # (a pass shorter than N ends the row)
    assert all(rows[j].data_ptr() % 16 == 0 for j in range(3))
    got = rows.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert np.abs(got).max() > 0 and len({got[j].tobytes() for j in range(3)}) == 3
    # the same buffer again, whole passes this time
    d = min(DOMAINS, key=lambda i: eng.n_rows(i, "train"))
    whole, steps = eng.domain_gradients([d], None, out=rows[:1])
    assert whole.data_ptr() == rows.data_ptr() and steps.tolist() == [-(-eng.n_rows(d, "train") // 256)]
    assert whole.cpu().numpy().tobytes() == manual_rows(eng, [d], None).tobytes()
    if which == "mlp-frozen":
        # plain sums even when a moving average is set, whose hidden state stays out of it
        eng.set_moving_average(0.999)
        keep = eng.new_vector()
        eng.bind_accumulator(keep)
        again, _ = eng.domain_gradients(DOMAINS, N_STEPS)
        assert again.cpu().numpy().tobytes() == want.tobytes()
        assert eng._ema["step"] == 0 and not eng._ema["biased"].any().item() and eng._acc is keep
    # the Gram of the rows as they stand now (a strided view), over the ranges the report asks for
    table = [(0, eng.n_params)] + [v for v in eng.segments.values()]
    G = eng.gram(rows, table).cpu().numpy()
    V = rows.cpu().numpy().astype(np.float64)
    for r, (off, cnt) in enumerate(table):
        ref = V[:, off:off + cnt] @ V[:, off:off + cnt].T
        assert np.all(np.abs(G[r] - ref) <= 2 * max(cnt, 1) * U * (np.abs(V[:, off:off + cnt]) @ np.abs(V[:, off:off + cnt]).T))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("which", ["deepfm-trainable", "star", "graph-mlp"])
def test_domain_gradients_leave_the_state_alone(which):
    """twin engines, the same Adam steps: a measures gradients between single-step, multi-step and mid-pass calls, b never
    does.  Weights, Adam slots, (aux,) both counters and the bound accumulator's content end equal."""
    import hashlib
    g = base.gen()
    sizes = [g["data"]["train"][i]["uid"].shape[0] for i in range(10)]
    d = max(range(10), key=lambda i: sizes[i])
    other = 3 if d != 3 else 0
    assert -(-sizes[d] // 256) >= 4
    a, b = make(which, (d, other)), make(which, (d, other))
    accs = []
    for e in (a, b):
        acc = e.new_vector()
        e.bind_accumulator(acc)
        e.train_steps(other, optimizer="accumulate", n_steps=1)
        e.train_steps(d, n_steps=2)
        accs.append(acc)

    def digest(e, acc):
        if which == "graph-mlp":
            h = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (e.weights, e.adam_m, e.adam_v)] + list(e.counters())
        else:
            h = (sbase if which == "star" else base).state_digest(e)
        return h + [hashlib.sha256(acc.cpu().numpy().tobytes()).hexdigest()]

    before = digest(a, accs[0])
    assert before == digest(b, accs[1])
    first = a.domain_gradients([other, d], 2)[0].cpu().numpy()
    assert digest(a, accs[0]) == before
    assert a.domain_gradients([other, d], 2)[0].cpu().numpy().tobytes() == first.tobytes()
    for first_step, n_steps in ((2, 1), (1, 2), (3, 1), (0, 3)):
        a.train_steps(d, first_step=first_step, n_steps=n_steps)
        a.domain_gradients([d, other], 1 if n_steps == 1 else None)
        b.train_steps(d, first_step=first_step, n_steps=n_steps)
    for e in (a, b):                                            # the bound accumulator is still the one accumulate steps add to
        e.train_steps(other, optimizer="accumulate", n_steps=1)
    assert digest(a, accs[0]) == digest(b, accs[1])
    assert digest(a, accs[0]) != before
    a.close()
    b.close()


def test_an_announced_window_survives_domain_gradients():
    """the step engine with frozen tables: two passes are announced (pregather), a measures gradients before they run, b
    does not.  The passes find their gathered rows on both (the digest counts the hits) and end in the same state."""
    g = base.gen()
    order = sorted(range(10), key=lambda i: -g["data"]["train"][i]["uid"].shape[0])
    d, other = order[0], order[1]
    a, b = make("mlp-frozen", (d, other)), make("mlp-frozen", (d, other))
    keep = []
    for e in (a, b):
        perms = [torch.from_numpy(np.random.RandomState(5 + i).permutation(e.n_rows(x, "train")).astype(np.int32)).to(e.device)
                 for i, x in enumerate((d, other))]
        keep.append(perms)
        e.pregather([(d, perms[0]), (other, perms[1])])
    before = base.state_digest(a)
    a.domain_gradients([other, d], 2)
    assert base.state_digest(a) == before
    for e, perms in zip((a, b), keep):
        e.train_steps(d, perm=perms[0])
        e.train_steps(other, perm=perms[1])
    da, db = base.state_digest(a), base.state_digest(b)
    print("pregather hits with / without domain_gradients in between: %d / %d" % (da[-1], db[-1]))
    assert da == db and da != before
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def run_config(tmp_path, name, **train):
    """tests/test_gpu_rank.py::run_config's run: the shipped Taobao-10 MAMDR config at a tenth of its size."""
    from mamdr_amd import cli
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name)
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"), **train)
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    return cfg, built[0]


def result_json(model):
    files = glob.glob(os.path.join(model.result_path, "*", "result.json"))
    assert len(files) == 1
    with open(files[0]) as f:
        return json.load(f)


def test_run_config_with_conflict(tmp_path, capsys):
    """run.py's entry with train.conflict = 2 under MAMDR: the .npz is complete, its "all" cosines are those of numpy's
    fp64 Gram of the engine's own gradient rows at the best theta, result.json carries the four scalars.  No quality bar.
    The cosine tolerance follows from bound 2 to first order: with dG_ab <= B_ab = 2 n u (|V| |V|^T)_ab and B_ii = 2 n u G_ii,
    d cos_ij <= B_ij / sqrt(G_ii G_jj) + |cos_ij| (B_ii / G_ii + B_jj / G_jj) / 2 <= 4 n u, plus 4 u for the division and
    the root."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import conflict, engine
    cfg, model = run_config(tmp_path, "mlp_meta_mamdr", conflict=2)
    eng = model.model
    assert isinstance(eng, engine.TowerEngine) and model.best_shared_weights is not None
    text = capsys.readouterr().out
    names = ["all", "meta"] + list(eng.segments)
    assert "Domain conflict" in text and text.count("ConflictRate") == len(names)
    R, n = len(names), eng.n_params
    with np.load(os.path.join(model.result_path, "domain_conflict.npz")) as z:
        assert sorted(z.files) == sorted(["domains", "steps", "ranges", "offsets", "counts", "gram", "cosine", "norm",
                                          "conflict_rate", "mean_cosine"])
        assert z["domains"].tolist() == list(range(10)) and z["ranges"].tolist() == names
        assert np.all((z["steps"] >= 1) & (z["steps"] <= 2))
        assert z["offsets"].tolist()[:2] == [0, eng.meta_off] and z["counts"].tolist()[:2] == [n, eng.n_meta]
        assert z["gram"].shape == z["cosine"].shape == (R, 10, 10) and z["norm"].shape == (R, 10)
        assert z["conflict_rate"].shape == z["mean_cosine"].shape == (R,)
        assert np.array_equal(z["cosine"], np.swapaxes(z["cosine"], 1, 2), equal_nan=True)
        cos_all, steps = z["cosine"][0], z["steps"]
        rate, mean = z["conflict_rate"], z["mean_cosine"]
    # the engine's own rows at the point the report measured: the best theta alone
    before = eng.get_weights().clone()
    model._set_model_meta_parms(model.best_shared_weights.clone())
    rows, steps2 = eng.domain_gradients(range(10), 2)
    eng.set_weights(before)
    assert steps2.tolist() == steps.tolist()
    V = rows.cpu().numpy().astype(np.float64) / steps[:, None]
    ref = conflict.cosines(V @ V.T)
    err = np.abs(cos_all - ref)
    print("cosines of \"all\" against numpy: worst error %.3e, tolerance %.3e" % (err.max(), (4 * n + 4) * U))
    assert np.all(err <= (4 * n + 4) * U)
    res = result_json(model)
    assert res["conflict_rate_all"] == rate[0] and res["conflict_rate_meta"] == rate[1]
    assert res["mean_cosine_all"] == mean[0] and res["mean_cosine_meta"] == mean[1]
    assert {"avg_auc", "domain_auc"} <= set(res)
    print(text[text.index("Domain conflict"):])


def test_run_config_without_the_flag_reports_nothing(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg, model = run_config(tmp_path, "mlp")
    assert not [k for k in result_json(model) if "conflict" in k or "cosine" in k]
    assert not os.path.exists(os.path.join(model.result_path, "domain_conflict.npz"))
