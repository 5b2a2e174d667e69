"""Diversified re-ranking (greedy MMR) on the device: mamdr_list_diversify through raw ctypes against

- the fp32 replay of its loop (list_metrics.diversify_replay) on the device's OWN cosines -- each pair's cosine read from
  mamdr_list_similarity on the 2-entry list [e_a, e_b] --: positions and values must be the replay's bytes, no tolerance;
- the float64 definition on the same fp32 inputs (list_metrics.diversify_audit / diversify_host), independently of the replay:
  every pick within 2 tol of its step's float64 best, tol = ((1 - lambda)(2 E + 8) + 8) * 2^-24 for rel in [0, 1] -- the
  cosine's derived bound (list_metrics.error_bound) scaled by its weight, plus 8 units for the rounding of 1 - lambda, of the
  two products, of the difference and of a |cos| slightly above 1; two entries can each be off by tol;
- exact cases, placement, refusals, and BaseModel.diversify on a step-engine mlp and a generic-layer mlp.

Tables of 500 rows, at most 64 lists per call."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import _lib                      # noqa: E402
from mamdr_amd import list_metrics as lm        # noqa: E402
from test_gpu_list_metrics import dev as _dev, list_similarity, need_gpu, one_hot_table, ptr, small_config, stream     # noqa: E402
from test_gpu_recommend import state_digest     # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
N_ROWS = 500
NS = (1, 2, 31, 32, 33, 64, 65, 127, 128)
LAMBDAS = (0.0, 0.3, 0.7, 1.0)


def dev(a):
    """a device copy (the fixtures are read-only arrays: copied first, torch wants writable memory)."""
    return _dev(np.array(a))


def diversify(ids, rel, d_rows, k, lam, values=True):
    """mamdr_list_diversify through ctypes -> (positions int32 [Q, k], values fp32 [Q, k] or None); the outputs start as
    garbage: the call writes every element."""
    lib = _lib.load()
    ids, rel = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(rel, F32)
    Q, n = ids.shape
    d_ids, d_rel = dev(ids), dev(rel)
    pos = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    val = torch.full((Q, k), float("nan"), dtype=torch.float32, device="cuda") if values else None
    _lib.check(lib.mamdr_list_diversify(ptr(d_ids), ptr(d_rel), Q, n, k, lam, ptr(d_rows), int(d_rows.shape[0]),
                                        int(d_rows.shape[1]), ptr(pos), ptr(val), stream()))
    return pos.cpu().numpy(), (val.cpu().numpy() if values else None)


def ks_of(n):
    return sorted({1, n, (n + 1) // 2})


# ------------------------------------------------------------------ fixtures, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def clustered_table(E):
    """500 Gaussian rows around 25 centres, scaled row by row: cosines from about -0.5 to 0.95, so similarity matters."""
    rs = np.random.RandomState(500 + E)
    centre = rs.standard_normal((25, E))
    rows = centre[rs.randint(0, 25, N_ROWS)] + 0.6 * rs.standard_normal((N_ROWS, E))
    rows = (rows * 10.0 ** rs.uniform(-1, 1, (N_ROWS, 1))).astype(F32)
    rows.setflags(write=False)
    return rows


def lists_of(rs, Q, n, scatter=True):
    """Q lists of n entries with DISTINCT valid ids: list 0 full, list 1 all padding (n > 1: else a second full one), the
    others of a drawn length 1 .. n; padding (-1, n_rows, INT32_MAX) scattered or at the tail.  rel = sigmoid(N(-1.5, 1.5)) in
    [0, 1]; list 2's rel is cut to multiples of 1/8, so equal values meet and the id decides (one list only: a tie has no
    float64 margin, and the share of lists with one is asserted below)."""
    ids = np.empty((Q, n), np.int32)
    for q in range(Q):
        L = n if q == 0 else (0 if q == 1 and n > 1 else rs.randint(1, n + 1))
        row = rs.choice(np.array([-1, N_ROWS, INT32_MAX], np.int64), n)
        where = np.sort(rs.choice(n, L, replace=False)) if scatter else np.arange(L)
        row[where] = rs.choice(N_ROWS, L, replace=False)
        ids[q] = row
    rel = (1.0 / (1.0 + np.exp(-rs.normal(-1.5, 1.5, (Q, n))))).astype(F32)
    if Q > 2:
        rel[2] = np.round(rel[2] * 8.0) / 8.0
    return ids, rel


def device_cosines(ids, d_rows):
    """per list the [L, L] fp32 matrix of the device's cosines of its valid entries a < b (zeros elsewhere): every pair's
    cosine is mamdr_list_similarity's sim_sum of the 2-entry list [e_a, e_b], in that order -- one fp32 cosine, exactly."""
    n_rows = int(d_rows.shape[0])
    pairs, shape = [], []
    for row in ids:
        e = row[(row >= 0) & (row < n_rows)]
        a, b = np.triu_indices(e.size, 1)
        pairs.append(np.stack([e[a], e[b]], 1))
        shape.append((e.size, a, b))
    flat = np.concatenate(pairs).astype(np.int32)
    sim = np.zeros(0)
    if flat.shape[0]:
        sim, n_pairs = list_similarity(flat, d_rows)
        assert np.all(n_pairs == 1)
        assert np.array_equal(sim.astype(F32).astype(np.float64), sim)        # one fp32 number each
    out, at = [], 0
    for L, a, b in shape:
        m = np.zeros((L, L), F32)
        m[a, b] = sim[at:at + a.size].astype(F32)
        at += a.size
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def problem(E, n):
    """(ids, rel, rows, the device rows, the device's cosines per list) for width E and list length n."""
    rows = clustered_table(E)
    d_rows = dev(rows)
    Q = 64 if n <= 33 else 24
    ids, rel = lists_of(np.random.RandomState(1000 * E + n), Q, n, scatter=bool(n % 2))
    cos = device_cosines(ids, d_rows)
    ids.setflags(write=False)
    rel.setflags(write=False)
    return ids, rel, rows, d_rows, cos


# ------------------------------------------------------------------ bit-exact replay
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_outputs_are_the_replays_bytes(E, n):
    need_gpu()
    ids, rel, rows, d_rows, cos = problem(E, n)
    picked_behind_relevance = 0
    for k in ks_of(n):
        for lam in LAMBDAS:
            pos, val = diversify(ids, rel, d_rows, k, lam)
            want_pos, want_val = lm.diversify_replay(ids, rel, cos, k, lam, n_rows=N_ROWS)
            assert pos.tobytes() == want_pos.tobytes(), (E, n, k, lam, np.argwhere(pos != want_pos)[:4])
            assert val.tobytes() == want_val.tobytes(), (E, n, k, lam)
            # without the values the positions are the same
            assert diversify(ids, rel, d_rows, k, lam, values=False)[0].tobytes() == pos.tobytes()
            if lam == 0.3 and k > 2:
                by_rel = lm.diversify_replay(ids, rel, cos, k, 1.0, n_rows=N_ROWS)[0]
                picked_behind_relevance += int((by_rel != pos).any(axis=1).sum())
    if n >= 31:
        assert picked_behind_relevance > 0           # the fixture's cosines matter: the picks are not relevance's order


# ------------------------------------------------------------------ the float64 definition, independently of the replay
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_every_pick_is_within_two_tol_of_the_float64_best(E, n):
    need_gpu()
    ids, rel, rows, d_rows, _ = problem(E, n)
    assert rel.min() >= 0.0 and rel.max() <= 1.0
    for k in ks_of(n):
        for lam in LAMBDAS:
            tol = lm.diversify_tol(E, lam)
            assert tol == ((1.0 - lam) * (2 * E + 8) + 8) * 2.0 ** -24
            pos, val = diversify(ids, rel, d_rows, k, lam)
            L = ((ids >= 0) & (ids < N_ROWS)).sum(axis=1)
            assert np.array_equal((pos >= 0).sum(axis=1), np.minimum(L, k))
            shortfall, _ = lm.diversify_audit(ids, rel, rows, pos, lam)        # (raises on a position picked twice)
            worst = float(shortfall.max())
            print("E %3d n %3d k %3d lambda %.1f: worst shortfall / (2 tol) = %.4f" % (E, n, k, lam, worst / (2 * tol)))
            assert worst <= 2 * tol, (E, n, k, lam)
            if k <= 20:
                want_pos, want_val = lm.diversify_host(ids, rel, rows, k, lam)
                _, margin = lm.diversify_audit(ids, rel, rows, want_pos, lam)
                clear = (margin > 2 * tol).all(axis=1)
                print("    %d of %d lists have a float64 margin above 2 tol at every step" % (clear.sum(), clear.size))
                assert clear.mean() >= 0.9, (E, n, k, lam)                     # a fixture that drifts fails loudly
                assert np.array_equal(pos[clear], want_pos[clear]), (E, n, k, lam)
                assert np.abs(val[clear] - want_val[clear]).max() <= tol


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("E", [32, 64, 128, 256])
def test_exact_cases(E):
    need_gpu()
    rows = one_hot_table(E)              # rows 0 / 8 / 24 share a column and a sign (cosine 1), 16 the column (cosine -1)
    rows = np.concatenate([rows, rows[:1]])          # row 49: a second copy of row 0 under another id
    d_rows = dev(rows)
    nan, inf = np.nan, np.inf
    cases = [   # (ids, rel, lambda, positions, values)
        # duplicated rows at lambda 0: behind the pick of 0, row 16 (cosine -1) stands at +1, the orthogonal rows at 0 in id
        # order, and the copy (cosine 1) is picked last
        ([0, 49, 1, 2, 3, 16], [0.875, 0.75, 0.125, 0.25, 0.375, 0.5], 0.0, [0, 5, 2, 3, 4, 1], [0.875, 1, 0, 0, 0, -1]),
        # the zero row's cosines are 0: row 8 (a copy of row 0 up to scale) falls behind it
        ([0, 48, 8], [1.0, 0.5, 0.75], 0.5, [0, 1, 2], [1.0, 0.25, -0.125]),
        ([48, 0, 8], [1.0, 0.5, 0.25], 0.5, [0, 1, 2], [1.0, 0.25, -0.375]),
        # all padding; a short list (L = 2 < k); one entry
        ([-1, 50, INT32_MAX, -9], [1, 1, 1, 1], 0.5, [], []),
        ([-1, 2, 50, 0], [9, 0.25, 9, 0.5], 0.5, [3, 1], [0.5, 0.125]),
        ([-1, -1, 7, -1], [9, 9, 0.5, 9], 0.25, [2], [0.5]),
        # equal values: ascending id
        ([5, 2, 4, 3], [0.5, 0.5, 0.5, 0.5], 1.0, [1, 3, 2, 0], [0.5, 0.5, 0.5, 0.5]),
        # NaN relevance goes behind every number, -inf included
        ([1, 2, 3, 4], [nan, 0.5, -inf, 0.25], 1.0, [1, 3, 2, 0], [0.5, 0.25, -inf, nan]),
    ]
    for n in (6, 32, 33, 128):                       # both kernel variants; the entries spread over the list
        for ids, rel, lam, want_pos, want_val in cases:
            where = np.round(np.linspace(0, n - 1, len(ids))).astype(int)
            row = np.full((1, n), -1, np.int32)
            r = np.full((1, n), 7.0, F32)
            row[0, where], r[0, where] = ids, rel
            for k in sorted({1, len(ids), n}):
                pos, val = diversify(row, r, d_rows, k, lam)
                wp = np.full(k, -1, np.int64)
                wv = np.zeros(k, np.float64)
                m = min(k, len(want_pos))
                wp[:m], wv[:m] = where[np.asarray(want_pos[:m], int)], want_val[:m]
                assert pos[0].tolist() == wp.tolist(), (E, n, k, ids, lam)
                assert np.array_equal(np.isnan(val[0]), np.isnan(wv)), (E, n, k, ids)
                ok = ~np.isnan(wv)
                assert val[0][ok].tobytes() == wv[ok].astype(F32).tobytes(), (E, n, k, ids, val, wv)


@pytest.mark.parametrize("E,n", [(32, 33), (64, 128), (128, 31), (256, 65)])
def test_lambda_one_is_the_stable_order_by_relevance_then_id(E, n):
    need_gpu()
    ids, rel, rows, d_rows, _ = problem(E, n)
    pos, val = diversify(ids, rel, d_rows, n, 1.0)
    for q in range(ids.shape[0]):
        at = np.flatnonzero((ids[q] >= 0) & (ids[q] < N_ROWS))
        order = at[np.lexsort((ids[q][at], -rel[q][at].astype(np.float64)))]
        assert pos[q, :at.size].tolist() == order.tolist(), (E, n, q)
        assert np.all(pos[q, at.size:] == -1) and not val[q, at.size:].any()
        assert val[q, :at.size].tobytes() == rel[q][order].tobytes()
    assert np.unique(rel[2]).size <= 9 < n               # ties are in the fixture


# ------------------------------------------------------------------ placement
def picked(ids, pos):
    """the picked item ids (-1 behind a short list)."""
    return np.where(pos >= 0, np.take_along_axis(ids, np.maximum(pos, 0).astype(np.int64), 1), -1)


def test_a_list_is_the_same_bits_wherever_it_sits():
    need_gpu()
    E, n, k, lam = 64, 48, 20, 0.3
    rows = clustered_table(E)
    d_rows = dev(rows)
    rs = np.random.RandomState(29)
    mine, rel = lists_of(rs, 64, n)
    alone = diversify(mine, rel, d_rows, k, lam)
    again = diversify(mine, rel, d_rows, k, lam)
    assert alone[0].tobytes() == again[0].tobytes() and alone[1].tobytes() == again[1].tobytes()
    rev = diversify(mine[::-1], rel[::-1], d_rows, k, lam)
    assert rev[0][::-1].tobytes() == alone[0].tobytes() and rev[1][::-1].tobytes() == alone[1].tobytes()
    # among other lists: 3 calls of 64, mine at drawn places
    others, orel = lists_of(rs, 128, n, scatter=False)
    where = np.sort(rs.choice(192, 64, replace=False))
    rest = np.setdiff1d(np.arange(192), where)
    mixed, mrel = np.empty((192, n), np.int32), np.empty((192, n), F32)
    mixed[where], mrel[where], mixed[rest], mrel[rest] = mine, rel, others, orel
    got = [diversify(mixed[i:i + 64], mrel[i:i + 64], d_rows, k, lam) for i in (0, 64, 128)]
    emb = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    assert emb[0][where].tobytes() == alone[0].tobytes() and emb[1][where].tobytes() == alone[1].tobytes()
    # the valid entries alone decide: padding at the front / in the middle / at the back / scattered, in a shorter and in a
    # longer call (both kernel variants)
    want = picked(mine, alone[0])
    valid = [np.flatnonzero((row >= 0) & (row < N_ROWS)) for row in mine]
    for n2 in (32, 33, 48, 128):
        for place in ("front", "middle", "back", "scattered"):
            ids2, rel2 = np.full((64, n2), -1, np.int32), np.full((64, n2), 0.99, F32)
            keep = np.ones(64, bool)
            for q, at in enumerate(valid):
                L = at.size
                if L > n2:
                    keep[q] = False
                    continue
                half = L // 2
                to = {"front": np.arange(n2 - L, n2), "back": np.arange(L),
                      "middle": np.concatenate([np.arange(half), np.arange(n2 - (L - half), n2)]),
                      "scattered": np.sort(rs.choice(n2, L, replace=False))}[place]
                ids2[q, to], rel2[q, to] = mine[q, at], rel[q, at]
            pos2, val2 = diversify(ids2, rel2, d_rows, k, lam)
            assert keep.sum() >= 20
            assert picked(ids2, pos2)[keep].tobytes() == want[keep].tobytes(), (n2, place)
            assert val2[keep].tobytes() == alone[1][keep].tobytes(), (n2, place)


# ------------------------------------------------------------------ refusals on live buffers
def test_refusals_launch_nothing():
    need_gpu()
    lib = _lib.load()
    d_rows = dev(clustered_table(32))
    ids, rel = dev(np.arange(8, dtype=np.int32).reshape(2, 4)), dev(np.full((2, 4), 0.5, F32))
    pos = torch.full((2, 4), 7, dtype=torch.int32, device="cuda")
    val = torch.full((2, 4), 7.0, dtype=torch.float32, device="cuda")
    call = lambda n_list=2, n=4, k=2, lam=0.5, n_rows=N_ROWS, emb=32, rows=d_rows, p=pos: lib.mamdr_list_diversify(       # noqa: E731
        ptr(ids), ptr(rel), n_list, n, k, lam, ptr(rows) if rows is not None else None, n_rows, emb, ptr(p) if p is not None else None,
        ptr(val), stream())
    for kw in (dict(n_list=0), dict(n=0, k=1), dict(n=129), dict(k=0), dict(k=5), dict(lam=-0.5), dict(lam=1.25),
               dict(lam=float("nan")), dict(n_rows=0), dict(emb=48), dict(rows=None), dict(p=None)):
        assert call(**kw) == _lib.EINVAL, kw
    assert lib.mamdr_list_diversify(ptr(ids), ptr(rel), 2, 4, 2, 0.5, C.c_void_p(d_rows.data_ptr() + 4), N_ROWS, 32, ptr(pos),
                                    ptr(val), stream()) == _lib.EINVAL
    assert lib.mamdr_list_diversify(C.c_void_p(ids.data_ptr() + 2), ptr(rel), 2, 4, 2, 0.5, ptr(d_rows), N_ROWS, 32, ptr(pos),
                                    ptr(val), stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert pos.cpu().tolist() == [[7] * 4] * 2 and val.cpu().tolist() == [[7.0] * 4] * 2         # nothing was written
    assert call() == _lib.OK


# ------------------------------------------------------------------ model level
def build(tmp_path, kind):
    from mamdr_amd import cli, engine, graph_engine
    from mamdr_amd.utils import MultiDomainDataset
    if kind == "step":
        cfg = small_config(tmp_path, "mlp", False)
    else:
        with open(os.path.join(ROOT, "config", "Taobao-10", "emb64", "deepctr_DN+DR.json")) as f:
            cfg = copy.deepcopy(json.load(f))
        cfg["model"].update(name="mlp")
        cfg["train"].update(epoch=1, patience=1, result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
        cfg["dataset"].update(batch_size=256, synthetic_scale=0.05, synthetic_seed=7)
    model = cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    eng = model.model
    assert isinstance(eng, engine.TowerEngine if kind == "step" else graph_engine.GraphEngine)
    for d in range(10):                             # a small trained tower: up to 4 whole batches of every domain
        steps = min(4, eng.n_rows(d, "train") // 256)
        if steps:
            eng.train_steps(d, n_steps=steps, lr=1e-2)
    return model, eng


def mean_ild(eng, ids):
    t = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(eng.device)
    sim, pairs = eng.list_similarity(t, eng.item_rows())
    sim, pairs = sim.cpu().numpy(), pairs.cpu().numpy()
    return float((1.0 - sim[pairs > 0] / pairs[pairs > 0]).mean())


@pytest.mark.parametrize("kind", ["step", "generic"])
def test_model_diversify(tmp_path, kind):
    need_gpu()
    model, eng = build(tmp_path, kind)
    before = state_digest(eng) if kind == "step" else eng.get_weights().clone()
    rows = eng.item_rows().cpu().numpy().copy()
    ds = model.dataset
    for d in (0, 4):
        k, pool = 10, 50
        r = model.diversify(d, k, pool, 0.3)
        base, wide = model.recommend(d, k), model.recommend(d, pool)
        assert r["ids"].shape == r["scores"].shape == r["pos"].shape == r["values"].shape == base["ids"].shape
        assert r["base_ids"].tobytes() == base["ids"].tobytes() and r["pool_ids"].tobytes() == wide["ids"].tobytes()
        # every re-ranked id comes from that user's pool, once, and none is an item the user has seen
        seen = {}
        for store in (ds.train_dataset, ds.val_dataset):
            c = store[d]["data"]
            for u, p in zip(np.asarray(c["uid"]).tolist(), np.asarray(c["pid"]).tolist()):
                seen.setdefault(u, set()).add(p)
        for q, u in enumerate(r["users"].tolist()):
            got = r["ids"][q][r["ids"][q] >= 0].tolist()
            assert len(set(got)) == len(got) == min(k, int((wide["ids"][q] >= 0).sum()))
            assert set(got) <= set(wide["ids"][q].tolist()) and not set(got) & seen.get(u, set())
        at = np.maximum(r["pos"], 0).astype(np.int64)
        assert np.array_equal(r["ids"], np.where(r["pos"] >= 0, np.take_along_axis(wide["ids"], at, 1), -1))
        assert np.array_equal(r["scores"], np.where(r["pos"] >= 0, np.take_along_axis(wide["scores"], at, 1), 0))
        # the picks against the float64 definition on the same relevance
        rel = lm.minmax_relevance(wide["scores"], wide["ids"], rows.shape[0])
        tol = lm.diversify_tol(rows.shape[1], 0.3)
        assert lm.diversify_audit(wide["ids"], rel, rows, r["pos"], 0.3)[0].max() <= 2 * tol
        # lambda = 1 on the scores as they are: recommend(domain, k)'s bytes
        same = model.diversify(d, k, pool, 1.0, relevance="score")
        assert same["ids"].tobytes() == base["ids"].tobytes() and same["scores"].tobytes() == base["scores"].tobytes()
        # intra-list diversity from list_eval's own similarity call: not below the base lists', on a fixture where the
        # float64 host definition already shows it
        host_pos, _ = lm.diversify_host(wide["ids"], rel, rows, k, 0.3)
        host_ids = np.where(host_pos >= 0, np.take_along_axis(wide["ids"], np.maximum(host_pos, 0).astype(np.int64), 1), -1)
        ild = lambda lists: float(np.mean([1.0 - s / p for s, p in zip(*lm.list_similarity_host(lists, rows)) if p > 0]))   # noqa: E731
        assert ild(host_ids) > ild(base["ids"])
        got, was = mean_ild(eng, r["ids"]), mean_ild(eng, base["ids"])
        print("%s domain %d: ILD@10 %.4f -> %.4f (lambda 0.3, pool 50)" % (kind, d, was, got))
        assert got >= was
    if kind == "step":
        assert state_digest(eng) == before                 # it reads state only
    else:
        assert torch.equal(eng.get_weights(), before)
    eng.close()


def test_run_config_with_diversify(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 MAMDR config, shrunk, with --recommend 10 --diversify 0.7: both sides are
    printed per domain, the .npz and the result.json keys exist, and the base side is the list report's."""
    need_gpu()
    from mamdr_amd import cli
    cfg = small_config(tmp_path, "mlp_meta_mamdr", False)
    cfg["train"].update(diversify=0.7, list_metrics=10)
    built = []
    res = cli.main(cfg, on_model=built.append, recommend=10)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    rdir = [os.path.join(model.result_path, f) for f in os.listdir(model.result_path) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    assert result["diversify_lambda"] == 0.7 and result["diversify_pool"] == 50
    with np.load(os.path.join(model.result_path, "diversify_top10.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and int(z["k"]) == 10 and int(z["pool"]) == 50
        for key in lm.ACCURACY + lm.FIGURES:
            assert sorted(result["domain_%s_diversified" % key]) == sorted(str(d) for d in range(10)), key
            assert result["domain_%s_diversified" % key]["3"] == float(z[key + "_diversified"][3])
            assert z[key].shape == z[key + "_diversified"].shape == (10,)
        for key in lm.AVERAGED + ("ndcg",):
            assert result["avg_%s_diversified" % key] == pytest.approx(float(np.mean(z[key + "_diversified"])))
        for key in lm.FIGURES:                             # the base side is --list-metrics' report of the same lists
            assert result["domain_" + key]["3"] == float(z[key][3]), key
        for d in range(10):
            Q = z["users_%d" % d].size
            assert z["ids_%d" % d].shape == z["base_ids_%d" % d].shape == z["pos_%d" % d].shape == z["values_%d" % d].shape == (Q, 10)
            assert np.all(z["pos_%d" % d][:, 0] == 0)      # step 0 is the most relevant entry
    text = capsys.readouterr().out
    assert "Diversify top-10 of top-50, lambda 0.7" in text and text.count(" ILD ") >= 10
    print(text[text.index("Diversify top-10"):])
