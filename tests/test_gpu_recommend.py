"""Top-K retrieval on the device (mamdr_recommend, TowerEngine.recommend, run.py --recommend) against oracle/tower.py's
`OracleModel.predict` over explicit (user, item, domain) triples.

Problem: synthetic.generate("taobao10", scale=0.05, seed=7) -- 1,188 users, 346 items, 10 domains; 346 candidates are five
64-wide tiles of k_rec_score plus a remainder of 26, eleven 32-row workgroups of k_rec_item_proj with a remainder of 26.
Weights as tests/test_gpu_embdim.py:make_problem sets them up: random biases and linear tables, gb = 0.1.

The prediction bar is the project's (test_evaluation_matches_oracle): rtol 2e-5, atol 2e-7.
"""
import copy
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import tower as otower      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-5, 2e-7
TOWERS = ["mlp", "wdl", "deepfm"]
Q_DOMAINS = np.array([0, 3, 3, 9, 5, 0, 7], np.int32)       # 7 queries, mixed domains (two users share domain 3 / 0)

_GEN, _ORACLE = {}, {}


def tol(x):
    return ATOL + RTOL * abs(float(x))


def gen():
    if "g" not in _GEN:
        from mamdr_amd import synthetic
        _GEN["g"] = synthetic.generate("taobao10", batch_size=256, seed=7, scale=0.05)
        assert (_GEN["g"]["n_user"], _GEN["g"]["n_item"], _GEN["g"]["n_domain"]) == (1188, 346, 10)
    return _GEN["g"]


def make_params(trainable, seed=7):
    g = gen()
    rs = np.random.RandomState(seed)
    params = otower.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for n in ("b0", "b1", "b2", "lin_domain", "lin_user", "lin_item"):
        params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    params["gb"] = np.array([0.1], F32)
    if not trainable:               # frozen linear tables stay at their zero initialisation
        params["lin_user"][...] = 0
        params["lin_item"][...] = 0
    return params


def make_engine(tower, trainable, params=None, dropout=0.5, bind=()):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd.engine import TowerEngine
    g = gen()
    params = make_params(trainable) if params is None else params
    eng = TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 256, dropout=dropout, emb_trainable=trainable, tower=tower)
    if not trainable:
        eng.bind_table("user_emb", params["user_emb"])
        eng.bind_table("item_emb", params["item_emb"])
    for d in bind:
        c = g["data"]["train"][d]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    return eng, params


def queries():
    uids = np.random.RandomState(11).choice(gen()["n_user"], Q_DOMAINS.size, replace=False).astype(np.int32)
    return uids, Q_DOMAINS


def oracle_scores(params, tower, trainable, cand, uids=None, doms=None):
    """[Q, n_cand] OracleModel.predict over the explicit triples."""
    if uids is None:
        uids, doms = queries()
    model = otower.OracleModel(params, emb_trainable=trainable, dropout=0.0, tower=tower)
    cand = np.asarray(cand, np.int32)
    return np.stack([model.predict(np.full(cand.size, u, np.int32), cand, np.full(cand.size, d, np.int32))
                     for u, d in zip(uids, doms)])


def reference(tower, trainable):
    """the oracle's scores of the 7 queries over all 346 items at make_params' weights: computed once, never modified."""
    key = (tower, trainable)
    if key not in _ORACLE:
        ref = oracle_scores(make_params(trainable), tower, trainable, np.arange(gen()["n_item"]))
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


@pytest.fixture(scope="module")
def engines():
    """one engine per (tower, trainable) for the tests that only read it."""
    made = {}

    def get(tower, trainable):
        if (tower, trainable) not in made:
            made[(tower, trainable)] = make_engine(tower, trainable)[0]
        return made[(tower, trainable)]
    yield get
    for e in made.values():
        e.close()


def exclusion_lists(ref, cand):
    """per query an unsorted list with duplicates: 40 random candidates, the oracle's best three, ids outside the
    candidate list; query 2 excludes nothing."""
    rs = np.random.RandomState(3)
    out = []
    for q in range(ref.shape[0]):
        best = cand[np.argsort(-ref[q, cand], kind="stable")[:3]]
        e = np.concatenate([rs.choice(cand, 40, replace=False), best, best[:1], np.setdiff1d(np.arange(346), cand)[:5]])
        out.append([] if q == 2 else rs.permutation(e))
    return out


def candidate_list(subset):
    return np.random.RandomState(5).permutation(346)[:201].astype(np.int32) if subset else np.arange(346, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
@pytest.mark.parametrize("tower", TOWERS)
def test_scores_match_oracle(engines, tower, trainable):
    uids, doms = queries()
    ids, scores, all_scores = engines(tower, trainable).recommend(uids, doms, 10, want_scores=True)
    ref = reference(tower, trainable)
    assert all_scores.shape == ref.shape == (7, 346) and all_scores.dtype == np.float32
    err = np.abs(all_scores - ref) / (ATOL + RTOL * np.abs(ref))
    print("%s %s: worst |err| / bar = %.4f" % (tower, "trainable" if trainable else "frozen", err.max()))
    np.testing.assert_allclose(all_scores, ref, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 2
def check_topk(ids, scores, all_scores, ref, cand, excl, k):
    """the contract of one call's outputs, every query: see the test's docstring."""
    for q in range(ids.shape[0]):
        ex = np.unique(np.asarray(excl[q], np.int64)) if excl is not None else np.zeros(0, np.int64)
        allowed = ~np.isin(cand, ex)
        n_out = min(k, int(allowed.sum()))
        got, sc = ids[q, :n_out], scores[q, :n_out]
        assert np.all(ids[q, n_out:] == -1) and np.all(scores[q, n_out:] == 0)
        assert np.all(all_scores[q, ~allowed] == 0)
        if n_out == 0:
            continue
        assert np.unique(got).size == n_out and np.all(np.isin(got, cand[allowed])), (q, got)
        pos = np.array([int(np.nonzero(cand == i)[0][0]) for i in got], np.int64)
        assert np.array_equal(sc.view(np.uint32), all_scores[q, pos].view(np.uint32)), q      # bit for bit
        assert np.all(np.diff(sc) <= 0), (q, sc)
        o = ref[q, cand]                                       # the oracle's scores in candidate order
        o_allowed = np.sort(o[allowed])[::-1]
        kth_oracle = o_allowed[n_out - 1]
        assert np.all(o[pos] >= kth_oracle - tol(kth_oracle)), (q, o[pos].min(), kth_oracle)
        must = cand[allowed & (o > sc[-1] + tol(sc[-1]))]
        assert np.all(np.isin(must, got)), (q, np.setdiff1d(must, got))


@pytest.mark.parametrize("subset", [False, True], ids=["all346", "subset201"])
@pytest.mark.parametrize("with_excl", [False, True], ids=["noexcl", "excl"])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("tower,trainable", [("mlp", False), ("deepfm", True)], ids=["mlp-frozen", "deepfm-trainable"])
def test_topk_semantics(engines, tower, trainable, k, with_excl, subset):
    """For every query: the returned ids are distinct, drawn from the candidates, not excluded; returned scores equal the
    same call's all_scores entries bit for bit and are non-increasing; against the oracle, with tol the bar of the score
    test: every returned id's oracle score >= the oracle's K-th best - tol, and every candidate whose oracle score exceeds
    the returned K-th score + tol is returned.  (Equal logits by ascending id: test_exact_ties -- two different logits
    can round to one score, so adjacent equal scores here say nothing about the ids' order.)"""
    uids, doms = queries()
    ref = reference(tower, trainable)
    cand = candidate_list(subset)
    excl = exclusion_lists(ref, cand) if with_excl else None
    ids, scores, all_scores = engines(tower, trainable).recommend(uids, doms, k, candidates=cand if subset else None,
                                                                  exclude=excl, want_scores=True)
    assert ids.shape == scores.shape == (7, k) and all_scores.shape == (7, cand.size)
    check_topk(ids, scores, all_scores, ref, cand, excl, k)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tower", TOWERS)
def test_exact_ties_rank_by_id_wherever_the_pair_sits(tower):
    """every item row identical (lin_item = 0: frozen tables): a query's 346 logits are ONE value whatever tile, lane and
    remainder a pair sits in, and the top 10 are the ten smallest non-excluded ids, ascending -- by id, not by position
    (the candidates are shuffled)."""
    params = make_params(False)
    params["item_emb"] = np.repeat(params["item_emb"][17:18], 346, axis=0)
    eng, _ = make_engine(tower, False, params)
    uids, doms = queries()
    cand = np.random.RandomState(9).permutation(346).astype(np.int32)
    excl = [[0, 3, 4, 300]] * 3 + [[]] * 4
    ids, scores, all_scores = eng.recommend(uids, doms, 10, candidates=cand, exclude=excl, want_scores=True)
    eng.close()
    for q in range(7):
        allowed = ~np.isin(cand, excl[q])
        bits = np.unique(all_scores[q, allowed].view(np.uint32))
        assert bits.size == 1, (q, bits)
        assert np.all(all_scores[q, ~allowed] == 0)
        want = np.setdiff1d(np.arange(346), excl[q])[:10]
        assert ids[q].tolist() == want.tolist(), (q, ids[q])
        assert np.all(scores[q].view(np.uint32) == bits[0])
    np.testing.assert_allclose(all_scores[3], oracle_scores(params, tower, False, cand)[3], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 4
def chunk_case(tower, trainable, path):
    """the calls of the chunking test, dumped to `path` (run in the test's process and in its child)."""
    eng, _ = make_engine(tower, trainable)
    uids, doms = queries()
    ref = reference(tower, trainable)
    out = {}
    for k, subset in ((10, False), (128, False), (10, True)):
        cand = candidate_list(subset)
        ids, scores, all_scores = eng.recommend(uids, doms, k, candidates=cand if subset else None,
                                                exclude=exclusion_lists(ref, cand), want_scores=True)
        out.update({"ids_%d_%d" % (k, subset): ids, "scores_%d_%d" % (k, subset): scores, "all_%d_%d" % (k, subset): all_scores})
    eng.close()
    np.savez(path, **out)


@pytest.mark.parametrize("tower,trainable", [("mlp", False), ("deepfm", True)], ids=["mlp-frozen", "deepfm-trainable"])
def test_chunking_does_not_change_a_bit(tmp_path, tower, trainable):
    """MAMDR_REC_CHUNK=128 in a fresh child process: three chunks (128 + 128 + 90) for 346 candidates, two for the 201-id
    subset -- ids, scores and the dense score matrix are bit-identical to the default (one chunk) run."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    chunk_case(tower, trainable, str(tmp_path / "one.npz"))
    code = "import test_gpu_recommend as t; t.chunk_case(%r, %r, %r)" % (tower, trainable, str(tmp_path / "three.npz"))
    env = dict(os.environ, MAMDR_REC_CHUNK="128",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(tmp_path / "one.npz")) as a, np.load(str(tmp_path / "three.npz")) as b:
        assert sorted(a.files) == sorted(b.files) and len(a.files) == 9
        for name in a.files:
            assert a[name].tobytes() == b[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- 5
def test_short_lists_end_in_padding(engines):
    eng = engines("wdl", True)
    uids, doms = queries()
    ref = reference("wdl", True)
    cand = np.array([340, 7, 120, 64, 345], np.int32)
    ids, scores, all_scores = eng.recommend(uids, doms, 10, candidates=cand, want_scores=True)
    check_topk(ids, scores, all_scores, ref, cand, None, 10)
    assert np.all(ids[:, 5:] == -1) and np.all(scores[:, 5:] == 0) and np.all(ids[:, :5] >= 0)
    # query 4's exclusion list covers all but two of the 346 candidates, query 1's all of them
    cand = np.arange(346, dtype=np.int32)
    excl = [[] for _ in range(7)]
    excl[4] = np.setdiff1d(cand, [33, 290])
    excl[1] = cand
    ids, scores, all_scores = eng.recommend(uids, doms, 10, exclude=excl, want_scores=True)
    check_topk(ids, scores, all_scores, ref, cand, excl, 10)
    assert sorted(ids[4, :2].tolist()) == [33, 290] and np.all(ids[4, 2:] == -1) and np.all(scores[4, 2:] == 0)
    assert np.all(ids[1] == -1) and np.all(scores[1] == 0) and np.all(all_scores[1] == 0)
    assert np.all(ids[0] >= 0)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("tower", ["mlp", "deepfm"])
def test_after_training_the_live_rows_are_scored(tower):
    """trainable tables, three Adam steps, then recommend BEFORE anything else synchronises the lazily stepped table rows:
    the scores are the oracle's at the weights get_weights() hands out afterwards."""
    g = gen()
    d = max(range(10), key=lambda i: g["data"]["train"][i]["uid"].shape[0])
    eng, params = make_engine(tower, True, bind=(d,))
    assert eng.train_steps(d, n_steps=3, lr=1e-2) == 3
    uids, doms = queries()
    ids, scores, all_scores = eng.recommend(uids, doms, 10, want_scores=True)
    live = eng.unpack(eng.get_weights())
    eng.close()
    moved = np.abs(live["item_emb"].reshape(346, 128) - params["item_emb"]).max(axis=1)
    assert (moved > 0).all()                                   # dense Adam moved every row, touched by a batch or not
    trained = {n: live[n].reshape(params[n].shape) for n in live}
    ref = oracle_scores(dict(params, **trained), tower, True, np.arange(346))
    np.testing.assert_allclose(all_scores, ref, rtol=RTOL, atol=ATOL)
    assert np.abs(ref - reference(tower, True)).max() > 1e-3   # ... and training did change the scores
    check_topk(ids, scores, all_scores, ref, np.arange(346, dtype=np.int32), None, 10)


# ---------------------------------------------------------------------------------------------------------------- 7
def state_digest(eng):
    from mamdr_amd import _lib
    h = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (eng.weights, eng.adam_m, eng.adam_v)]
    return h + [int(eng.lib.mamdr_optimizer_steps(eng.ctx)), int(eng.lib.mamdr_dropout_steps(eng.ctx))] + \
        [int(_lib.load().mamdr_pregather_hits(eng.ctx))]


@pytest.mark.parametrize("tower,trainable", [("mlp", False), ("deepfm", True)], ids=["mlp-frozen", "deepfm-trainable"])
def test_recommend_reads_the_state_only(tower, trainable):
    g = gen()
    d = max(range(10), key=lambda i: g["data"]["train"][i]["uid"].shape[0])
    n_steps = -(-g["data"]["train"][d]["uid"].shape[0] // 256)
    assert n_steps >= 4
    uids, doms = queries()
    a, _ = make_engine(tower, trainable, bind=(d,))
    b, _ = make_engine(tower, trainable, bind=(d,))
    a.train_steps(d, n_steps=2)
    b.train_steps(d, n_steps=2)
    before = state_digest(a)
    first = a.recommend(uids, doms, 10, want_scores=True)
    assert state_digest(a) == before
    again = a.recommend(uids, doms, 10, want_scores=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    # one Adam pass, twin b never calls recommend: the same calls otherwise
    for s in range(2, n_steps):
        a.train_steps(d, first_step=s, n_steps=1)
        a.recommend(uids, doms, 128, exclude=[[1, 2]] * 7)
        if s % 2:
            a.recommend(uids[:1], doms[:1], 1, candidates=[5, 6, 7])
        b.train_steps(d, first_step=s, n_steps=1)
    assert state_digest(a) == state_digest(b)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals(engines):
    from mamdr_amd import _lib, graph_engine
    from mamdr_amd.engine import TowerEngine
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    uids, doms = queries()
    for tower in ("star", "pnn", "nfm"):
        eng = TowerEngine(1188, 346, 10, 256, tower=tower)
        with pytest.raises(_lib.NotBuiltError, match=r"\b%s tower" % tower):
            eng.recommend(uids, doms, 10)
        eng.close()
    eng = engines("mlp", False)
    for k in (0, 129):
        with pytest.raises(_lib.MamdrError) as e:
            eng.recommend(uids, doms, k)
        assert e.value.code == _lib.EINVAL and "k %d" % k in str(e.value)
    launched = []
    real = eng.lib.mamdr_recommend
    try:
        eng.lib.mamdr_recommend = lambda *a: launched.append(a) or 0
        for bad in (dict(uids=[1188], domains=[0]), dict(uids=[-1], domains=[0]), dict(uids=[0], domains=[10])):
            with pytest.raises(ValueError):
                eng.recommend(k=5, **bad)
        with pytest.raises(ValueError):
            eng.recommend([0], [0], 5, candidates=[346])
        with pytest.raises(ValueError):
            eng.recommend([0], [0], 5, candidates=[3, 3])
        with pytest.raises(ValueError):
            eng.recommend([0], [0], 5, exclude=[[1], [2]])
    finally:
        eng.lib.mamdr_recommend = real
    assert not launched                                        # refused on the host, before any launch
    # state not bound: ESTATE
    import ctypes as C
    raw = TowerEngine(1188, 346, 10, 256)                      # frozen tables, none bound
    out_i = torch.zeros(10, dtype=torch.int32, device=raw.device)
    out_f = torch.zeros(10, dtype=torch.float32, device=raw.device)
    q = torch.zeros(1, dtype=torch.int32, device=raw.device)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert real(raw.ctx, 1, p(q), p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.ESTATE
    assert real(raw.ctx, 0, p(q), p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    assert real(raw.ctx, 1, p(q), p(q), p(q), 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    assert real(raw.ctx, 1, None, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    assert real(raw.ctx, 1, C.c_void_p(q.data_ptr() + 2), p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    raw.close()
    geng = graph_engine.GraphEngine("mlp", 1188, 346, 10, 256, (128, 64), (), emb_dim=64)
    with pytest.raises(NotImplementedError, match="generic-layer towers"):
        geng.recommend(uids, doms, 10)
    geng.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_run_config_with_recommend(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 config (width 128, sized as test_run_config_at_width_64 sizes its run) with
    --recommend 10: the .npz, no seen item returned, metrics inside [0, 1].  No quality bar: HitRate@10 is printed beside
    the random ranking's expectation 10 / |catalogue| (recorded in profiles/recommend_bench.txt)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    out = str(tmp_path / "rec.npz")
    res = cli.main(cfg, on_model=built.append, recommend=10, recommend_out=out)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    assert isinstance(model.model, engine.TowerEngine)
    ds = model.dataset
    text = capsys.readouterr().out
    with np.load(out) as z:
        assert z["domains"].tolist() == list(range(10))
        for name in ("hit_rate", "recall", "ndcg"):
            assert z[name].shape == (10,) and np.all(np.isfinite(z[name])) and np.all((z[name] >= 0) & (z[name] <= 1))
        for d in range(10):
            users, ids, scores = z["users_%d" % d], z["ids_%d" % d], z["scores_%d" % d]
            assert np.array_equal(users, np.unique(ds.test_dataset[d]["data"]["uid"]))
            assert ids.shape == scores.shape == (users.size, 10) and ids.dtype == np.int32 and scores.dtype == np.float32
            splits = (ds.train_dataset[d]["data"], ds.val_dataset[d]["data"], ds.test_dataset[d]["data"])
            catalogue = np.unique(np.concatenate([c["pid"] for c in splits]))
            assert np.all(np.isin(ids[ids >= 0], catalogue))
            seen = {}
            for c in splits[:2]:
                for u, p in zip(c["uid"].tolist(), c["pid"].tolist()):
                    seen.setdefault(u, set()).add(p)
            for q, u in enumerate(users.tolist()):
                got = ids[q][ids[q] >= 0].tolist()
                assert len(set(got)) == len(got) and not (set(got) & seen.get(u, set())), (d, u)
            print("domain %d: HitRate@10 %.4f, random ranking %.4f (catalogue %d)" % (
                d, z["hit_rate"][d], min(1.0, 10.0 / catalogue.size), catalogue.size))
    assert "Recommend top-10" in text and text.count("HitRate@10") == 10
    print(text[text.index("Recommend top-10"):])
