"""Single-domain top-K retrieval on the device (mamdr_recommend_domain, TowerEngine.recommend_domain, run.py --recommend on
the Star tower) against oracle/star.py's inference forward over explicit (user, item, domain) triples with a constant domain
column, and against the engine's own evaluation of the same triples.

Problem: tests/test_gpu_recommend.py's -- synthetic.generate("taobao10", scale=0.05, seed=7): 1,188 users, 346 items, 10
domains; 346 candidates are five 64-wide tiles of k_rec_score plus a remainder of 26, ten full 32-row workgroups of
k_rec_item_proj plus the same remainder.  Star weights as tests/test_gpu_parity.py:make_star_problem sets them up (gamma
perturbed by 0.2, betas and biases at 0.05, Wd* x 8).  Moving statistics: domains 0 and 3 carry the moments of their raw
train rows [u | i | dm] (the domain columns' variance is 0: scale = gamma / sqrt(1e-3)), domain 9 the initial mean 0 /
variance 1.

The score bar (tests 1 - 3) is the project's retrieval bar, rtol 2e-5, atol 2e-7 (test_gpu_recommend.py).  Measured on an
MI355X at this problem (profiles/recommend_star_parity.txt), worst |err| / (2e-7 + 2e-5 |x|) over the 7 x 346 pairs of
domains 0 / 3 / 9: retrieval against the oracle 0.0117 / 0.0121 / 0.0090, the evaluation path (mamdr_eval_domain) against
the oracle 0.0115 / 0.0118 / 0.0089, retrieval against the evaluation 0.0114 / 0.0116 / 0.0060 -- the Star tower meets the
bar as it stands, so it is not widened.  After training (test 8) the bar is the project's Star evaluation bar, rtol 5e-4,
atol 5e-5 (test_star_step_adam_eval); measured worst error 0.145 of it in the trained domain.
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

from oracle import star as ostar        # noqa: E402
from oracle import tower as otower      # noqa: E402
import test_gpu_recommend as base       # noqa: E402  (the problem, the mlp / wdl / deepfm engines, the lists of its tests)

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the retrieval bar of tests/test_gpu_recommend.py, met as it stands (module docstring, profiles/recommend_star_parity.txt)
RTOL, ATOL = 2e-5, 2e-7
RTOL_TRAINED, ATOL_TRAINED = 5e-4, 5e-5
DOMAINS = (0, 3, 9)
STAT_DOMAINS = (0, 3)              # domains whose moving statistics are their train rows' moments

_CACHE = {}


def tol(x, rtol=RTOL, atol=ATOL):
    return atol + rtol * abs(float(x))


def users7():
    return base.queries()[0]


def star_params(seed=11):
    """tests/test_gpu_parity.py:make_star_problem's recipe at this problem."""
    g = base.gen()
    rs = np.random.RandomState(seed)
    p = ostar.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
    p["user_emb"] = g["tables"]["user_emb"].copy()
    p["item_emb"] = g["tables"]["item_emb"].copy()
    for n in ("pn_gamma_shared", "pn_gamma_spec"):
        p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
    for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
        p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
    for l in range(3):
        p["Wd%d" % l] = (p["Wd%d" % l] * 8).astype(F32)
    return p


def star_state(params):
    """the oracle's PartitionedNorm state with domains 0 and 3 at the moments of their raw train rows."""
    g = base.gen()
    state = ostar.init_state(g["n_domain"])
    for d in STAT_DOMAINS:
        c = g["data"]["train"][d]
        mean, var = ostar.batch_moments(otower.gather(params, c["uid"], c["pid"], c["domain"]))
        state["mov_mean"][d], state["mov_var"][d] = mean, var
    return state


def make_star_engine(trainable, bind=(), stats=True):
    """-> (engine, params, state): the Star step engine at star_params with star_state's moving statistics in eng.aux
    (layout: TowerEngine.aux_state -- mov_mean [D, 384] | mov_var [D, 384] | ...)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd.engine import TowerEngine
    g = base.gen()
    params = star_params()
    eng = TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 256, dropout=0.0, emb_trainable=trainable, tower="star")
    if not trainable:
        eng.bind_table("user_emb", params["user_emb"])
        eng.bind_table("item_emb", params["item_emb"])
    for d in bind:
        c = g["data"]["train"][d]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    eng.set_weights(eng.pack(params))
    state = star_state(params) if stats else ostar.init_state(g["n_domain"])
    if stats:
        dx = g["n_domain"] * 384
        for d in STAT_DOMAINS:
            eng.aux[d * 384:(d + 1) * 384] = torch.from_numpy(state["mov_mean"][d]).to(eng.device)
            eng.aux[dx + d * 384:dx + (d + 1) * 384] = torch.from_numpy(state["mov_var"][d]).to(eng.device)
        aux = eng.aux_state()
        assert np.array_equal(aux["mov_mean"], state["mov_mean"]) and np.array_equal(aux["mov_var"], state["mov_var"])
        assert np.abs(aux["mov_mean"][3]).max() > 0 and np.all(aux["mov_var"][9] == 1)
    return eng, params, state


def oracle_scores(params, state, uids, cand, domain):
    """[Q, n_cand] oracle/star.py's inference forward over the explicit triples, constant domain column."""
    uids, cand = np.asarray(uids, np.int32), np.asarray(cand, np.int32)
    uid = np.repeat(uids, cand.size)
    pid = np.tile(cand, uids.size)
    p, _ = ostar.forward(params, state, uid, pid, np.full(uid.shape, domain, np.int32), training=False)
    return p.reshape(uids.size, cand.size)


def reference(domain):
    """the oracle's scores of the 7 users over all 346 items in `domain`: computed once, never modified (the Star tower
    has no linear tables: frozen and trainable engines hold the same weights)."""
    if ("ref", domain) not in _CACHE:
        params = star_params()
        ref = oracle_scores(params, star_state(params), users7(), np.arange(346), domain)
        ref.setflags(write=False)
        _CACHE[("ref", domain)] = ref
    return _CACHE[("ref", domain)]


@pytest.fixture(scope="module")
def star_engines():
    """one Star engine per `trainable` for the tests that only read it."""
    made = {}

    def get(trainable):
        if trainable not in made:
            made[trainable] = make_star_engine(trainable)[0]
        return made[trainable]
    yield get
    for e in made.values():
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
def test_scores_match_oracle(star_engines, trainable, domain):
    ids, scores, all_scores = star_engines(trainable).recommend_domain(users7(), domain, 10, want_scores=True)
    ref = reference(domain)
    assert all_scores.shape == ref.shape == (7, 346) and all_scores.dtype == np.float32
    assert len(np.unique(ref)) > 2000 and ref.std() > 1e-3            # (no saturated tower: the scores do differ)
    err = np.abs(all_scores - ref) / (ATOL + RTOL * np.abs(ref))
    print("star %s domain %d: retrieval against the oracle, worst |err| / bar = %.4f (bar rtol %g atol %g)" % (
        "trainable" if trainable else "frozen", domain, err.max(), RTOL, ATOL))
    np.testing.assert_allclose(all_scores, ref, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
def test_scores_match_the_engines_own_evaluation(star_engines, trainable, domain):
    """the same (user, item, domain) triples bound as the domain's test split: mamdr_eval_domain's predictions against
    recommend_domain's dense scores at the bar of test 1 (printed: the evaluation path's own worst error against the
    oracle, in units of the retrieval bar rtol 2e-5 / atol 2e-7)."""
    eng = star_engines(trainable)
    uids = users7()
    uid, pid = np.repeat(uids, 346), np.tile(np.arange(346, dtype=np.int32), uids.size)
    eng.bind_domain_data(domain, "test", uid, pid, np.full(uid.shape, domain, np.int32), np.zeros(uid.shape, F32))
    preds = eng.evaluate(domain, "test", want_preds=True)[3].reshape(7, 346)
    all_scores = eng.recommend_domain(uids, domain, 10, want_scores=True)[2]
    ref = reference(domain)
    unit = 2e-7 + 2e-5 * np.abs(ref)
    print("star %s domain %d: evaluation against the oracle, worst |err| / (2e-7 + 2e-5 |x|) = %.4f; retrieval against the "
          "oracle %.4f; retrieval against the evaluation %.4f" % (
              "trainable" if trainable else "frozen", domain, (np.abs(preds - ref) / unit).max(),
              (np.abs(all_scores - ref) / unit).max(), (np.abs(all_scores - preds) / unit).max()))
    np.testing.assert_allclose(all_scores, preds, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 3
def check_topk(ids, scores, all_scores, ref, cand, excl, k):
    """the contract of one call's outputs, every query (tests/test_gpu_recommend.py:check_topk at this module's bar):
    returned ids distinct, drawn from the candidates, not excluded; returned scores equal the call's all_scores entries bit
    for bit and are non-increasing; -1 / 0 behind a short list; against the oracle a swap only between items whose oracle
    scores differ by less than the bar."""
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
        # the top n_out of the call's own dense scores: nothing left out scores above the last one returned
        rest = allowed.copy()
        rest[pos] = False
        assert not rest.any() or all_scores[q, rest].max() <= sc[-1], q
        o = ref[q, cand]                                       # the oracle's scores in candidate order
        kth_oracle = np.sort(o[allowed])[::-1][n_out - 1]
        assert np.all(o[pos] >= kth_oracle - tol(kth_oracle)), (q, o[pos].min(), kth_oracle)
        must = cand[allowed & (o > sc[-1] + tol(sc[-1]))]
        assert np.all(np.isin(must, got)), (q, np.setdiff1d(must, got))


@pytest.mark.parametrize("subset", [False, True], ids=["all346", "subset201"])
@pytest.mark.parametrize("with_excl", [False, True], ids=["noexcl", "excl"])
@pytest.mark.parametrize("k", [1, 10, 64, 128])
def test_topk_semantics(star_engines, k, with_excl, subset):
    ref = reference(3)
    cand = base.candidate_list(subset)
    excl = base.exclusion_lists(ref, cand) if with_excl else None
    ids, scores, all_scores = star_engines(True).recommend_domain(users7(), 3, k, candidates=cand if subset else None,
                                                                  exclude=excl, want_scores=True)
    assert ids.shape == scores.shape == (7, k) and all_scores.shape == (7, cand.size)
    check_topk(ids, scores, all_scores, ref, cand, excl, k)


# ---------------------------------------------------------------------------------------------------------------- 4
def chunk_case(path):
    """the calls of the chunking test, dumped to `path` (run in the test's process and in its children)."""
    eng = make_star_engine(True)[0]
    ref = reference(3)
    out = {}
    for k, subset in ((10, False), (128, False), (10, True)):
        cand = base.candidate_list(subset)
        ids, scores, all_scores = eng.recommend_domain(users7(), 3, k, candidates=cand if subset else None,
                                                       exclude=base.exclusion_lists(ref, cand), want_scores=True)
        out.update({"ids_%d_%d" % (k, subset): ids, "scores_%d_%d" % (k, subset): scores, "all_%d_%d" % (k, subset): all_scores})
    eng.close()
    np.savez(path, **out)


@pytest.mark.parametrize("chunk", [64, 128])
def test_chunking_does_not_change_a_bit(tmp_path_factory, chunk):
    """MAMDR_REC_CHUNK = 64 / 128 in a fresh child process (the switch is read at load): six / three chunks for 346
    candidates, four / two for the 201-id subset -- ids, scores and the dense score matrix are bit-identical to the default
    (one chunk) run."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if "one_chunk" not in _CACHE:
        _CACHE["one_chunk"] = str(tmp_path_factory.mktemp("chunks") / "one.npz")
        chunk_case(_CACHE["one_chunk"])
    path = str(tmp_path_factory.mktemp("chunks") / ("chunk%d.npz" % chunk))
    code = "import test_gpu_recommend_star as t; t.chunk_case(%r)" % path
    env = dict(os.environ, MAMDR_REC_CHUNK=str(chunk),
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(_CACHE["one_chunk"]) as a, np.load(path) as b:
        assert sorted(a.files) == sorted(b.files) and len(a.files) == 9
        for name in a.files:
            assert a[name].tobytes() == b[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("tower", ["star", "mlp"])
def test_a_second_query_block_changes_no_byte(star_engines, tower):
    """300 users in one domain = query blocks of 256 + 44: every row of ids, scores and dense scores is the bytes of a
    call with that user alone."""
    eng = star_engines(False) if tower == "star" else base.make_engine("mlp", False)[0]
    uids = np.random.RandomState(13).choice(1188, 300, replace=False).astype(np.int32)
    ids, scores, all_scores = eng.recommend_domain(uids, 3, 10, want_scores=True)
    assert ids.shape == (300, 10) and all_scores.shape == (300, 346) and np.all(ids >= 0)
    for q in range(300):
        i1, s1, a1 = eng.recommend_domain(uids[q:q + 1], 3, 10, want_scores=True)
        assert i1.tobytes() == ids[q].tobytes() and s1.tobytes() == scores[q].tobytes() \
            and a1.tobytes() == all_scores[q].tobytes(), q
    if tower == "star":          # ... and rows behind the first block are scores of the right users
        ref = oracle_scores(star_params(), star_state(star_params()), uids[[0, 255, 256, 299]], np.arange(346), 3)
        np.testing.assert_allclose(all_scores[[0, 255, 256, 299]], ref, rtol=RTOL, atol=ATOL)
    else:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
@pytest.mark.parametrize("tower", base.TOWERS)
def test_one_domain_is_the_broadcast_of_recommend(tower, trainable):
    """mlp / wdl / deepfm: recommend_domain(u, d, ...) returns the bytes of recommend(u, [d] * Q, ...)."""
    eng = base.make_engine(tower, trainable)[0]
    uids = users7()
    cand = base.candidate_list(True)
    excl = base.exclusion_lists(base.reference(tower, trainable), cand)
    for d, k, kw in ((3, 10, {}), (9, 128, dict(exclude=excl[:7], candidates=cand)), (0, 1, dict(candidates=cand))):
        one = eng.recommend_domain(uids, d, k, want_scores=True, **kw)
        vec = eng.recommend(uids, [d] * uids.size, k, want_scores=True, **kw)
        assert all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(one, vec)), (d, k)
        assert np.all(one[0][:, 0] >= 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def state_digest(eng):
    from mamdr_amd import _lib
    h = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (eng.weights, eng.adam_m, eng.adam_v, eng.aux)]
    return h + [int(eng.lib.mamdr_optimizer_steps(eng.ctx)), int(eng.lib.mamdr_dropout_steps(eng.ctx))] + \
        [int(_lib.load().mamdr_pregather_hits(eng.ctx))]


def test_recommend_domain_reads_the_state_only():
    """twin Star engines with trainable tables: a retrieves in domain 3 between training calls on another domain --
    multi-step calls (their effective block and lazily replayed slices), a single-step call, a call starting mid-pass --,
    b never retrieves: weights, both Adam slots, aux and the counters end equal."""
    g = base.gen()
    sizes = [g["data"]["train"][i]["uid"].shape[0] for i in range(10)]
    d = max((i for i in range(10) if i != 3), key=lambda i: sizes[i])
    assert -(-sizes[d] // 256) >= 4
    uids = users7()
    a = make_star_engine(True, bind=(d,))[0]
    b = make_star_engine(True, bind=(d,))[0]
    a.train_steps(d, n_steps=2)
    b.train_steps(d, n_steps=2)
    before = state_digest(a)
    assert before == state_digest(b)
    first = a.recommend_domain(uids, 3, 10, want_scores=True)
    assert state_digest(a) == before
    again = a.recommend_domain(uids, 3, 10, want_scores=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    for first_step, n_steps in ((2, 1), (1, 2), (3, 1), (0, 3)):
        a.train_steps(d, first_step=first_step, n_steps=n_steps)
        a.recommend_domain(uids, 3, 128, exclude=[[1, 2]] * 7)
        if n_steps == 1:
            a.recommend_domain(uids[:1], 3, 1, candidates=[5, 6, 7])
        b.train_steps(d, first_step=first_step, n_steps=n_steps)
    assert state_digest(a) == state_digest(b)
    assert state_digest(a) != before
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_after_training_the_live_state_is_scored():
    """trainable tables, three Adam steps on domain d in one call, then recommend_domain at once -- in d (its moving
    statistics, its stepped slices, lagging table rows) and in another domain (slices replayed at the call's end) --
    against the oracle trained on the same batches."""
    g = base.gen()
    sizes = [g["data"]["train"][i]["uid"].shape[0] for i in range(10)]
    d = max(range(10), key=lambda i: sizes[i])
    other = 3 if d != 3 else 0
    eng, params, state = make_star_engine(True, bind=(d,))
    model = ostar.OracleStar({k: v.copy() for k, v in params.items()}, emb_trainable=True, lr=1e-3)
    model.state = {k: v.copy() for k, v in state.items()}
    assert eng.train_steps(d, n_steps=3, lr=1e-3) == 3
    uids = users7()
    got = {dom: eng.recommend_domain(uids, dom, 10, want_scores=True) for dom in (d, other)}
    eng.close()
    c = g["data"]["train"][d]
    for s in range(3):
        sl = slice(256 * s, 256 * (s + 1))
        model.train_on_batch(c["uid"][sl], c["pid"][sl], c["domain"][sl], c["label"][sl])
    start = star_params()
    for dom in (d, other):
        ref = oracle_scores(model.params, model.state, uids, np.arange(346), dom)
        before = oracle_scores(start, state, uids, np.arange(346), dom)
        err = np.abs(got[dom][2] - ref) / (ATOL_TRAINED + RTOL_TRAINED * np.abs(ref))
        print("star after 3 Adam steps on domain %d, retrieval in domain %d: worst |err| / bar = %.4f; training moved the "
              "scores by up to %.3e" % (d, dom, err.max(), np.abs(ref - before).max()))
        np.testing.assert_allclose(got[dom][2], ref, rtol=RTOL_TRAINED, atol=ATOL_TRAINED)
        assert np.abs(ref - before).max() > 1e-3               # ... and training did change the scores
        ids, scores, all_scores = got[dom]
        for q in range(7):
            assert np.array_equal(np.sort(all_scores[q])[::-1][:10], scores[q]) and np.unique(ids[q]).size == 10
            assert np.array_equal(all_scores[q, ids[q]], scores[q])


# ---------------------------------------------------------------------------------------------------------------- 9
def test_refusals(star_engines):
    import ctypes as C
    from mamdr_amd import _lib
    from mamdr_amd.engine import TowerEngine
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    uids = users7()
    for tower in ("pnn", "nfm"):
        eng = TowerEngine(1188, 346, 10, 256, tower=tower)
        with pytest.raises(_lib.NotBuiltError, match=r"\b%s tower" % tower):
            eng.recommend_domain(uids, 3, 10)
        eng.close()
    eng = star_engines(False)
    for k in (0, 129):
        with pytest.raises(_lib.MamdrError) as e:
            eng.recommend_domain(uids, 3, k)
        assert e.value.code == _lib.EINVAL and "k %d" % k in str(e.value)
    launched = []
    real = eng.lib.mamdr_recommend_domain
    try:
        eng.lib.mamdr_recommend_domain = lambda *a: launched.append(a) or 0
        for bad in (-1, 10):
            with pytest.raises(ValueError):
                eng.recommend_domain(uids, bad, 5)
        for bad in ([1188], [-1]):
            with pytest.raises(ValueError):
                eng.recommend_domain(bad, 3, 5)
        with pytest.raises(ValueError):
            eng.recommend_domain([0], 3, 5, candidates=[346])
        with pytest.raises(ValueError):
            eng.recommend_domain([0], 3, 5, candidates=[3, 3])
        with pytest.raises(ValueError):
            eng.recommend_domain([0], 3, 5, exclude=[[1], [2]])
    finally:
        eng.lib.mamdr_recommend_domain = real
    assert not launched                                        # refused on the host, before any launch
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out_i = torch.zeros(10, dtype=torch.int32, device=eng.device)
    out_f = torch.zeros(10, dtype=torch.float32, device=eng.device)
    q = torch.zeros(1, dtype=torch.int32, device=eng.device)
    for bad in (-1, 10):
        assert real(eng.ctx, bad, 1, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
        assert b"domain %d" % bad in eng.lib.mamdr_last_error()
    assert real(eng.ctx, 3, 0, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    assert real(eng.ctx, 3, 1, None, None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.OK
    raw = TowerEngine(1188, 346, 10, 256, tower="star")        # frozen tables, none bound
    assert real(raw.ctx, 3, 1, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.ESTATE
    assert real(raw.ctx, 10, 1, p(q), None, 0, None, None, 10, p(out_i), p(out_f), None) == _lib.EINVAL
    raw.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_run_config_with_recommend_on_star(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 Star config (sized as test_gpu_recommend.py's test_run_config_with_recommend
    sizes its run) with --recommend 10: the step engine, the .npz over all 10 domains, no seen item returned, metrics
    inside [0, 1].  No quality bar."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "star_taobao.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["train"].update(epoch=3, patience=1, result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
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
            assert np.all(np.isfinite(scores)) and np.all(np.diff(scores, axis=1) <= 0)
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
