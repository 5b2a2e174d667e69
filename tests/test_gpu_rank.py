"""Exact ranks of target items on the device (mamdr_rank_domain, TowerEngine.rank_domain, BaseModel.rank_eval,
run.py --rank-eval) against the complete orderings mamdr_recommend_domain returns for candidate lists of at most 128 items,
and against oracle/tower.py's scores.

Problem: tests/test_gpu_recommend.py's -- 1,188 users, 346 items, 10 domains: 346 candidates are five 64-wide tiles plus a
remainder of 26.  Every query in domain 3.  The 346 items are partitioned into three disjoint candidate lists of 128, 128
and 90 ids: for each, recommend_domain(k = 128) is the COMPLETE order of the live candidates, so a listed target's rank
must be its position there; a rank over all 346 candidates is the sum of the three.

Targets per query: the oracle's best three items, its worst, 20 random ones (unsorted, with a duplicate); query 2 has
none, query 5 has 70 (more than a tile of the pair pre-pass).
"""
import copy
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_recommend as base            # noqa: E402  (the problem, the engines, the exclusion lists)
import test_gpu_recommend_star as sbase      # noqa: E402  (the Star engine and its digest)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = base.RTOL, base.ATOL            # the project's prediction bar: rtol 2e-5 / atol 2e-7
DOMAIN = 3
CASES = [("mlp", False), ("deepfm", True)]
CASE_IDS = ["mlp-frozen", "deepfm-trainable"]
ALL = np.arange(346, dtype=np.int32)

_REF = {}
engines = base.engines          # the module-scoped fixture of test_gpu_recommend.py: one engine per (tower, trainable)


def users7():
    return base.queries()[0]


def reference(tower, trainable):
    """the oracle's scores of the 7 users over all 346 items in domain 3: computed once, never modified."""
    if (tower, trainable) not in _REF:
        ref = base.oracle_scores(base.make_params(trainable), tower, trainable, ALL, users7(), [DOMAIN] * 7)
        ref.setflags(write=False)
        _REF[(tower, trainable)] = ref
    return _REF[(tower, trainable)]


def parts():
    perm = np.random.RandomState(21).permutation(346).astype(np.int32)
    return [perm[:128], perm[128:256], perm[256:]]


def target_lists(ref):
    rs = np.random.RandomState(17)
    out = []
    for q in range(ref.shape[0]):
        order = np.argsort(-ref[q], kind="stable")
        t = np.concatenate([order[:3], order[-1:], rs.choice(346, 70 if q == 5 else 20, replace=False), order[:1]])
        out.append([] if q == 2 else rs.permutation(t))
    return out


def csr_rows(res):
    off = res["offsets"]
    return [(q, slice(off[q], off[q + 1])) for q in range(off.size - 1)]


def expected_listed(res, cand, excl):
    want = np.zeros(res["ids"].size, bool)
    for q, sl in csr_rows(res):
        ex = np.asarray(excl[q], np.int64) if excl is not None else np.zeros(0, np.int64)
        want[sl] = np.isin(res["ids"][sl], cand) & ~np.isin(res["ids"][sl], ex)
    return want


def check_against_complete_order(eng, uids, domain, targets, cand, excl):
    """check 1 of one candidate list of at most 128 ids -> the rank_domain result."""
    assert cand.size <= 128
    ids = eng.recommend_domain(uids, domain, 128, candidates=cand, exclude=excl)[0]
    res = eng.rank_domain(uids, domain, targets, candidates=cand, exclude=excl, want_scores=True)
    assert res["ranks"].dtype == np.int32 and res["live"].dtype == np.int32 and res["listed"].dtype == bool
    assert np.array_equal(res["listed"], expected_listed(res, cand, excl))
    n_listed = 0
    for q, sl in csr_rows(res):
        ex = np.unique(np.asarray(excl[q], np.int64)) if excl is not None else np.zeros(0, np.int64)
        assert res["live"][q] == cand.size - np.isin(ex, cand).sum() == (ids[q] >= 0).sum(), q
        assert np.array_equal(res["ids"][sl], np.unique(np.asarray(targets[q], np.int64))), q
        for j in range(sl.start, sl.stop):
            if res["listed"][j]:
                pos = np.nonzero(ids[q] == res["ids"][j])[0]
                assert pos.size == 1 and res["ranks"][j] == pos[0], (q, res["ids"][j], res["ranks"][j], pos)
                n_listed += 1
            assert 0 <= res["ranks"][j] <= res["live"][q]
    assert n_listed > 0
    return res


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("with_excl", [False, True], ids=["noexcl", "excl"])
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_rank_is_the_position_in_the_complete_order(engines, tower, trainable, with_excl):
    ref = reference(tower, trainable)
    targets = target_lists(ref)
    for cand in parts():
        excl = base.exclusion_lists(ref, cand) if with_excl else None
        check_against_complete_order(engines(tower, trainable), users7(), DOMAIN, targets, cand, excl)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_ranks_add_up_over_a_partition(engines, tower, trainable):
    """a target outside a list is still counted against that list, so rank(all 346) = the sum of the three ranks, exactly;
    below 128 the rank over all 346 is the position in the full list's top 128."""
    eng = engines(tower, trainable)
    ref = reference(tower, trainable)
    targets = target_lists(ref)
    excl = base.exclusion_lists(ref, ALL)
    uids = users7()
    full = eng.rank_domain(uids, DOMAIN, targets, exclude=excl)
    assert np.diff(full["offsets"]).tolist() == [np.unique(t).size for t in targets]
    assert np.diff(full["offsets"])[2] == 0 and np.diff(full["offsets"])[5] > 64
    total, live = np.zeros_like(full["ranks"]), np.zeros_like(full["live"])
    for cand in parts():
        r = eng.rank_domain(uids, DOMAIN, targets, candidates=cand, exclude=excl)
        assert np.array_equal(r["ids"], full["ids"]) and np.array_equal(r["offsets"], full["offsets"])
        total += r["ranks"]
        live += r["live"]
    assert np.array_equal(full["ranks"], total) and np.array_equal(full["live"], live)
    assert np.array_equal(full["listed"], expected_listed(full, ALL, excl))
    ids = eng.recommend_domain(uids, DOMAIN, 128, exclude=excl)[0]
    seen = 0
    for q, sl in csr_rows(full):
        for j in range(sl.start, sl.stop):
            if full["listed"][j] and full["ranks"][j] < 128:
                assert ids[q, full["ranks"][j]] == full["ids"][j], (q, j)
                seen += 1
            elif full["listed"][j]:
                assert full["ids"][j] not in ids[q]
    assert seen > 20
    again = eng.rank_domain(uids, DOMAIN, targets, exclude=excl)
    assert all(again[n].tobytes() == full[n].tobytes() for n in ("ranks", "live"))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_rank_lies_in_the_oracles_band(engines, tower, trainable):
    """#{ref_c > ref_t + tol} <= rank <= #{ref_c >= ref_t - tol, c != t} over the live candidates c, tol = ATOL + RTOL |ref_t|
    at the project's prediction bar -- compared on the scores, as check_topk compares (the sigmoid is monotone: the order
    of the logits is the order of the scores up to that bar)."""
    ref = reference(tower, trainable)
    targets = target_lists(ref)
    excl = base.exclusion_lists(ref, ALL)
    res = engines(tower, trainable).rank_domain(users7(), DOMAIN, targets, exclude=excl)
    worst = 0
    for q, sl in csr_rows(res):
        livec = ~np.isin(ALL, np.asarray(excl[q], np.int64))
        for j in range(sl.start, sl.stop):
            t = res["ids"][j]
            x, tol = ref[q, t], base.tol(ref[q, t])
            lo = int((ref[q, livec] > x + tol).sum())
            hi = int(((ref[q] >= x - tol) & livec & (ALL != t)).sum())
            worst = max(worst, hi - lo)
            assert lo <= res["ranks"][j] <= hi, (q, t, lo, res["ranks"][j], hi)
    print("%s: widest band %d ranks" % (tower, worst))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_scores_are_the_dense_matrix_entries_bit_for_bit(engines, tower, trainable):
    eng = engines(tower, trainable)
    ref = reference(tower, trainable)
    targets = target_lists(ref)
    cand = base.candidate_list(True)
    excl = base.exclusion_lists(ref, cand)
    all_scores = eng.recommend_domain(users7(), DOMAIN, 10, candidates=cand, exclude=excl, want_scores=True)[2]
    res = eng.rank_domain(users7(), DOMAIN, targets, candidates=cand, exclude=excl, want_scores=True)
    assert res["scores"].dtype == np.float32 and res["scores"].shape == res["ranks"].shape
    n = 0
    for q, sl in csr_rows(res):
        for j in range(sl.start, sl.stop):
            if res["listed"][j]:
                pos = int(np.nonzero(cand == res["ids"][j])[0][0])
                assert res["scores"][j:j + 1].view(np.uint32)[0] == all_scores[q, pos:pos + 1].view(np.uint32)[0], (q, j)
                n += 1
    assert n > 50 and not res["listed"].all()
    np.testing.assert_allclose(res["scores"], np.concatenate([ref[q, res["ids"][sl]] for q, sl in csr_rows(res)]),
                               rtol=RTOL, atol=ATOL)                   # ... the unlisted targets' scores included


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("tower", ["mlp", "deepfm"])
def test_exact_ties_rank_by_id(tower):
    """every item row identical (test_exact_ties_rank_by_id_wherever_the_pair_sits' construction): one logit per query, so
    a target's rank is the number of live candidates of smaller id -- consecutive ranks in ascending id order, a target
    never behind a larger id of its tie, whatever tile and lane the pair sits in (the candidates are shuffled)."""
    params = base.make_params(False)
    params["item_emb"] = np.repeat(params["item_emb"][17:18], 346, axis=0)
    eng, _ = base.make_engine(tower, False, params)
    cand = np.random.RandomState(9).permutation(346).astype(np.int32)
    excl = [[0, 3, 4, 300]] * 3 + [[]] * 4
    targets = [[345, 0, 1, 2, 3, 5, 64, 63, 300, 301, 128]] * 6 + [list(range(346))]
    res = eng.rank_domain(users7(), DOMAIN, targets, candidates=cand, exclude=excl, want_scores=True)
    sub = eng.rank_domain(users7(), DOMAIN, targets, candidates=cand[:100], exclude=excl)
    eng.close()
    for q, sl in csr_rows(res):
        livec = np.setdiff1d(np.arange(346), excl[q])
        want = [int((livec < t).sum()) for t in res["ids"][sl]]
        assert res["ranks"][sl].tolist() == want, (q, res["ranks"][sl], want)
        assert res["live"][q] == livec.size
        assert np.unique(res["scores"][sl].view(np.uint32)).size == 1
        lives = np.setdiff1d(cand[:100], excl[q])
        assert sub["ranks"][sl].tolist() == [int((lives < t).sum()) for t in sub["ids"][sl]], q
    q6 = res["ranks"][res["offsets"][6]:]
    assert q6.tolist() == list(range(346))


# ---------------------------------------------------------------------------------------------------------------- 6
def chunk_case(tower, trainable, path):
    """the calls of the chunking test, dumped to `path` (run in the test's process and in its children)."""
    eng, _ = base.make_engine(tower, trainable)
    ref = reference(tower, trainable)
    targets = target_lists(ref)
    out = {}
    for subset in (False, True):
        cand = base.candidate_list(subset)
        res = eng.rank_domain(users7(), DOMAIN, targets, candidates=cand if subset else None,
                              exclude=base.exclusion_lists(ref, cand), want_scores=True)
        out.update({"ranks_%d" % subset: res["ranks"], "live_%d" % subset: res["live"], "scores_%d" % subset: res["scores"]})
    eng.close()
    np.savez(path, **out)


@pytest.mark.parametrize("chunk", [64, 128])
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_chunking_does_not_change_a_bit(tmp_path_factory, tower, trainable, chunk):
    """MAMDR_REC_CHUNK = 64 / 128 in a fresh child process (the switch is read at load): six / three candidate chunks, and
    as many passes of the target pre-pass over the ~190 targets -- ranks, live counts and score bits are those of the
    default (one chunk) run."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    key = ("one_chunk", tower, trainable)
    if key not in _REF:
        _REF[key] = str(tmp_path_factory.mktemp("rank_chunks") / "one.npz")
        chunk_case(tower, trainable, _REF[key])
    path = str(tmp_path_factory.mktemp("rank_chunks") / ("chunk%d.npz" % chunk))
    code = "import test_gpu_rank as t; t.chunk_case(%r, %r, %r)" % (tower, trainable, path)
    env = dict(os.environ, MAMDR_REC_CHUNK=str(chunk),
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(_REF[key]) as a, np.load(path) as b:
        assert sorted(a.files) == sorted(b.files) and len(a.files) == 6
        for name in a.files:
            assert a[name].size and a[name].tobytes() == b[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- 7
def test_a_second_query_block_changes_no_byte(engines):
    """300 users = query blocks of 256 + 44, between 0 and 6 targets each: queries 256 .. 299 give the bytes they give
    when called alone (their targets sit behind the first block's in the flat list), and so do single queries."""
    eng = engines("mlp", False)
    rs = np.random.RandomState(13)
    uids = rs.choice(1188, 300, replace=False).astype(np.int32)
    targets = [rs.choice(346, q % 7, replace=False) for q in range(300)]
    excl = [rs.choice(346, 5 * (q % 3), replace=False) for q in range(300)]
    res = eng.rank_domain(uids, DOMAIN, targets, exclude=excl, want_scores=True)
    assert res["offsets"][-1] == sum(q % 7 for q in range(300)) and res["live"].tolist() == [346 - 5 * (q % 3) for q in range(300)]
    tail = eng.rank_domain(uids[256:], DOMAIN, targets[256:], exclude=excl[256:], want_scores=True)
    t0 = res["offsets"][256]
    assert tail["offsets"].tolist() == (res["offsets"][256:] - t0).tolist()
    for n in ("ids", "ranks", "listed", "scores"):
        assert tail[n].tobytes() == res[n][t0:].tobytes(), n
    assert tail["live"].tobytes() == res["live"][256:].tobytes()
    for q in (0, 6, 255, 256, 299):
        one = eng.rank_domain(uids[q:q + 1], DOMAIN, targets[q:q + 1], exclude=excl[q:q + 1], want_scores=True)
        sl = slice(res["offsets"][q], res["offsets"][q + 1])
        assert one["ranks"].tobytes() == res["ranks"][sl].tobytes() and one["scores"].tobytes() == res["scores"][sl].tobytes(), q
        assert one["live"][0] == res["live"][q]
    # a call without any target produces the live counts alone
    none = eng.rank_domain(uids[:9], DOMAIN, [[]] * 9, exclude=excl[:9])
    assert none["ranks"].size == 0 and none["live"].tolist() == res["live"][:9].tolist()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("domain", [0, 3])
def test_star(domain):
    """the Star tower (sbase.make_star_engine: domains 0 and 3 carry moving statistics of their own): checks 1 and 4."""
    eng = sbase.make_star_engine(True)[0]
    ref = sbase.reference(domain)
    targets = target_lists(ref)
    uids = users7()
    for i, cand in enumerate(parts()):
        excl = base.exclusion_lists(ref, cand) if i != 1 else None
        res = check_against_complete_order(eng, uids, domain, targets, cand, excl)
        all_scores = eng.recommend_domain(uids, domain, 10, candidates=cand, exclude=excl, want_scores=True)[2]
        for q, sl in csr_rows(res):
            for j in range(sl.start, sl.stop):
                if res["listed"][j]:
                    pos = int(np.nonzero(cand == res["ids"][j])[0][0])
                    assert res["scores"][j:j + 1].view(np.uint32)[0] == all_scores[q, pos:pos + 1].view(np.uint32)[0], (q, j)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("tower", ["deepfm", "star"])
def test_rank_domain_reads_the_state_only(tower):
    """twin engines with trainable tables: a ranks in domain 3 between training calls on another domain -- single-step,
    multi-step and mid-pass calls --, b never does: weights, both Adam slots, the counters (Star: and the moving
    statistics) end equal."""
    g = base.gen()
    sizes = [g["data"]["train"][i]["uid"].shape[0] for i in range(10)]
    d = max((i for i in range(10) if i != DOMAIN), key=lambda i: sizes[i])
    assert -(-sizes[d] // 256) >= 4
    if tower == "star":
        make, digest = (lambda: sbase.make_star_engine(True, bind=(d,))[0]), sbase.state_digest
    else:
        make, digest = (lambda: base.make_engine(tower, True, bind=(d,))[0]), base.state_digest
    a, b = make(), make()
    uids = users7()
    targets = [[1, 2, 3, 340]] * 6 + [[]]
    a.train_steps(d, n_steps=2)
    b.train_steps(d, n_steps=2)
    before = digest(a)
    assert before == digest(b)
    first = a.rank_domain(uids, DOMAIN, targets, want_scores=True)
    assert digest(a) == before
    again = a.rank_domain(uids, DOMAIN, targets, want_scores=True)
    assert all(first[n].tobytes() == again[n].tobytes() for n in ("ranks", "live", "scores"))
    for first_step, n_steps in ((2, 1), (1, 2), (3, 1), (0, 3)):
        a.train_steps(d, first_step=first_step, n_steps=n_steps)
        a.rank_domain(uids, DOMAIN, targets, exclude=[[1, 2]] * 7)
        if n_steps == 1:
            a.rank_domain(uids[:1], DOMAIN, [[5]], candidates=[5, 6, 7])
        b.train_steps(d, first_step=first_step, n_steps=n_steps)
    assert digest(a) == digest(b)
    assert digest(a) != before
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_refusals(engines):
    from mamdr_amd import _lib, graph_engine
    from mamdr_amd.engine import TowerEngine
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    uids = users7()
    targets = [[1, 2]] * 7
    for tower in ("pnn", "nfm"):
        eng = TowerEngine(1188, 346, 10, 256, tower=tower)
        with pytest.raises(_lib.NotBuiltError, match=r"\b%s tower" % tower):
            eng.rank_domain(uids, DOMAIN, targets)
        eng.close()
    geng = graph_engine.GraphEngine("mlp", 1188, 346, 10, 256, (128, 64), (), emb_dim=64)
    with pytest.raises(NotImplementedError, match="generic-layer towers"):
        geng.rank_domain(uids, DOMAIN, targets)
    geng.close()
    eng = engines("mlp", False)
    launched = []
    real = eng.lib.mamdr_rank_domain
    try:
        eng.lib.mamdr_rank_domain = lambda *a: launched.append(a) or 0
        for bad in (-1, 10, 3.0, True):
            with pytest.raises(ValueError):
                eng.rank_domain(uids, bad, targets)
        for bad in ([[346]] * 7, [[-1]] * 7, [[1]] * 6, [[1]] * 8):          # a target id out of range; a mismatched length
            with pytest.raises(ValueError):
                eng.rank_domain(uids, DOMAIN, bad)
        with pytest.raises(ValueError):
            eng.rank_domain([1188], DOMAIN, [[1]])
        with pytest.raises(ValueError):
            eng.rank_domain([0], DOMAIN, [[1]], candidates=[346])
        with pytest.raises(ValueError):
            eng.rank_domain([0], DOMAIN, [[1]], candidates=[3, 3])
        with pytest.raises(ValueError):
            eng.rank_domain([0], DOMAIN, [[1]], exclude=[[1], [2]])
    finally:
        eng.lib.mamdr_rank_domain = real
    assert not launched                                        # refused on the host, before any launch
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    q = torch.zeros(1, dtype=torch.int32, device=eng.device)
    off = torch.tensor([0, 1], dtype=torch.int64, device=eng.device)
    tid = torch.tensor([5], dtype=torch.int32, device=eng.device)
    rank = torch.full((4,), -7, dtype=torch.int32, device=eng.device)
    live = torch.full((4,), -7, dtype=torch.int32, device=eng.device)
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, p(off), p(tid), p(rank), None, p(live)) == _lib.OK
    assert rank.tolist()[1:] == [-7] * 3 and live.tolist() == [346, -7, -7, -7] and 0 <= rank.tolist()[0] < 346
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, None, p(tid), p(rank), None, p(live)) == _lib.EINVAL
    assert b"mamdr_rank_domain" in eng.lib.mamdr_last_error()
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, p(off), p(tid), None, None, p(live)) == _lib.EINVAL
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, p(off), p(tid), p(rank), None, None) == _lib.EINVAL
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, p(off), None, p(rank), None, p(live)) == _lib.EINVAL      # targets exist
    assert real(eng.ctx, 3, 1, None, None, 0, None, None, p(off), p(tid), p(rank), None, p(live)) == _lib.EINVAL
    assert real(eng.ctx, 3, 0, p(q), None, 0, None, None, p(off), p(tid), p(rank), None, p(live)) == _lib.EINVAL
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, C.c_void_p(off.data_ptr() + 4), p(tid), p(rank), None, p(live)) == _lib.EINVAL
    late = torch.tensor([1, 2], dtype=torch.int64, device=eng.device)                                    # offsets start at 1
    assert real(eng.ctx, 3, 1, p(q), None, 0, None, None, p(late), p(tid), p(rank), None, p(live)) == _lib.EINVAL
    for bad in (-1, 10):
        assert real(eng.ctx, bad, 1, p(q), None, 0, None, None, p(off), p(tid), p(rank), None, p(live)) == _lib.EINVAL
        assert b"domain %d" % bad in eng.lib.mamdr_last_error()
    raw = TowerEngine(1188, 346, 10, 256)                      # frozen tables, none bound
    assert real(raw.ctx, 3, 1, p(q), None, 0, None, None, p(off), p(tid), p(rank), None, p(live)) == _lib.ESTATE
    raw.close()


# ---------------------------------------------------------------------------------------------------------------- 11
def run_config(tmp_path, name, ks):
    from mamdr_amd import cli
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name)
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5, rank_eval=ks,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    return cfg, built[0]


def test_run_config_with_rank_eval(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 config as a plain mlp (sized as test_run_config_with_recommend) with
    train.rank_eval = [10, 128]: the .npz is complete, and HitRate / Recall / NDCG @10 and @128 are those of
    recommend.ranking_metrics over model.recommend(d, K) -- the same weights, two routes."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine, recommend
    cfg, model = run_config(tmp_path, "mlp", [10, 128])
    assert isinstance(model.model, engine.TowerEngine)
    text = capsys.readouterr().out
    assert "Rank eval" in text and text.count("MRR ") == 10 and text.count("NDCG@128") == 10
    ds = model.dataset
    with np.load(os.path.join(model.result_path, "rank_eval.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and z["ks"].tolist() == [10, 128]
        assert z["mrr"].shape == z["mean_percentile"].shape == (10,) and np.all((z["mrr"] >= 0) & (z["mrr"] <= 1))
        assert z["mrr"].max() > 0
        assert np.all((z["mean_percentile"] >= 0) & (z["mean_percentile"] <= 1))
        for d in range(10):
            users, offsets = z["users_%d" % d], z["offsets_%d" % d]
            ids, ranks, listed, live = z["ids_%d" % d], z["ranks_%d" % d], z["listed_%d" % d], z["live_%d" % d]
            assert np.array_equal(users, np.unique(ds.test_dataset[d]["data"]["uid"]))
            assert offsets.shape == (users.size + 1,) and offsets[-1] == ids.size == ranks.size == listed.size
            assert live.shape == (users.size,) and np.all(ranks[listed] < np.repeat(live, np.diff(offsets))[listed])
            for i, k in enumerate((10, 128)):
                r = model.recommend(d, k)
                assert np.array_equal(r["users"], users)
                m = recommend.ranking_metrics(r["ids"], recommend.split_positives(ds, d, users))
                for name in ("hit_rate", "recall", "ndcg"):
                    assert abs(z[name][d, i] - m[name]) <= 1e-12, (d, k, name, z[name][d, i], m[name])
                # ... and target by target: a listed target of rank r < k is the r-th id of the list
                for q in range(users.size):
                    for j in range(offsets[q], offsets[q + 1]):
                        if listed[j] and ranks[j] < k:
                            assert r["ids"][q, ranks[j]] == ids[j], (d, q, j)
                        else:
                            assert ids[j] not in r["ids"][q], (d, q, j)
    print(text[text.index("Rank eval"):])


def test_rank_eval_ranks_a_domain_under_its_own_merged_weights(tmp_path):
    """mlp_meta_mamdr: rank_eval(d) is engine.rank_domain after installing merge(best theta, best phi_d) by hand, and it
    leaves the live flat vector as it found it."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import recommend
    cfg, model = run_config(tmp_path, "mlp_meta_mamdr", [10])
    eng = model.model
    digest = lambda: hashlib.sha256(eng.weights.cpu().numpy().tobytes()).hexdigest()      # noqa: E731
    before = digest()
    got = {d: model.rank_eval(d) for d in (0, 4, 9)}
    assert digest() == before
    keep = eng.get_weights().clone()
    differs = 0
    for d, r in got.items():
        catalogue, users, exclude = model._retrieval_problem(d, None, True)
        targets = recommend.split_positives(model.dataset, d, users)
        as_live = eng.rank_domain(users, d, targets, candidates=catalogue, exclude=exclude)
        merged = eng.new_vector(meta=True)
        eng.merge(merged, model.best_shared_weights, model.best_domain_weights[d], cfg["train"]["merged_method"])
        eng.assign_meta(merged)
        by_hand = eng.rank_domain(users, d, targets, candidates=catalogue, exclude=exclude)
        eng.set_weights(keep)
        for n in ("offsets", "ids", "ranks", "listed", "live"):
            assert by_hand[n].tobytes() == r[n].tobytes(), (d, n)
        assert np.array_equal(r["users"], users) and np.array_equal(r["catalogue"], catalogue)
        assert np.array_equal(r["n_positives"], np.diff(r["offsets"]))
        differs += int(not np.array_equal(as_live["ranks"], r["ranks"]))
    assert digest() == before
    print("domains whose ranks under the live weights differ from those under their own merged weights: %d of 3" % differs)
