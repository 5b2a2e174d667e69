"""Top-K lists, exact ranks and slates from the generic-layer engine's single-output towers (mamdr_graph_recommend,
_recommend_domain, _rank_domain, _rank_slates; GraphEngine's four retrieval methods) against the oracles' `predict` over
explicit (user, item, domain) triples.

Problem: tests/test_gpu_recommend.py's -- synthetic.generate("taobao10", batch_size=256, seed=7, scale=0.05): 1,188 users, 346
items, 10 domains, max_batch 256.  346 candidates are five 64-key tiles plus a remainder of 26; seven queries x 384 padded rows
are 10.5 forward batches of 256 rows, so the padded last batch is exercised.  Weights and oracles as
tests/test_gpu_fmnets.py:make_problem and tests/test_gpu_embdim.py:make_problem set them up.

The score bar is the project's for evaluation predictions at equal weights: rtol 2e-5, atol 2e-7.
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

import test_gpu_embdim as emb           # noqa: E402
import test_gpu_fmnets as fm            # noqa: E402
from test_gpu_recommend import (ATOL, RTOL, candidate_list, check_topk, exclusion_lists, queries, tol)      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEM = 346
DOMAIN = 3
# case -> (kind, emb_dim, hidden): the four towers of test_gpu_fmnets at hidden (256, 128, 64), E 128; three of test_gpu_embdim's
CASES = {"nfm": ("nfm", 128, fm.HIDDEN), "pnn": ("pnn", 128, fm.HIDDEN), "ccpm": ("ccpm", 128, fm.HIDDEN),
         "autoint": ("autoint", 128, fm.HIDDEN), "mlp64": ("mlp", 64, (128, 64)), "deepfm32": ("deepfm", 32, (64,)),
         "wdl256": ("wdl", 256, (128, 64, 64, 64))}

_REF = {}


def make_case(case, trainable, mutate=None):
    """(g, engine, oracle) of a case; `mutate(params)` changes the weights of both before they are installed."""
    kind, e, hidden = CASES[case]
    if e == 128 and kind not in ("mlp", "wdl", "deepfm"):
        g, eng, model = fm.make_problem(kind, emb_trainable=trainable)
    else:
        g, eng, model = emb.make_problem(kind, e, hidden, emb_trainable=trainable)
    assert (g["n_user"], g["n_item"], g["n_domain"]) == (1188, N_ITEM, 10)
    eng.enable_retrieval()              # (mlp / wdl / deepfm: a bare engine of these kinds serves the calls once asked to)
    if mutate is not None:
        mutate(model.params)
        if not trainable:
            eng.bind_table("user_emb", model.params["user_emb"])
            eng.bind_table("item_emb", model.params["item_emb"])
        eng.set_weights(eng.pack(model.params))
    return g, eng, model


@pytest.fixture(scope="module")
def cases():
    """one engine per (case, trainable) for the tests that only read it."""
    made = {}

    def get(case, trainable):
        if (case, trainable) not in made:
            made[(case, trainable)] = make_case(case, trainable)
        return made[(case, trainable)]
    yield get
    for _, eng, _ in made.values():
        eng.close()


def oracle_scores(model, uids, doms, cand):
    cand = np.asarray(cand, np.int32)
    return np.stack([model.predict(np.full(cand.size, u, np.int32), cand, np.full(cand.size, d, np.int32))
                     for u, d in zip(uids, doms)])


def reference(cases, case, trainable, doms=None):
    """the oracle's scores of the 7 queries over all 346 items: computed once per case, never modified."""
    key = (case, trainable, None if doms is None else int(doms[0]))
    if key not in _REF:
        uids, qd = queries()
        ref = oracle_scores(cases(case, trainable)[2], uids, qd if doms is None else doms, np.arange(N_ITEM))
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("trainable", [False, True], ids=["frozen", "trainable"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_scores_match_oracle(cases, case, trainable):
    eng = cases(case, trainable)[1]
    uids, doms = queries()
    ids, scores, all_scores = eng.recommend(uids, doms, 10, want_scores=True)
    ref = reference(cases, case, trainable)
    assert all_scores.shape == ref.shape == (7, N_ITEM) and all_scores.dtype == np.float32
    err = np.abs(all_scores - ref) / (ATOL + RTOL * np.abs(ref))
    print("%s %s: worst |err| / bar = %.4f" % (case, "trainable" if trainable else "frozen", err.max()))
    np.testing.assert_allclose(all_scores, ref, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 2
TOPK_CASES = [("ccpm", False), ("deepfm32", True)]
TOPK_IDS = ["ccpm-frozen", "deepfm32-trainable"]


@pytest.mark.parametrize("subset", [False, True], ids=["all346", "subset201"])
@pytest.mark.parametrize("with_excl", [False, True], ids=["noexcl", "excl"])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("case,trainable", TOPK_CASES, ids=TOPK_IDS)
def test_topk_semantics(cases, case, trainable, k, with_excl, subset):
    """test_gpu_recommend.check_topk's properties: distinct ids from the allowed candidates, scores equal to the call's own
    all_scores bit for bit and non-increasing, and against the oracle within the score bar.  The exclusion lists are unsorted,
    hold duplicates and ids outside the candidates."""
    eng = cases(case, trainable)[1]
    uids, doms = queries()
    ref = reference(cases, case, trainable)
    cand = candidate_list(subset)
    excl = exclusion_lists(ref, cand) if with_excl else None
    ids, scores, all_scores = eng.recommend(uids, doms, k, candidates=cand if subset else None, exclude=excl, want_scores=True)
    assert ids.shape == scores.shape == (7, k) and all_scores.shape == (7, cand.size)
    check_topk(ids, scores, all_scores, ref, cand, excl, k)


@pytest.mark.parametrize("case,trainable", TOPK_CASES, ids=TOPK_IDS)
def test_short_lists_end_in_padding(cases, case, trainable):
    eng = cases(case, trainable)[1]
    uids, doms = queries()
    ref = reference(cases, case, trainable)
    cand = np.array([340, 7, 120, 64, 345], np.int32)           # 5 candidates, k 10
    ids, scores, all_scores = eng.recommend(uids, doms, 10, candidates=cand, want_scores=True)
    check_topk(ids, scores, all_scores, ref, cand, None, 10)
    assert np.all(ids[:, 5:] == -1) and np.all(scores[:, 5:] == 0) and np.all(ids[:, :5] >= 0)
    cand = np.arange(N_ITEM, dtype=np.int32)
    excl = [[] for _ in range(7)]
    excl[4] = np.setdiff1d(cand, [33, 290])                      # keeps two items
    excl[1] = cand                                               # excludes everything
    ids, scores, all_scores = eng.recommend(uids, doms, 10, exclude=excl, want_scores=True)
    check_topk(ids, scores, all_scores, ref, cand, excl, 10)
    assert sorted(ids[4, :2].tolist()) == [33, 290] and np.all(ids[4, 2:] == -1) and np.all(scores[4, 2:] == 0)
    assert np.all(ids[1] == -1) and np.all(scores[1] == 0) and np.all(all_scores[1] == 0)
    assert np.all(ids[0] >= 0)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", ["nfm", "autoint"])
def test_exact_ties_rank_by_id_wherever_the_pair_sits(case):
    """every item row identical and the linear item table zero (frozen tables): a query's 346 logits are ONE value in every
    tile and in the padded last batch, and the top 10 are the ten smallest non-excluded ids although the candidates are
    shuffled."""
    def same_rows(p):
        p["item_emb"] = np.repeat(p["item_emb"][17:18], N_ITEM, axis=0)
        p["lin_item"][...] = 0
    _, eng, model = make_case(case, False, same_rows)
    uids, doms = queries()
    cand = np.random.RandomState(9).permutation(N_ITEM).astype(np.int32)
    excl = [[0, 3, 4, 300]] * 3 + [[]] * 4
    ids, scores, all_scores = eng.recommend(uids, doms, 10, candidates=cand, exclude=excl, want_scores=True)
    eng.close()
    for q in range(7):
        allowed = ~np.isin(cand, excl[q])
        b = np.unique(bits(all_scores[q, allowed]))
        assert b.size == 1, (q, b)
        assert np.all(all_scores[q, ~allowed] == 0)
        want = np.setdiff1d(np.arange(N_ITEM), excl[q])[:10]
        assert ids[q].tolist() == want.tolist(), (q, ids[q])
        assert np.all(bits(scores[q]) == b[0])
    np.testing.assert_allclose(all_scores[3], oracle_scores(model, uids, doms, cand)[3], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------------------- 4
def rank_targets(ref_d, cand, excl):
    """per query: the oracle's best and worst candidate, an excluded id, an id outside the candidates; query 5 has none."""
    outside = np.setdiff1d(np.arange(N_ITEM), cand)
    out = []
    for q in range(7):
        o = ref_d[q, cand]
        t = [cand[np.argmax(o)], cand[np.argmin(o)], cand[(7 * q + 3) % cand.size], cand[(11 * q + 50) % cand.size]]
        if excl is not None and len(excl[q]):
            t.append(int(np.asarray(excl[q])[0]))
        if outside.size:
            t.append(int(outside[q]))
        out.append([] if q == 5 else t)
    return out


SLATE_LENS = [0, 1, 63, 64, 65, 256, 257, N_ITEM]


def slate_lists(seed=21):
    rs = np.random.RandomState(seed)
    return [rs.permutation(N_ITEM)[:n].astype(np.int32) for n in SLATE_LENS]


def all_calls(eng, ref_d):
    """the four calls on one engine -> {name: array}: what the chunking and the two-runs tests compare byte for byte."""
    uids, doms = queries()
    out = {}
    for k, subset in ((10, False), (128, True)):
        cand = candidate_list(subset)
        excl = exclusion_lists(ref_d, cand)
        ids, scores, all_scores = eng.recommend(uids, doms, k, candidates=cand if subset else None, exclude=excl, want_scores=True)
        out.update({"ids_%d" % k: ids, "scores_%d" % k: scores, "all_%d" % k: all_scores})
        r = eng.rank_domain(uids, DOMAIN, rank_targets(ref_d, cand, excl), candidates=cand if subset else None, exclude=excl,
                            want_scores=True)
        out.update({"ranks_%d" % k: r["ranks"], "live_%d" % k: r["live"], "tscores_%d" % k: r["scores"]})
    s = eng.rank_slates(np.resize(uids, len(SLATE_LENS)), DOMAIN, slate_lists(), want_order=True)
    out.update(slate_pos=s["pos"], slate_scores=s["scores"], slate_order=s["order"])
    return out


def chunk_case(case, trainable, path):
    """the calls of the chunking test, dumped to `path` (run in the test's child processes)."""
    _, eng, model = make_case(case, trainable)
    uids, _ = queries()
    out = all_calls(eng, oracle_scores(model, uids, np.full(7, DOMAIN), np.arange(N_ITEM)))
    eng.close()
    np.savez(path, **out)


@pytest.mark.parametrize("case,trainable", [("pnn", False), ("mlp64", True)], ids=["pnn-frozen", "mlp64-trainable"])
def test_chunking_does_not_change_a_bit(tmp_path, case, trainable):
    """MAMDR_REC_CHUNK=64 and =128 in fresh child processes (six and three chunks for 346 candidates): ids, scores, the dense
    score matrix, ranks, live counts, slate positions and slate scores are the default run's bytes."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    paths = {}
    for chunk in (None, "64", "128"):
        paths[chunk] = str(tmp_path / ("chunk_%s.npz" % chunk))
        code = "import test_gpu_graph_retrieval as t; t.chunk_case(%r, %r, %r)" % (case, trainable, paths[chunk])
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
        env.pop("MAMDR_REC_CHUNK", None)
        if chunk:
            env["MAMDR_REC_CHUNK"] = chunk
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
    with np.load(paths[None]) as a:
        assert len(a.files) == 15
        for chunk in ("64", "128"):
            with np.load(paths[chunk]) as b:
                assert sorted(a.files) == sorted(b.files)
                for name in a.files:
                    assert a[name].tobytes() == b[name].tobytes(), (chunk, name)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("case,trainable", [("autoint", False), ("nfm", True), ("wdl256", False)],
                         ids=["autoint-frozen", "nfm-trainable", "wdl256-frozen"])
def test_one_score_everywhere(cases, case, trainable):
    """recommend_domain = recommend with a constant domain vector, byte for byte; rank_domain's and rank_slates's scores of a
    pair are the bits of scores_all."""
    eng = cases(case, trainable)[1]
    uids, _ = queries()
    cand = candidate_list(True)
    ref_d = reference(cases, case, trainable, np.full(7, DOMAIN))
    excl = exclusion_lists(ref_d, cand)
    a = eng.recommend(uids, np.full(7, DOMAIN), 128, candidates=cand, exclude=excl, want_scores=True)
    b = eng.recommend_domain(uids, DOMAIN, 128, candidates=cand, exclude=excl, want_scores=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    full = eng.recommend_domain(uids, DOMAIN, 10, want_scores=True)[2]          # nothing excluded: every pair's score
    r = eng.rank_domain(uids, DOMAIN, rank_targets(ref_d, cand, excl), candidates=cand, exclude=excl, want_scores=True)
    for q in range(7):
        sl = slice(r["offsets"][q], r["offsets"][q + 1])
        assert np.array_equal(bits(r["scores"][sl]), bits(full[q, r["ids"][sl]])), q
    slates = slate_lists()
    s = eng.rank_slates(np.resize(uids, len(slates)), DOMAIN, slates)
    for q in range(len(slates)):
        sl = slice(s["offsets"][q], s["offsets"][q + 1])
        assert np.array_equal(bits(s["scores"][sl]), bits(full[q % 7, s["ids"][sl]])), q
    np.testing.assert_allclose(full, ref_d, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("case,trainable", [("ccpm", False), ("pnn", True), ("deepfm32", False), ("autoint", True)],
                         ids=["ccpm-frozen", "pnn-trainable", "deepfm32-frozen", "autoint-trainable"])
def test_retrieval_score_is_the_evaluation_score(case, trainable):
    """a split of exactly 512 triples (two full batches of max_batch rows) bound as a domain's test split:
    evaluate(want_preds=True) gives the same triples' retrieval scores bit for bit -- through the list form (one slate of
    one item per triple) and through the grid form (scores_all)."""
    g, eng, model = make_case(case, trainable)
    rs = np.random.RandomState(4)
    uid = rs.randint(0, g["n_user"], 512).astype(np.int32)
    pid = rs.randint(0, N_ITEM, 512).astype(np.int32)
    eng.bind_domain_data(DOMAIN, "test", uid, pid, np.full(512, DOMAIN, np.int32), (rs.rand(512) < 0.3).astype(np.float32))
    preds = eng.evaluate(DOMAIN, "test", want_preds=True)[3]
    assert preds.shape == (512,)
    s = eng.rank_slates(uid, DOMAIN, [[p] for p in pid])
    assert np.array_equal(bits(s["scores"]), bits(preds))
    full = eng.recommend_domain(uid[:7], DOMAIN, 10, want_scores=True)[2]
    assert np.array_equal(bits(full[np.arange(7), pid[:7]]), bits(preds[:7]))
    np.testing.assert_allclose(preds, model.predict(uid, pid, np.full(512, DOMAIN, np.int32)), rtol=RTOL, atol=ATOL)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("subset", [False, True], ids=["all346", "subset201"])
@pytest.mark.parametrize("case,trainable", [("ccpm", True), ("mlp64", False)], ids=["ccpm-trainable", "mlp64-frozen"])
def test_ranks(cases, case, trainable, subset):
    eng = cases(case, trainable)[1]
    uids, _ = queries()
    cand = candidate_list(subset)
    ref_d = reference(cases, case, trainable, np.full(7, DOMAIN))
    excl = exclusion_lists(ref_d, cand)
    targets = rank_targets(ref_d, cand, excl)
    kw = dict(candidates=cand if subset else None, exclude=excl)
    r = eng.rank_domain(uids, DOMAIN, targets, want_scores=True, **kw)
    again = eng.rank_domain(uids, DOMAIN, targets, want_scores=True, **kw)
    for name in ("ranks", "live", "scores"):
        assert r[name].tobytes() == again[name].tobytes(), name
    top = eng.recommend_domain(uids, DOMAIN, 128, **kw)[0]
    assert r["offsets"][6] == r["offsets"][5]                    # the query without targets
    n_listed = 0
    for q in range(7):
        ex = np.unique(np.asarray(excl[q], np.int64))
        allowed = ~np.isin(cand, ex)
        assert r["live"][q] == int(allowed.sum()), q
        o = ref_d[q, cand][allowed]
        for j in range(r["offsets"][q], r["offsets"][q + 1]):
            t, rank = int(r["ids"][j]), int(r["ranks"][j])
            s = float(ref_d[q, t])
            lo, hi = int((o > s + tol(s)).sum()), int((o >= s - tol(s)).sum())
            assert lo <= rank <= hi, (q, t, rank, lo, hi)
            assert abs(float(r["scores"][j]) - s) <= tol(s)
            if r["listed"][j]:
                n_listed += 1
                if rank < 128:
                    assert top[q, rank] == t, (q, t, rank)
                else:
                    assert t not in top[q]
            else:
                assert t not in top[q]
        best = cand[allowed][np.argmax(o)]
        assert top[q, 0] == best or abs(float(ref_d[q, top[q, 0]]) - float(o.max())) <= 2 * tol(o.max())
    assert n_listed >= 12 and not r["listed"].all()
    none = eng.rank_domain(uids, DOMAIN, [[] for _ in range(7)], **kw)     # a call with no targets at all
    assert none["ranks"].size == 0 and np.array_equal(none["live"], r["live"])


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case,trainable", [("pnn", False), ("deepfm32", True)], ids=["pnn-frozen", "deepfm32-trainable"])
def test_slates(cases, case, trainable):
    eng = cases(case, trainable)[1]
    uids, _ = queries()
    slates = slate_lists()
    quids = np.resize(uids, len(slates))
    s = eng.rank_slates(quids, DOMAIN, slates, want_order=True)
    ref_d = reference(cases, case, trainable, np.full(7, DOMAIN))
    assert np.diff(s["offsets"]).tolist() == SLATE_LENS
    per_item, n_ties, n_inverted = [], 0, 0
    for q, L in enumerate(SLATE_LENS):
        sl = slice(s["offsets"][q], s["offsets"][q + 1])
        ids, sc, pos, order = s["ids"][sl], s["scores"][sl], s["pos"][sl], s["order"][sl]
        assert sorted(pos.tolist()) == list(range(L)), q
        assert np.array_equal(order[pos], np.arange(L)), q
        by_pos = np.argsort(pos)
        assert np.all(np.diff(sc[by_pos]) <= 0), q                # consistent with the call's own scores
        np.testing.assert_allclose(sc, ref_d[q % 7, ids], rtol=RTOL, atol=ATOL)
        per_item.append(dict(zip(ids.tolist(), zip(bits(sc).tolist(), pos.tolist()))))
        # the keys order by LOGIT, then id: two different logits can round to one score, so equal scores of random rows do not
        # bind the ids' order (counted and printed here); where the logits themselves are equal the order is by id:
        # test_slates_with_equal_scores_order_by_id, at every one of these lengths
        tie = np.diff(bits(sc[by_pos])) == 0
        n_ties += int(tie.sum())
        n_inverted += int((tie & (np.diff(ids[by_pos]) < 0)).sum())
    print("%s: %d adjacent equal scores, %d of them with descending ids" % (case, n_ties, n_inverted))
    shuffled = [np.random.RandomState(q).permutation(x) for q, x in enumerate(slates)]
    t = eng.rank_slates(quids, DOMAIN, shuffled)
    for q in range(len(SLATE_LENS)):
        sl = slice(t["offsets"][q], t["offsets"][q + 1])
        got = dict(zip(t["ids"][sl].tolist(), zip(bits(t["scores"][sl]).tolist(), t["pos"][sl].tolist())))
        assert got == per_item[q], q                              # no score bit and no position of an item moved


def test_slates_with_equal_scores_order_by_id():
    """every item row identical: one logit per query, so where scores are equal the positions are ordered by id -- at every
    slate length of test_slates, the entries shuffled."""
    def same_rows(p):
        p["item_emb"] = np.repeat(p["item_emb"][17:18], N_ITEM, axis=0)
        p["lin_item"][...] = 0
    _, eng, _ = make_case("nfm", False, same_rows)
    uids, _ = queries()
    slates = slate_lists(5)
    s = eng.rank_slates(np.resize(uids, len(slates)), DOMAIN, slates)
    eng.close()
    for q, ids in enumerate(slates):
        sl = slice(s["offsets"][q], s["offsets"][q + 1])
        assert np.unique(bits(s["scores"][sl])).size <= 1
        assert np.array_equal(s["ids"][sl], ids) and np.array_equal(s["pos"][sl], np.argsort(np.argsort(ids))), q


def test_a_second_query_block_changes_no_byte(cases):
    """257 queries are a block of 256 and a block of one (REC_QBLOCK): the module's 7 queries, 249 repeats of query 0 without
    targets or slates, and query 3 again as query 256.  Over 70 candidates (one full tile and 6: 257 x 128 padded pairs per
    call) all four calls give queries 0-6 the 7-query call's bytes and query 256 those of query 3; a slates call whose
    second block is empty writes nothing behind its entries."""
    eng = cases("mlp64", False)[1]
    uids, doms = queries()
    rs = np.random.RandomState(31)
    cand = rs.permutation(N_ITEM)[:70].astype(np.int32)
    ref_d = reference(cases, "mlp64", False, np.full(7, DOMAIN))
    excl = exclusion_lists(ref_d, cand)
    targets = rank_targets(ref_d, cand, excl)
    slates = [rs.permutation(N_ITEM)[:n].astype(np.int32) for n in (0, 1, 63, 64, 65, 70, 2)]
    last_slate = rs.permutation(N_ITEM)[:65].astype(np.int32)
    big_u = np.concatenate([uids, np.full(249, uids[0], np.int32), uids[3:4]])
    big_d = np.concatenate([doms, np.full(249, doms[0]), doms[3:4]]).astype(np.int32)
    big_excl = list(excl) + [[]] * 249 + [excl[3]]
    big_targets = list(targets) + [[]] * 249 + [targets[3]]
    big_slates = slates + [last_slate[:0]] * 249 + [last_slate]
    assert big_u.size == 257
    rows = np.r_[0:7, 256]
    same = lambda a, b, what: (a.tobytes() == b.tobytes()) or pytest.fail(what)       # noqa: E731

    small = eng.recommend(uids, doms, 10, candidates=cand, exclude=excl, want_scores=True)
    big = eng.recommend(big_u, big_d, 10, candidates=cand, exclude=big_excl, want_scores=True)
    for name, s, b in zip(("ids", "scores", "all_scores"), small, big):
        assert b.shape[0] == 257
        same(b[rows], s[np.r_[0:7, 3]], "recommend: " + name)
    small = eng.recommend_domain(uids, DOMAIN, 128, candidates=cand, exclude=excl, want_scores=True)
    big = eng.recommend_domain(big_u, DOMAIN, 128, candidates=cand, exclude=big_excl, want_scores=True)
    for name, s, b in zip(("ids", "scores", "all_scores"), small, big):
        same(b[rows], s[np.r_[0:7, 3]], "recommend_domain: " + name)
    assert np.all(big[0][:, 70:] == -1) and np.all(big[0][0, :20] >= 0)

    small = eng.rank_domain(uids, DOMAIN, targets, candidates=cand, exclude=excl, want_scores=True)
    big = eng.rank_domain(big_u, DOMAIN, big_targets, candidates=cand, exclude=big_excl, want_scores=True)
    n7, q3 = small["offsets"][7], slice(small["offsets"][3], small["offsets"][4])
    assert big["offsets"][256] == n7 and big["offsets"][257] - n7 == q3.stop - q3.start > 0
    for name in ("ids", "ranks", "scores"):
        same(big[name][:n7], small[name], "rank_domain: " + name)
        same(big[name][n7:], small[name][q3], "rank_domain, query 256: " + name)
    same(big["live"][rows], small["live"][np.r_[0:7, 3]], "rank_domain: live")
    assert np.all(big["live"][7:256] == 70)         # queries without targets are counted all the same: nothing excluded

    small = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    small3 = eng.rank_slates(uids, DOMAIN, slates[:3] + [last_slate] + slates[4:], want_order=True)   # query 3 with query 256's slate
    big = eng.rank_slates(big_u, DOMAIN, big_slates, want_order=True)
    n7 = small["offsets"][7]
    q3 = slice(small3["offsets"][3], small3["offsets"][4])
    assert big["offsets"][256] == n7 == 265 and big["offsets"][257] == n7 + 65
    for name in ("pos", "order", "scores"):
        same(big[name][:n7], small[name], "rank_slates: " + name)
        same(big[name][n7:], small3[name][q3], "rank_slates, query 256: " + name)

    # the same 7 slates with an EMPTY second block, through the C ABI into outputs 64 entries too long
    dev = torch.device("cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = np.concatenate([small["offsets"], np.full(250, n7)]).astype(np.int64)
    assert off.size == 258
    d_uid, d_off, d_ids = (torch.from_numpy(a).to(dev) for a in (big_u, off, small["ids"]))
    outs = [torch.full((n7 + 64,), -7, dtype=torch.int32, device=dev), torch.full((n7 + 64,), -7, dtype=torch.int32, device=dev),
            torch.full((n7 + 64,), -7.0, dtype=torch.float32, device=dev)]
    assert eng.lib.mamdr_graph_rank_slates(eng.ctx, DOMAIN, 257, p(d_uid), p(d_off), p(d_ids), p(outs[2]), p(outs[0]), p(outs[1])) == 0
    for name, t in zip(("pos", "order", "scores"), outs):
        got = t.cpu().numpy()
        same(got[:n7], small[name], "rank_slates, empty second block: " + name)
        assert np.all(got[n7:] == -7), name


# ---------------------------------------------------------------------------------------------------------------- 8
def state_digest(eng):
    return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (eng.weights, eng.adam_m, eng.adam_v)] + list(eng.counters())


@pytest.mark.parametrize("case,trainable", [("autoint", True), ("ccpm", False)], ids=["autoint-trainable", "ccpm-frozen"])
def test_retrieval_reads_the_state_only(case, trainable):
    g, a, _ = make_case(case, trainable)
    _, b, _ = make_case(case, trainable)
    d = max(range(10), key=lambda i: g["data"]["train"][i]["uid"].shape[0])
    uids, doms = queries()
    for e in (a, b):
        e.train_steps(d, n_steps=2)
    before = state_digest(a)
    assert before[3:] == [2, 2]
    calls = (lambda: a.recommend(uids, doms, 10, want_scores=True),
             lambda: a.recommend_domain(uids, DOMAIN, 128, exclude=[[1, 2]] * 7),
             lambda: a.rank_domain(uids, DOMAIN, [[5, 6]] * 7, candidates=candidate_list(True)),
             lambda: a.rank_slates(uids, DOMAIN, [[5, 6, 9]] * 7, want_order=True))
    for call in calls:
        call()
        assert state_digest(a) == before
    # a training step and an evaluation behind the calls: the bytes of the twin that made no retrieval call
    for e in (a, b):
        e.train_steps(d, first_step=2, n_steps=1)
    assert state_digest(a) == state_digest(b)
    ea, eb = a.evaluate(d, "val", want_preds=True), b.evaluate(d, "val", want_preds=True)
    assert ea[0] == eb[0] and ea[1] == eb[1] and ea[3].tobytes() == eb[3].tobytes()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_refusals_through_the_c_abi(cases):
    """argument checks only: none of these calls launches anything."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import _lib, graph_engine
    lib = _lib.load()
    dev = torch.device("cuda")
    q = torch.zeros(2, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 1, 2], dtype=torch.int64, device=dev)
    bad_off = torch.tensor([0, 2, 1], dtype=torch.int64, device=dev)
    ids = torch.zeros(4, dtype=torch.int32, device=dev)
    out_i = torch.zeros(256, dtype=torch.int32, device=dev)
    out_f = torch.zeros(256, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def four(ctx, n_query=2, uid=q, domain=0, k=10, o=off):
        u = p(uid) if uid is not None else None
        return (lib.mamdr_graph_recommend(ctx, n_query, u, p(q), None, 0, None, None, k, p(out_i), p(out_f), None),
                lib.mamdr_graph_recommend_domain(ctx, domain, n_query, u, None, 0, None, None, k, p(out_i), p(out_f), None),
                lib.mamdr_graph_rank_domain(ctx, domain, n_query, u, None, 0, None, None, p(o), p(ids), p(out_i), None, p(out_i)),
                lib.mamdr_graph_rank_slates(ctx, domain, n_query, u, p(o), p(ids), None, p(out_i), None))

    refused = {"mmoe": graph_engine.GraphEngine("mmoe", 1188, N_ITEM, 10, 256, (128, 64), (64,), (64,), num_experts=2),
               "star": graph_engine.GraphEngine("star", 1188, N_ITEM, 10, 256, (256, 128, 64), (), norm="bn", dense="dense")}
    for kind, eng in refused.items():
        for fn in (0, 1, 2, 3):
            assert four(eng.ctx)[fn] == _lib.ENOTBUILT
            assert kind in lib.mamdr_graph_last_error().decode(), (kind, fn)
        eng.close()
    ctx = cases("ccpm", False)[1].ctx
    assert four(ctx, k=0)[:2] == (_lib.EINVAL, _lib.EINVAL) and "k 0" in lib.mamdr_graph_last_error().decode()
    assert four(ctx, k=129)[:2] == (_lib.EINVAL, _lib.EINVAL)
    assert four(ctx, n_query=0) == (_lib.EINVAL,) * 4
    assert four(ctx, uid=None) == (_lib.EINVAL,) * 4
    assert four(ctx, domain=10)[1:] == (_lib.EINVAL,) * 3 and four(ctx, domain=-1)[1:] == (_lib.EINVAL,) * 3
    assert four(ctx, o=bad_off)[2:] == (_lib.EINVAL,) * 2 and "descend" in lib.mamdr_graph_last_error().decode()
    raw = graph_engine.GraphEngine("mlp", 1188, N_ITEM, 10, 256, (128, 64), (), emb_dim=64)      # frozen tables, none bound
    assert four(raw.ctx) == (_lib.ESTATE,) * 4
    with pytest.raises(NotImplementedError, match="generic-layer towers.*mlp.*not built for retrieval.*enable_retrieval"):
        raw.recommend([0], [0], 5)      # as an engine object of this kind always answered, until it is asked to serve
    raw.enable_retrieval()
    with pytest.raises(_lib.MamdrError) as e:
        raw.recommend([0], [0], 5)
    assert e.value.code == _lib.ESTATE
    launched = []
    real = raw.lib.mamdr_graph_recommend
    try:                                # the host's range checks run before any launch on this engine too
        raw.lib.mamdr_graph_recommend = lambda *a: launched.append(a) or 0
        for bad in (dict(uids=[1188], domains=[0]), dict(uids=[0], domains=[10])):
            with pytest.raises(ValueError):
                raw.recommend(k=5, **bad)
        with pytest.raises(ValueError):
            raw.recommend([0], [0], 5, candidates=[3, 3])
    finally:
        raw.lib.mamdr_graph_recommend = real
    assert not launched
    raw.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def hit_rate_at_k(ids, ds, d, users):
    """HitRate@K by hand: the share of users with a label-1 item of the test split that have one of them in their list."""
    c = ds.test_dataset[d]["data"]
    uid, pid, lab = np.asarray(c["uid"]), np.asarray(c["pid"]), np.asarray(c["label"])
    hits = n = 0
    for row, u in zip(ids, users):
        pos = set(pid[(uid == u) & (lab > 0)].tolist())
        if pos:
            n += 1
            hits += bool(pos & set(row[row >= 0].tolist()))
    return hits / float(max(n, 1))


def test_run_config_at_width_64_with_every_ranking_report(tmp_path):
    """run.py's entry on the shipped 64-wide config at the smallest synthetic scale, one epoch, with --recommend 10,
    train.rank_eval, train.sampled_eval and train.list_metrics: the four .npz files with their documented arrays, the
    list-metric keys in result.json, and one domain's HitRate@10 recomputed from the written ids."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, graph_engine, list_metrics as lm
    with open(os.path.join(ROOT, "config", "Taobao-10", "emb64", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=1, patience=1, sample_num=2, meta_learning_rate=0.5, rank_eval=[10, 50], sampled_eval=20,
                        sampled_eval_ks=[1, 5], list_metrics=10,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.05)
    built = []
    res = cli.main(cfg, on_model=built.append, recommend=10)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    assert isinstance(model.model, graph_engine.GraphEngine) and model.model.kind == "mlp" and model.model.emb_dim == 64
    ds, rp = model.dataset, model.result_path
    with np.load(os.path.join(rp, "recommend_top10.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and z["hit_rate"].shape == z["recall"].shape == z["ndcg"].shape == (10,)
        for d in range(10):
            users, ids = z["users_%d" % d], z["ids_%d" % d]
            assert np.array_equal(users, np.unique(ds.test_dataset[d]["data"]["uid"]))
            assert ids.shape == z["scores_%d" % d].shape == (users.size, 10) and ids.dtype == np.int32
        d = int(np.argmax(z["hit_rate"]))
        assert abs(hit_rate_at_k(z["ids_%d" % d], ds, d, z["users_%d" % d]) - z["hit_rate"][d]) <= 1e-12
        rec_ids = {d: z["ids_%d" % d] for d in range(10)}
    with np.load(os.path.join(rp, "rank_eval.npz")) as z:
        assert z["ks"].tolist() == [10, 50] and z["mrr"].shape == (10,) and z["hit_rate"].shape == (10, 2)
        for d in range(10):
            off, ids, ranks, listed, live = (z["%s_%d" % (n, d)] for n in ("offsets", "ids", "ranks", "listed", "live"))
            assert off[-1] == ids.size == ranks.size == listed.size and live.shape == (z["users_%d" % d].size,)
            # (the lists above are the live weights', these ranks each domain's own merged weights': two different rankings
            # under this wrapper; test_ccpm_model_recommends_and_ranks holds the two routes together on a plain model)
            assert listed.any() and np.all(ranks[listed] < np.repeat(live, np.diff(off))[listed])
            assert rec_ids[d].shape[0] == live.size
    with np.load(os.path.join(rp, "sampled_eval_neg20.npz")) as z:
        want = {"domains", "ks", "n_neg", "seed", "mrr", "mean_percentile", "hit_rate", "recall", "ndcg", "n_short"}
        want |= {"%s_%d" % (n, d) for d in range(10) for n in ("users", "positives", "offsets", "ids", "scores", "pos", "rank")}
        assert set(z.files) == want and int(z["n_neg"]) == 20 and z["ks"].tolist() == [1, 5]
    with np.load(os.path.join(rp, "list_metrics_top10.npz")) as z:
        assert z["domains"].tolist() == list(range(10)) and int(z["k"]) == 10
    rdir = [os.path.join(rp, f) for f in os.listdir(rp) if f.startswith("loss_")][0]
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    for key in lm.FIGURES:
        assert sorted(result["domain_" + key]) == sorted(str(d) for d in range(10)), key
    for key in lm.AVERAGED:
        assert np.isfinite(result["avg_" + key])


def test_ccpm_model_recommends_and_ranks(tmp_path):
    """a CCPM config through BaseModel.recommend and rank_eval directly: HitRate@10 by hand equals recommend.ranking_metrics,
    and a listed target of rank r < 10 is the r-th id of the list."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, graph_engine, recommend
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_taobao_10.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="ccpm")
    cfg["train"].update(epoch=1, patience=1, result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.05)
    built = []
    cli.main(cfg, on_model=built.append)
    model = built[0]
    assert isinstance(model.model, graph_engine.GraphEngine) and model.model.kind == "ccpm"
    d = 2
    r = model.recommend(d, 10)
    m = recommend.ranking_metrics(r["ids"], recommend.split_positives(model.dataset, d, r["users"]))
    assert abs(hit_rate_at_k(r["ids"], model.dataset, d, r["users"]) - m["hit_rate"]) <= 1e-12
    e = model.rank_eval(d)
    assert np.array_equal(e["users"], r["users"])
    n = 0
    for q in range(e["live"].size):
        for j in range(e["offsets"][q], e["offsets"][q + 1]):
            if e["listed"][j] and e["ranks"][j] < 10:
                n += 1
                assert r["ids"][q, e["ranks"][j]] == e["ids"][j], (q, j)
            else:
                assert e["ids"][j] not in r["ids"][q], (q, j)
    print("ccpm domain %d: HitRate@10 %.4f, %d targets inside the top 10" % (d, m["hit_rate"], n))
    lst = model.list_eval(d, 10)
    assert lst is not None
