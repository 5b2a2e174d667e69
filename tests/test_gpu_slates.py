"""Per-query candidate slates on the device (mamdr_rank_slates, TowerEngine.rank_slates, run.py --sampled-eval) against the
calls that share one candidate list per call: a pair's score must be the bits mamdr_rank_domain gives it, an entry's
position its index in mamdr_recommend_domain's complete order of the slate or its mamdr_rank_domain rank among the slate.
A pair's logit is the same bits wherever it sits, so every comparison with those calls is exact; only the comparison with
oracle/tower.py's scores carries the project's prediction bar.

Problem: tests/test_gpu_recommend.py's -- 1,188 users, 346 items, 10 domains, the seven users of queries(), every query in
domain 3; the cases are mlp with frozen tables and deepfm with trainable ones, and the Star engine of
tests/test_gpu_recommend_star.py.  Slate lengths 0, 1, 2, 63, 64, 65, 130 and 346 cover the wave regime of k_slate_order
(up to 64 entries), its boundary, a remainder of the 256-entry tile, and a slate of two tiles -- all inside ONE LDS stage of
1,024 keys, the fixture's catalogue being 346 items.  The stage loop's later rounds (the barrier that guards the reuse of the
staged keys, the offset of a stage, a partial last stage) run in test_slates_longer_than_an_lds_stage, on an engine of 2,300
items."""
import copy
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_recommend as base            # noqa: E402  (the problem, the engines)
import test_gpu_rank as rbase                # noqa: E402  (users7, reference, parts)
import test_gpu_recommend_star as sbase      # noqa: E402  (the Star engine)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = base.RTOL, base.ATOL            # the project's prediction bar: rtol 2e-5 / atol 2e-7
DOMAIN = 3
CASES = rbase.CASES
CASE_IDS = rbase.CASE_IDS
RAGGED = [0, 1, 2, 63, 64, 65, 130, 346]
E2E_NEG = 50          # run.py --sampled-eval N of the end-to-end test: every test user of that data has >= 187 free items

_REF = {}
engines = base.engines          # the module-scoped fixture of test_gpu_recommend.py: one engine per (tower, trainable)
users7 = rbase.users7


def users8():
    """the seven users and the first of them again: one query per length of RAGGED."""
    u = users7()
    return np.concatenate([u, u[:1]])


def ragged_slates(seed=31):
    rs = np.random.RandomState(seed)
    return [rs.choice(346, n, replace=False).astype(np.int32) for n in RAGGED]


def rows(res):
    off = res["offsets"]
    return [(q, slice(off[q], off[q + 1])) for q in range(off.size - 1)]


def by_id(res, name):
    """per query {item id: res[name] of its entry}."""
    return [dict(zip(res["ids"][sl].tolist(), res[name][sl].tolist())) for _, sl in rows(res)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check_permutations(res):
    for q, sl in rows(res):
        assert sorted(res["pos"][sl].tolist()) == list(range(sl.stop - sl.start)), q
        if "order" in res:
            assert np.array_equal(res["order"][sl][res["pos"][sl]], np.arange(sl.stop - sl.start)), q
    if "order" in res:
        assert res["order"].dtype == np.int32 and (res["order"] >= 0).all()
    assert res["pos"].dtype == np.int32 and res["scores"].dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_scores_are_rank_domains_bit_for_bit(engines, tower, trainable):
    eng = engines(tower, trainable)
    uids, slates = users8(), ragged_slates()
    res = eng.rank_slates(uids, DOMAIN, slates)
    assert np.diff(res["offsets"]).tolist() == RAGGED and np.array_equal(res["ids"], np.concatenate(slates))
    rd = eng.rank_domain(uids, DOMAIN, slates, want_scores=True)
    want = by_id(rd, "scores")
    ref = rbase.reference(tower, trainable)
    n = 0
    for q, sl in rows(res):
        w = np.asarray([want[q][i] for i in res["ids"][sl].tolist()], np.float32)
        assert np.array_equal(bits(res["scores"][sl]), bits(w)), q
        np.testing.assert_allclose(res["scores"][sl], ref[q % 7, res["ids"][sl]], rtol=RTOL, atol=ATOL)
        n += w.size
    assert n == sum(RAGGED)
    # ... and the dense matrix entries of recommend_domain
    dense = eng.recommend_domain(uids, DOMAIN, 1, want_scores=True)[2]
    for q, sl in rows(res):
        assert np.array_equal(bits(res["scores"][sl]), bits(dense[q, res["ids"][sl]])), q


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_pos_is_the_index_in_the_complete_order(engines, tower, trainable):
    eng = engines(tower, trainable)
    uids = users7()
    rs = np.random.RandomState(41)
    for cand in rbase.parts():
        assert cand.size in (128, 90)
        slates = [rs.permutation(cand) for _ in range(7)]
        res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
        ids = eng.recommend_domain(uids, DOMAIN, 128, candidates=cand)[0]
        for q, sl in rows(res):
            assert np.array_equal(ids[q, res["pos"][sl]], res["ids"][sl]), q            # pos[j] = index of the item
            assert np.array_equal(res["ids"][sl][res["order"][sl]], ids[q, :cand.size]), q  # order = the inverse permutation
        check_permutations(res)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_ragged_slates_hold_rank_domains_ranks(engines, tower, trainable):
    eng = engines(tower, trainable)
    uids, slates = users8(), ragged_slates()
    res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    check_permutations(res)
    for q, sl in rows(res):
        if not slates[q].size:
            assert sl.start == sl.stop
            continue
        rd = eng.rank_domain(uids[q:q + 1], DOMAIN, [slates[q]], candidates=slates[q])
        assert rd["listed"].all() and rd["live"][0] == slates[q].size
        want = dict(zip(rd["ids"].tolist(), rd["ranks"].tolist()))
        assert res["pos"][sl].tolist() == [want[i] for i in res["ids"][sl].tolist()], q


# ---------------------------------------------------------------------------------------------------------------- 3b
BIG_ITEMS = 2300
LONG = [1024, 1025, 2138, 65, 2300, 100]      # one full stage; + 1; 2 stages + 90; (wave boundary + 1); 2 stages + 252; N = 99


def make_big_engine(tied=False):
    """an mlp engine with frozen random tables of 64 users x 2,300 items (no oracle: every comparison below is with the
    library's own calls); tied: every item row identical."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd.engine import TowerEngine
    rs = np.random.RandomState(61)
    eng = TowerEngine(64, BIG_ITEMS, 10, 256, dropout=0.0, emb_trainable=False, tower="mlp")
    eng.bind_table("user_emb", (rs.standard_normal((64, 128)) * 0.1).astype(np.float32))
    items = (rs.standard_normal((BIG_ITEMS, 128)) * 0.1).astype(np.float32)
    eng.bind_table("item_emb", np.repeat(items[17:18], BIG_ITEMS, axis=0) if tied else items)
    scale = {"domain_emb": 0.05, "W0": 0.06, "W1": 0.07, "W2": 0.1, "wo": 0.17, "gb": 0.0}
    eng.set_weights(eng.pack({n: (rs.standard_normal(cnt) * scale.get(n, 0.05)).astype(np.float32)
                              for n, (off, cnt) in eng.segments.items()}))
    return eng


def test_slates_longer_than_an_lds_stage():
    """slates of 1,024, 1,025, 2,138 (= 2 x 1,024 + 90) and 2,300 entries: two and three rounds of k_slate_order's stage loop
    with a partial last stage, several 256-entry tiles per slate with a remainder.  pos is rank_domain's rank of every entry
    among its own slate, exactly; order is its inverse; the first 128 positions are recommend_domain's list; a second call
    with the entries permuted gives every item the same position."""
    eng = make_big_engine()
    rs = np.random.RandomState(67)
    uids = rs.choice(64, len(LONG), replace=False).astype(np.int32)
    slates = [rs.choice(BIG_ITEMS, n, replace=False).astype(np.int32) for n in LONG]
    res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    assert np.diff(res["offsets"]).tolist() == LONG
    check_permutations(res)
    shuffled = eng.rank_slates(uids, DOMAIN, [rs.permutation(s) for s in slates])
    for q, sl in rows(res):
        rd = eng.rank_domain(uids[q:q + 1], DOMAIN, [slates[q]], candidates=slates[q], want_scores=True)
        assert rd["listed"].all() and rd["live"][0] == slates[q].size
        want = dict(zip(rd["ids"].tolist(), rd["ranks"].tolist()))
        assert res["pos"][sl].tolist() == [want[i] for i in res["ids"][sl].tolist()], q
        sc = dict(zip(rd["ids"].tolist(), bits(rd["scores"]).tolist()))
        assert bits(res["scores"][sl]).tolist() == [sc[i] for i in res["ids"][sl].tolist()], q
        top = eng.recommend_domain(uids[q:q + 1], DOMAIN, 128, candidates=slates[q])[0][0]
        k = min(128, slates[q].size)
        assert np.array_equal(res["ids"][sl][res["order"][sl][:k]], top[:k]), q
        same_per_item(res, shuffled, q, q)
    eng.close()
    # ties across stages: every item row identical, so an entry's position is the number of smaller ids in its slate
    eng = make_big_engine(tied=True)
    tied = eng.rank_slates(uids, DOMAIN, slates)
    eng.close()
    for q, sl in rows(tied):
        assert np.unique(bits(tied["scores"][sl])).size == 1, q
        assert tied["pos"][sl].tolist() == np.argsort(np.argsort(tied["ids"][sl])).tolist(), q


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("tower", ["mlp", "deepfm"])
def test_exact_ties_order_by_id_wherever_the_entry_sits(tower):
    """every item row identical (test_exact_ties_rank_by_id_wherever_the_pair_sits' construction): one logit per query, so
    an entry's position is the number of smaller ids in its slate, wherever it sits in it."""
    params = base.make_params(False)
    params["item_emb"] = np.repeat(params["item_emb"][17:18], 346, axis=0)
    eng, _ = base.make_engine(tower, False, params)
    res = eng.rank_slates(users8(), DOMAIN, ragged_slates(43), want_order=True)
    eng.close()
    for q, sl in rows(res):
        ids = res["ids"][sl]
        assert np.unique(bits(res["scores"][sl])).size <= 1, q
        assert res["pos"][sl].tolist() == np.argsort(np.argsort(ids)).tolist(), q
        assert np.array_equal(ids[res["order"][sl]], np.sort(ids)), q


# ---------------------------------------------------------------------------------------------------------------- 5
def same_per_item(a, b, qa, qb):
    """query qa of result a and query qb of result b hold the same bytes per item id."""
    pa, pb = by_id(a, "pos"), by_id(b, "pos")
    sa = [dict(zip(a["ids"][sl].tolist(), bits(a["scores"][sl]).tolist())) for _, sl in rows(a)]
    sb = [dict(zip(b["ids"][sl].tolist(), bits(b["scores"][sl]).tolist())) for _, sl in rows(b)]
    assert pa[qa] == pb[qb] and sa[qa] == sb[qb], (qa, qb)


@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_neighbours_and_entry_order_change_no_byte(engines, tower, trainable):
    eng = engines(tower, trainable)
    uids, slates = users8(), ragged_slates()
    res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    again = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    assert all(res[n].tobytes() == again[n].tobytes() for n in ("offsets", "ids", "scores", "pos", "order"))
    rs = np.random.RandomState(47)
    shuffled = eng.rank_slates(uids, DOMAIN, [rs.permutation(s) for s in slates])
    assert not np.array_equal(shuffled["ids"], res["ids"])
    for q in range(8):
        same_per_item(res, shuffled, q, q)
    head, tail = eng.rank_slates(uids[:5], DOMAIN, slates[:5]), eng.rank_slates(uids[5:], DOMAIN, slates[5:])
    cut = res["offsets"][5]
    for n in ("scores", "pos"):
        assert head[n].tobytes() == res[n][:cut].tobytes() and tail[n].tobytes() == res[n][cut:].tobytes(), n
    # a call without entries returns empty arrays and launches nothing
    none = eng.rank_slates(uids[:3], DOMAIN, [[], [], []], want_order=True)
    assert none["offsets"].tolist() == [0, 0, 0, 0] and none["pos"].size == none["scores"].size == none["order"].size == 0


def many_queries():
    rs = np.random.RandomState(53)
    uids = rs.choice(1188, 300, replace=False).astype(np.int32)
    return uids, [rs.choice(346, 3 + q % 7, replace=False).astype(np.int32) for q in range(300)]


def test_a_second_query_block_changes_no_byte(engines):
    """300 queries with slates of 3 to 9 entries: query blocks of 256 + 44, pair tiles that span several queries."""
    eng = engines("mlp", False)
    uids, slates = many_queries()
    res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
    check_permutations(res)
    assert np.diff(res["offsets"]).tolist() == [3 + q % 7 for q in range(300)]
    a, b = eng.rank_slates(uids[:150], DOMAIN, slates[:150], want_order=True), eng.rank_slates(uids[150:], DOMAIN, slates[150:], want_order=True)
    cut = res["offsets"][150]
    for n in ("scores", "pos", "order"):
        assert a[n].tobytes() == res[n][:cut].tobytes() and b[n].tobytes() == res[n][cut:].tobytes(), n
    for q in (0, 1, 63, 149, 150, 255, 256, 257, 298, 299):
        one = eng.rank_slates(uids[q:q + 1], DOMAIN, slates[q:q + 1], want_order=True)
        sl = slice(res["offsets"][q], res["offsets"][q + 1])
        assert all(one[n].tobytes() == res[n][sl].tobytes() for n in ("scores", "pos", "order")), q


# ---------------------------------------------------------------------------------------------------------------- 6
def chunk_case(tower, trainable, path):
    """the calls of the chunking test, dumped to `path` (run in the test's process and in its child)."""
    eng, _ = base.make_engine(tower, trainable)
    out = {}
    for name, (uids, slates) in (("ragged", (users8(), ragged_slates())), ("many", many_queries())):
        res = eng.rank_slates(uids, DOMAIN, slates, want_order=True)
        out.update({"%s_%s" % (name, n): res[n] for n in ("scores", "pos", "order")})
    eng.close()
    np.savez(path, **out)


@pytest.mark.parametrize("tower,trainable", CASES, ids=CASE_IDS)
def test_chunking_does_not_change_a_bit(tmp_path, tower, trainable):
    """MAMDR_REC_CHUNK = 64 in a fresh child process (the switch is read at load): the entries of a query block pass through
    the workspace 64 at a time -- eleven passes over the ragged slates' 671 entries -- and every output is the bytes of the
    default run."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    chunk_case(tower, trainable, str(tmp_path / "one.npz"))
    code = "import test_gpu_slates as t; t.chunk_case(%r, %r, %r)" % (tower, trainable, str(tmp_path / "chunk64.npz"))
    env = dict(os.environ, MAMDR_REC_CHUNK="64",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(tmp_path / "one.npz")) as a, np.load(str(tmp_path / "chunk64.npz")) as b:
        assert sorted(a.files) == sorted(b.files) and len(a.files) == 6
        for name in a.files:
            assert a[name].size and a[name].tobytes() == b[name].tobytes(), name


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("tower", ["deepfm", "star"])
def test_rank_slates_reads_the_state_only(tower):
    """trainable tables, two Adam steps, then the call: weights, both Adam slots, the counters (Star: and the moving
    statistics) keep their digest, and an evaluation returns what it returned before the call."""
    g = base.gen()
    sizes = [g["data"]["train"][i]["uid"].shape[0] for i in range(10)]
    d = max((i for i in range(10) if i != DOMAIN), key=lambda i: sizes[i])
    if tower == "star":
        eng, digest = sbase.make_star_engine(True, bind=(d,))[0], sbase.state_digest
    else:
        eng, digest = base.make_engine(tower, True, bind=(d,))[0], base.state_digest
    eng.train_steps(d, n_steps=2)
    ev = eng.evaluate(d, "train", want_preds=True)
    before = digest(eng)
    first = eng.rank_slates(users8(), DOMAIN, ragged_slates(), want_order=True)
    assert digest(eng) == before
    ev2 = eng.evaluate(d, "train", want_preds=True)
    assert ev[0] == ev2[0] and ev[1] == ev2[1] and ev[-1].tobytes() == ev2[-1].tobytes()
    again = eng.rank_slates(users8(), DOMAIN, ragged_slates(), want_order=True)
    assert all(first[n].tobytes() == again[n].tobytes() for n in ("scores", "pos", "order"))
    assert digest(eng) == before
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("domain", [0, 3])
def test_star(domain):
    """the Star tower (sbase.make_star_engine: domains 0 and 3 carry moving statistics of their own)."""
    eng = sbase.make_star_engine(True)[0]
    uids, slates = users8(), ragged_slates()
    res = eng.rank_slates(uids, domain, slates, want_order=True)
    check_permutations(res)
    rd = eng.rank_domain(uids, domain, slates, want_scores=True)
    want = by_id(rd, "scores")
    ref = sbase.reference(domain)
    for q, sl in rows(res):
        w = np.asarray([want[q][i] for i in res["ids"][sl].tolist()], np.float32)
        assert np.array_equal(bits(res["scores"][sl]), bits(w)), q
        np.testing.assert_allclose(res["scores"][sl], ref[q % 7, res["ids"][sl]], rtol=sbase.RTOL, atol=sbase.ATOL)
    cand = rbase.parts()[0]
    rs = np.random.RandomState(59)
    one = eng.rank_slates(uids[:7], domain, [rs.permutation(cand) for _ in range(7)])
    ids = eng.recommend_domain(uids[:7], domain, 128, candidates=cand)[0]
    for q, sl in rows(one):
        assert np.array_equal(ids[q, one["pos"][sl]], one["ids"][sl]), q
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_refusals(engines):
    from mamdr_amd import _lib, graph_engine
    from mamdr_amd.engine import TowerEngine
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    uids = users7()
    slates = [[1, 2]] * 7
    for tower in ("pnn", "nfm"):
        eng = TowerEngine(1188, 346, 10, 256, tower=tower)
        with pytest.raises(_lib.NotBuiltError, match=r"\b%s tower" % tower):
            eng.rank_slates(uids, DOMAIN, slates)
        eng.close()
    geng = graph_engine.GraphEngine("mlp", 1188, 346, 10, 256, (128, 64), (), emb_dim=64)
    with pytest.raises(NotImplementedError, match="generic-layer towers"):
        geng.rank_slates(uids, DOMAIN, slates)
    geng.close()
    eng = engines("mlp", False)
    launched = []
    real = eng.lib.mamdr_rank_slates
    try:
        eng.lib.mamdr_rank_slates = lambda *a: launched.append(a) or 0
        for bad in (-1, 10, 3.0, True):
            with pytest.raises(ValueError):
                eng.rank_slates(uids, bad, slates)
        # an item id out of range; a duplicate inside a slate; a mismatched length
        for bad in ([[346]] * 7, [[-1]] * 7, [[1, 2]] * 6 + [[5, 9, 5]], [[1]] * 6, [[1]] * 8):
            with pytest.raises(ValueError):
                eng.rank_slates(uids, DOMAIN, bad)
        for bad in ([1188], [-1]):
            with pytest.raises(ValueError):
                eng.rank_slates(bad, DOMAIN, [[1]])
    finally:
        eng.lib.mamdr_rank_slates = real
    assert not launched                                        # refused on the host, before any launch
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    q = torch.zeros(2, dtype=torch.int32, device=eng.device)
    off = torch.tensor([0, 1, 3], dtype=torch.int64, device=eng.device)
    sid = torch.tensor([5, 9, 7], dtype=torch.int32, device=eng.device)
    pos = torch.full((5,), -7, dtype=torch.int32, device=eng.device)
    order = torch.full((5,), -7, dtype=torch.int32, device=eng.device)
    assert real(eng.ctx, 3, 2, p(q), p(off), p(sid), None, p(pos), p(order)) == _lib.OK
    assert pos.tolist()[0] == 0 and sorted(pos.tolist()[1:3]) == [0, 1] and pos.tolist()[3:] == [-7, -7]
    assert order.tolist()[0] == 0 and sorted(order.tolist()[1:3]) == [0, 1] and order.tolist()[3:] == [-7, -7]
    # duplicates share a position; the slot nobody claims keeps -1
    dup = torch.tensor([5, 9, 9], dtype=torch.int32, device=eng.device)
    assert real(eng.ctx, 3, 2, p(q), p(off), p(dup), None, p(pos), p(order)) == _lib.OK
    assert pos.tolist()[1:3] == [0, 0] and order.tolist()[1] in (0, 1) and order.tolist()[2] == -1
    # no entries: MAMDR_OK, nothing written
    pos.fill_(-7)
    empty = torch.zeros(3, dtype=torch.int64, device=eng.device)
    assert real(eng.ctx, 3, 2, p(q), p(empty), None, None, p(pos), p(order)) == _lib.OK
    assert pos.tolist() == [-7] * 5
    assert real(eng.ctx, 3, 2, p(q), None, p(sid), None, p(pos), None) == _lib.EINVAL
    assert b"mamdr_rank_slates" in eng.lib.mamdr_last_error()
    assert real(eng.ctx, 3, 2, p(q), p(off), p(sid), None, None, None) == _lib.EINVAL
    assert real(eng.ctx, 3, 2, p(q), p(off), None, None, p(pos), None) == _lib.EINVAL                     # entries exist
    assert real(eng.ctx, 3, 2, None, p(off), p(sid), None, p(pos), None) == _lib.EINVAL
    assert real(eng.ctx, 3, 0, p(q), p(off), p(sid), None, p(pos), None) == _lib.EINVAL
    assert real(eng.ctx, 3, 2, p(q), C.c_void_p(off.data_ptr() + 4), p(sid), None, p(pos), None) == _lib.EINVAL
    assert real(eng.ctx, 3, 2, p(q), p(off), C.c_void_p(sid.data_ptr() + 2), None, p(pos), None) == _lib.EINVAL
    late = torch.tensor([1, 2, 3], dtype=torch.int64, device=eng.device)                                   # offsets start at 1
    assert real(eng.ctx, 3, 2, p(q), p(late), p(sid), None, p(pos), None) == _lib.EINVAL
    down = torch.tensor([0, 2, 1], dtype=torch.int64, device=eng.device)
    assert real(eng.ctx, 3, 2, p(q), p(down), p(sid), None, p(pos), None) == _lib.EINVAL
    assert b"descend" in eng.lib.mamdr_last_error()
    for bad in (-1, 10):
        assert real(eng.ctx, bad, 2, p(q), p(off), p(sid), None, p(pos), None) == _lib.EINVAL
        assert b"domain %d" % bad in eng.lib.mamdr_last_error()
    assert pos.tolist() == [-7] * 5                            # none of the refused calls wrote
    raw = TowerEngine(1188, 346, 10, 256)                      # frozen tables, none bound
    assert real(raw.ctx, 3, 2, p(q), p(off), p(sid), None, p(pos), None) == _lib.ESTATE
    raw.close()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_run_py_with_sampled_eval(tmp_path):
    """run.py on the shipped Taobao-10 config as mlp_meta_mamdr (sized as test_run_config_with_recommend sizes its run) with
    --sampled-eval 50 --sampled-eval-ks 1,5.  On that data every test user has at least 187 free items in its domain
    (counted on the host: the data generation is host code), so no slate is short."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import recommend
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    cfg_path = str(tmp_path / "config.json")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    run = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "run.py"), "--config", cfg_path,
                          "--sampled-eval", str(E2E_NEG), "--sampled-eval-ks", "1,5"], cwd=str(tmp_path), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    text = run.stdout
    found = glob.glob(os.path.join(str(tmp_path / "result"), "**", "sampled_eval_neg%d.npz" % E2E_NEG), recursive=True)
    assert len(found) == 1, found
    assert "Sampled eval (%d negatives" % E2E_NEG in text and os.path.basename(found[0]) in text
    with np.load(found[0]) as z:
        want = {"domains", "ks", "n_neg", "seed", "mrr", "mean_percentile", "hit_rate", "recall", "ndcg", "n_short"}
        want |= {"%s_%d" % (n, d) for d in range(10) for n in ("users", "positives", "offsets", "ids", "scores", "pos", "rank")}
        assert set(z.files) == want
        assert z["domains"].tolist() == list(range(10)) and z["ks"].tolist() == [1, 5]
        assert int(z["n_neg"]) == E2E_NEG and int(z["seed"]) == 0
        assert z["n_short"].tolist() == [0] * 10
        n_pairs = 0
        for d in range(10):
            off, ids, scores, pos, rank = (z["%s_%d" % (n, d)] for n in ("offsets", "ids", "scores", "pos", "rank"))
            n = rank.size
            n_pairs += n
            assert off.shape == (n + 1,) and np.all(np.diff(off) == E2E_NEG + 1) and off[-1] == ids.size == scores.size == pos.size
            table, sc = ids.reshape(n, E2E_NEG + 1), scores.reshape(n, E2E_NEG + 1)
            assert np.array_equal(table[:, 0], z["positives_%d" % d]) and np.array_equal(rank, pos.reshape(n, -1)[:, 0])
            srt = np.sort(table, axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all()
            above, not_below = (sc[:, 1:] > sc[:, :1]).sum(1), (sc[:, 1:] >= sc[:, :1]).sum(1)
            assert np.all((above <= rank) & (rank <= not_below)), d
            m = recommend.rank_metrics(np.arange(n + 1), rank, np.ones(n, bool), np.diff(off), np.ones(n), [1, 5])
            assert m["mrr"] == z["mrr"][d] and m["mean_percentile"] == z["mean_percentile"][d]
            for name in ("hit_rate", "recall", "ndcg"):
                assert m[name].tolist() == z[name][d].tolist(), (d, name)
            line = re.search(r"^%d: MRR (\d\.\d{4}) HitRate@1 (\d\.\d{4}) NDCG@1 (\d\.\d{4}) HitRate@5 (\d\.\d{4}) NDCG@5 (\d\.\d{4}) "
                             r"\((\d+) pairs, 0 short slates" % d, text, flags=re.M)
            assert line, d
            assert [float(x) for x in line.groups()[:5]] == [float("%.4f" % v) for v in (
                m["mrr"], m["hit_rate"][0], m["ndcg"][0], m["hit_rate"][1], m["ndcg"][1])]
            assert int(line.group(6)) == n
        assert n_pairs == 1456 and z["mrr"].max() > 0
    print(text[text.index("Sampled eval"):])
