"""Per-user grouped AUC on the device (mamdr_group_auc, DeviceEngine.group_auc / evaluate(want_gauc=True), run.py --gauc).

The integers T_u and P_u are held to a brute force over all (positive, negative) pairs written here, the scalar to the
float64 value of the same terms within a relative G * 2^-52: both sides form every term r_u * (T_u / (2 P_u N_u)) by the
same two correctly rounded operations, so they differ in the order of the sum alone, and any two orders of G non-negative
terms are within (G - 1) * 2^-53 of the exact sum each.

Shapes: one crafted split of about 6,000 rows -- group sizes 1, 2, 63, 64, 65 (the wave path's edge and the first tiled
size), 255, 256, 257 (a full tile and its remainders), 513 and 1,100 (three and five tiles) plus 200 groups of 1 .. 30 rows;
one split of 2,049 groups of two rows (one more group than a block of k_gauc_terms takes: the finish adds two partials);
the engines run at tests/test_gpu_recommend.py's problem (taobao10 at scale 0.05: 1,188 users, 10 domains).
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import gauc      # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 513, 1100]

_CACHE = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def bound(n_groups):
    """relative distance allowed between two summation orders of n_groups non-negative terms."""
    return n_groups * 2.0 ** -52


def brute_force(pred, label, uid):
    """every (positive, negative) pair of every user, compared under the definition's three rules ->
    (uids ascending, T, P, rows) as int64 arrays."""
    pred, label, uid = np.asarray(pred, F32), np.asarray(label), np.asarray(uid)
    users = np.unique(uid)
    T, P, R = [], [], []
    for u in users:
        rows = uid == u
        p, q = pred[rows & (label != 0)].astype(np.float64), pred[rows & (label == 0)].astype(np.float64)
        pn, qn = np.isnan(p)[:, None], np.isnan(q)[None, :]
        with np.errstate(invalid="ignore"):
            above = (~pn & qn) | (~pn & ~qn & (p[:, None] > q[None, :]))
            level = (pn & qn) | (~pn & ~qn & (p[:, None] == q[None, :]))         # (IEEE: -0.0 == 0.0)
        T.append(2 * int(above.sum()) + int(level.sum()))
        P.append(p.size)
        R.append(int(rows.sum()))
    return users, np.array(T, np.int64), np.array(P, np.int64), np.array(R, np.int64)


def float64_report(T, P, R):
    N = R - P
    valid = (P > 0) & (N > 0)
    terms = R[valid].astype(np.float64) * (T[valid].astype(np.float64) / (2 * P[valid] * N[valid]).astype(np.float64))
    return gauc.finish(float(terms.sum()), int(R[valid].sum()), int(valid.sum()), R.size)


def crafted():
    """the crafted split and its brute force: computed once, never modified."""
    if "crafted" not in _CACHE:
        rs = np.random.RandomState(17)
        sizes = np.array(BIG_SIZES + rs.randint(1, 31, 200).tolist())
        users = rs.permutation(100000)[:sizes.size]
        uid = np.repeat(users, sizes).astype(np.int32)
        # per-user click rate: 0 for some users, 1 for others -> all-negative and all-positive groups occur
        rate = rs.choice([0.0, 0.15, 0.5, 1.0], sizes.size, p=[0.1, 0.5, 0.3, 0.1])
        rate[:len(BIG_SIZES)] = [1.0, 0.5, 0.3, 0.5, 0.2, 0.0, 0.4, 0.1, 0.3, 0.25]
        label = (rs.random_sample(uid.size) < np.repeat(rate, sizes)).astype(F32)
        pred = (rs.randint(0, 16, uid.size) / 16.0).astype(F32)          # 16 levels: ties abound
        file_order = rs.permutation(uid.size)
        uid, label, pred = uid[file_order], label[file_order], pred[file_order]
        users_sorted, T, P, R = brute_force(pred, label, uid)
        for a in (uid, label, pred, T, P, R):
            a.setflags(write=False)
        _CACHE["crafted"] = dict(uid=uid, label=label, pred=pred, T=T, P=P, R=R, users=users_sorted)
    return _CACHE["crafted"]


def device_call(pred, label, plan, want_groups=True):
    """the stateless export on torch's current stream -> (report, T, P, the four result doubles' bytes)."""
    from mamdr_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, t: torch.from_numpy(np.array(a, dtype=t)).to(dev)      # noqa: E731 (a writable, contiguous copy)
    d_pred, d_label = up(pred, F32), up(label, F32)
    d_order, d_off = up(plan.order, np.int32), up(plan.group_off, np.int64)
    d_tg, d_tf = up(plan.tile_group, np.int32), up(plan.tile_first, np.int64)
    n, G, nt = plan.order.size, plan.group_off.size - 1, plan.tile_group.size
    T = torch.full((max(G, 1),), -1, dtype=torch.int64, device=dev) if want_groups else None
    P = torch.full((max(G, 1),), -1, dtype=torch.int32, device=dev) if want_groups else None
    res = torch.full((4,), -1.0, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
    L.check(lib.mamdr_group_auc(ptr(d_pred), ptr(d_label), ptr(d_order), n, ptr(d_off), G, ptr(d_tg) if nt else None,
                                ptr(d_tf) if nt else None, nt, ptr(T), ptr(P), ptr(res),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = res.cpu().numpy()
    rep = gauc.finish(*out.tolist())
    if not want_groups:
        return rep, None, None, out.tobytes()
    return rep, T.cpu().numpy()[:G], P.cpu().numpy()[:G], out.tobytes()


# ------------------------------------------------------------------ the stateless call
def test_crafted_groups_match_brute_force():
    need_gpu()
    c = crafted()
    plan = gauc.group_plan(c["uid"])
    assert 5500 <= c["uid"].size <= 6500 and plan.tile_group.size == 1 + 1 + 1 + 2 + 3 + 5
    assert np.any((c["P"] == c["R"]) & (c["R"] > 1)) and np.any((c["P"] == 0) & (c["R"] > 1))     # one-class groups occur
    rep, T, P, bits = device_call(c["pred"], c["label"], plan)
    print("crafted: device", rep)
    assert np.array_equal(T, c["T"]), np.flatnonzero(T != c["T"])[:10]
    assert np.array_equal(P, c["P"]), np.flatnonzero(P != c["P"])[:10]
    want = float64_report(c["T"], c["P"], c["R"])
    print("crafted: float64", want)
    assert (rep["n_groups"], rep["n_valid"], rep["rows_valid"]) == (want["n_groups"], want["n_valid"], want["rows_valid"])
    assert want["n_groups"] == 210 and 0 < want["n_valid"] < 210
    print("crafted: relative difference %.3e, bound %.3e" % (abs(rep["gauc"] - want["gauc"]) / want["gauc"], bound(210)))
    assert abs(rep["gauc"] - want["gauc"]) <= bound(210) * want["gauc"]
    # the host definition (another algorithm: sort and mid-ranks) gives the same integers
    host = gauc.group_auc_host(c["pred"], c["label"], c["uid"], want_groups=True)
    assert np.array_equal(host["T"].astype(np.int64), c["T"]) and np.array_equal(host["P"].astype(np.int64), c["P"])
    # a second run, and a run without the optional outputs: the same bits
    assert device_call(c["pred"], c["label"], plan)[3] == bits
    assert device_call(c["pred"], c["label"], plan, want_groups=False)[3] == bits


def test_exact_values():
    need_gpu()
    rs = np.random.RandomState(3)
    sizes = np.array([2, 5, 64, 65, 300, 700] + rs.randint(2, 20, 40).tolist())
    uid = np.repeat(np.arange(sizes.size), sizes).astype(np.int32)
    label = np.zeros(uid.size, F32)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for s, r in zip(start, sizes):                       # every user has both classes
        label[s:s + max(1, r // 3)] = 1
    shuffle = rs.permutation(uid.size)
    uid, label = uid[shuffle], label[shuffle]
    plan = gauc.group_plan(uid)
    n_rows, n_users = int(uid.size), int(sizes.size)
    # all predictions equal: every pair ties
    rep = device_call(np.full(uid.size, 0.3, F32), label, plan)[0]
    assert rep == {"gauc": 0.5, "n_groups": n_users, "n_valid": n_users, "rows_valid": n_rows}
    # a perfect ranking, and its inverse
    score = (label * 2 - 1) * (1 + rs.random_sample(uid.size)).astype(F32)
    assert device_call(score.astype(F32), label, plan)[0]["gauc"] == 1.0
    assert device_call((-score).astype(F32), label, plan)[0]["gauc"] == 0.0
    # nobody valid: 0.0 with n_valid 0; an empty split
    rep = device_call(score.astype(F32), np.ones(uid.size, F32), plan)[0]
    assert rep == {"gauc": 0.0, "n_groups": n_users, "n_valid": 0, "rows_valid": 0}
    rep = device_call(np.zeros(0, F32), np.zeros(0, F32), gauc.group_plan(np.zeros(0, np.int32)))[0]
    assert rep == {"gauc": 0.0, "n_groups": 0, "n_valid": 0, "rows_valid": 0}
    # NaN below -inf, NaN == NaN, -0 == +0: in a wave-path group (7 rows) and in a tiled one (the same 7 rows x 20)
    nan, ninf = np.nan, -np.inf
    pred7 = np.array([nan, ninf, nan, -0.0, 0.0, ninf, 1.0], F32)
    lab7 = np.array([1, 0, 0, 1, 0, 1, 0], F32)
    # positives nan, -0, -inf against negatives -inf, nan, +0, 1: nan (0 1 0 0) + -0 (2 2 1 0) + -inf (1 2 0 0) = 9
    pred, label, uid = np.concatenate([pred7, np.tile(pred7, 20)]), np.concatenate([lab7, np.tile(lab7, 20)]), \
        np.concatenate([np.zeros(7, np.int32), np.ones(140, np.int32)])
    rep, T, P, _ = device_call(pred, label, gauc.group_plan(uid))
    assert T.tolist() == [9, 9 * 400] and P.tolist() == [3, 60]
    users, bT, bP, _ = brute_force(pred, label, uid)
    assert bT.tolist() == T.tolist() and bP.tolist() == P.tolist()
    assert rep["gauc"] == (7 * (9 / 24.0) + 140 * (3600 / 9600.0)) / 147


def two_row_groups(G, rs):
    """G users of one positive and one negative row each, seven of them with two positives instead (never the user of the
    highest id), predictions on 4 levels (wins, ties and losses), in a shuffled file order -> (pred, label, uid)."""
    uid = np.repeat(np.sort(rs.permutation(100000)[:G]), 2).astype(np.int32)
    label = np.tile(np.array([1, 0], F32), G)
    label[2 * rs.choice(G - 1, 7, replace=False) + 1] = 1
    pred = (rs.randint(0, 4, uid.size) / 4.0).astype(F32)
    file_order = rs.permutation(uid.size)
    return pred[file_order], label[file_order], uid[file_order]


def test_more_groups_than_one_block_of_terms():
    """2,049 groups of two rows: k_gauc_terms writes two partials (a block takes 2,048 groups) and k_gauc_finish adds more
    than one.  Held to the brute force as the crafted split is."""
    need_gpu()
    rs = np.random.RandomState(29)
    G = 2049
    pred, label, uid = two_row_groups(G, rs)
    plan = gauc.group_plan(uid)
    assert plan.group_off.size - 1 == G and plan.tile_group.size == 0
    rep, T, P, bits = device_call(pred, label, plan)
    _, bT, bP, bR = brute_force(pred, label, uid)
    assert np.array_equal(T, bT) and np.array_equal(P, bP)
    assert bP[-1] == 1 and set(bT.tolist()) == {0, 1, 2}          # the second block's one group counts; every outcome occurs
    want = float64_report(bT, bP, bR)
    assert (rep["n_groups"], rep["n_valid"], rep["rows_valid"]) == (want["n_groups"], want["n_valid"], want["rows_valid"])
    assert (want["n_groups"], want["n_valid"], want["rows_valid"]) == (G, G - 7, 2 * (G - 7))
    print("2049 groups: relative difference %.3e, bound %.3e" % (abs(rep["gauc"] - want["gauc"]) / want["gauc"], bound(G)))
    assert abs(rep["gauc"] - want["gauc"]) <= bound(G) * want["gauc"]
    # a second run, and the same rows in another file order: the same bits
    assert device_call(pred, label, plan)[3] == bits
    p = rs.permutation(uid.size)
    assert device_call(pred[p], label[p], gauc.group_plan(uid[p]))[3] == bits


def test_invariance_under_row_and_member_order():
    need_gpu()
    c = crafted()
    plan = gauc.group_plan(c["uid"])
    rep, T, P, bits = device_call(c["pred"], c["label"], plan)
    # the same rows in another file order, with a fresh plan
    rs = np.random.RandomState(8)
    p = rs.permutation(c["uid"].size)
    rep2, T2, P2, bits2 = device_call(c["pred"][p], c["label"][p], gauc.group_plan(c["uid"][p]))
    assert np.array_equal(T2, T) and np.array_equal(P2, P) and bits2 == bits
    # the same groups with their members listed in a different order inside `order`
    order = plan.order.copy()
    for g in range(plan.group_off.size - 1):
        lo, hi = plan.group_off[g], plan.group_off[g + 1]
        order[lo:hi] = order[lo:hi][rs.permutation(hi - lo)]
    assert not np.array_equal(order, plan.order)
    rep3, T3, P3, bits3 = device_call(c["pred"], c["label"], plan._replace(order=order))
    assert np.array_equal(T3, T) and np.array_equal(P3, P) and bits3 == bits


# ------------------------------------------------------------------ the engines
def gen():
    if "g" not in _CACHE:
        from mamdr_amd import synthetic
        _CACHE["g"] = synthetic.generate("taobao10", batch_size=256, seed=7, scale=0.05)
    return _CACHE["g"]


def make_engine(which):
    """TowerEngine mlp / GraphEngine mlp (hidden [128, 64]) with frozen tables, every test split bound, random weights."""
    from mamdr_amd import engine, graph_engine
    g = gen()
    if which == "tower":
        eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 256, dropout=0.5, emb_trainable=False, tower="mlp")
    else:
        eng = graph_engine.GraphEngine("mlp", g["n_user"], g["n_item"], g["n_domain"], 256, (128, 64), (), dropout=0.5)
    eng.bind_table("user_emb", g["tables"]["user_emb"])
    eng.bind_table("item_emb", g["tables"]["item_emb"])
    for d in range(g["n_domain"]):
        c = g["data"]["test"][d]
        eng.bind_domain_data(d, "test", c["uid"], c["pid"], c["domain"], c["label"])
    rs = np.random.RandomState(7)
    named = {n: (rs.standard_normal(cnt) * (0.0 if n in ("user_emb", "item_emb") else 0.08)).astype(F32)
             for n, (off, cnt) in eng.segments.items()}
    eng.set_weights(eng.pack(named))
    return eng


def check_against_host(eng, d, cols):
    """evaluate(want_gauc) of the bound split against group_auc_host on the predictions it returns."""
    plain = eng.evaluate(d, "test", want_preds=True)
    both = eng.evaluate(d, "test", want_preds=True, want_gauc=True)
    only = eng.evaluate(d, "test", want_gauc=True)
    assert len(plain) == 4 and len(both) == 5 and len(only) == 3
    # loss, histogram and predictions: the bits of a call without want_gauc
    assert plain[0] == both[0] == only[0] and plain[1] == both[1] == only[1]
    assert np.array_equal(plain[2], both[2]) and plain[3].tobytes() == both[3].tobytes()
    assert eng.evaluate(d, "test") == plain[:2]
    rep = both[4]
    assert only[2] == rep
    host = gauc.group_auc_host(both[3], cols["label"], cols["uid"], want_groups=True)
    # the integers through group_auc on device tensors
    dev = eng.group_auc(torch.from_numpy(both[3]).to(eng.device), eng.data[(d, "test")]["label"],
                        eng.group_auc_plan(d, "test"), want_groups=True)
    assert np.array_equal(dev["T"], host["T"]) and np.array_equal(dev["P"], host["P"])
    assert dev["T"].dtype == np.uint64 and dev["P"].dtype == np.uint32
    for k in ("n_groups", "n_valid", "rows_valid"):
        assert rep[k] == host[k] == dev[k], k
    assert dev["gauc"] == rep["gauc"]                       # the same call twice: the same bits
    assert abs(rep["gauc"] - host["gauc"]) <= bound(host["n_groups"]) * host["gauc"]
    return rep, host


@pytest.mark.parametrize("which", ["tower", "graph"])
def test_engine_evaluate_with_gauc(which):
    need_gpu()
    g = gen()
    eng = make_engine(which)
    total_valid = 0
    for d in (0, 4, 9):
        rep, host = check_against_host(eng, d, g["data"]["test"][d])
        print("%s engine, domain %d: %s (host %.17g)" % (which, d, rep, host["gauc"]))
        total_valid += rep["n_valid"]
    assert total_valid > 0
    # re-binding a (domain, split) with other rows: the new data's grouping and value
    before = eng.evaluate(0, "test", want_gauc=True)[2]
    other = g["data"]["test"][4]
    eng.bind_domain_data(0, "test", other["uid"], other["pid"], np.zeros_like(other["domain"]), other["label"])
    rep, host = check_against_host(eng, 0, other)
    assert rep["n_groups"] == np.unique(other["uid"]).size and (rep["n_groups"], rep["rows_valid"]) != (before["n_groups"], before["rows_valid"])
    eng.close()


# ------------------------------------------------------------------ end to end
def test_run_config_with_gauc(tmp_path, capsys):
    """run.py's entry on the shipped Taobao-10 config (sized as tests/test_gpu_recommend.py's test_run_config_with_recommend
    sizes its run) with train.report_gauc.  No quality bar: at scale 0.1, batch 256, the generator alone leaves 7 to 222
    valid users in every sampled domain's test split."""
    need_gpu()
    from mamdr_amd import cli, engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name="mlp_meta_mamdr")
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5, report_gauc=True,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    res = cli.main(cfg, on_model=built.append)
    assert len(res) == 4 and len(res[3]) == 10
    model = built[0]
    assert isinstance(model.model, engine.TowerEngine)
    rdir = os.path.join(model.result_path, os.listdir(model.result_path)[0])
    with open(os.path.join(rdir, "result.json")) as f:
        result = json.load(f)
    assert {"avg_gauc", "weighted_gauc", "domain_gauc", "domain_gauc_users"} <= set(result)
    assert set(result["domain_gauc"]) == set(result["domain_gauc_users"]) == {str(d) for d in range(10)}
    assert all(0.0 <= v <= 1.0 for v in result["domain_gauc"].values())
    assert 0.0 <= result["avg_gauc"] <= 1.0 and 0.0 <= result["weighted_gauc"] <= 1.0
    assert sum(result["domain_gauc_users"].values()) > 0
    text = capsys.readouterr().out
    assert "Overall test GAUC: {}, Weighted GAUC: {}".format(result["avg_gauc"], result["weighted_gauc"]) in text
    print(text[text.rindex("GAUC: \n"):])
    print("valid users per domain:", result["domain_gauc_users"])
