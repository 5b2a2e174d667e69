"""Every loss head at saturated predictions: k_tower (step_kernels.hip, 16-row tiles, training and evaluation, the Star
tower), k_tower4 (tower4_kernels.hip, 4-row tiles, training) and k_graph_head (graph_engine.hip, every generic-layer kind)
against the oracles, on batches that tests/saturation.py builds from the ORACLE's logits: rows outside the Keras clip
[1e-7, 1 - 1e-7] (saturated, 20 <= |z| <= 80; extreme, 100 <= |z| <= 1000), normal rows (|z| <= 6), nothing in between.

1. all-saturated batches (5 rows: one 4-row tile plus one row; 1 row), one SGD step at lr 1 and one Adam step: the
   clip's zero gradient (`inside`) leaves every tensor without a regulariser term bit-unchanged and its Adam slots exactly
   zero; the others (the domain table, the linear domain table, the uncertainty scalars, trainable tables) move by that
   term alone; the loss is a mean of the four clipped constants.
2. a mixed batch of 24 rows (8 normal, 16 clipped, every clipped class with both labels): every gradient against the oracle
   at the suite's one-step bars, and the 1-row batch whose single row is saturated the wrong way.
3. evaluation of a bound split of 24 such rows: predictions, exact 1.0f / < 1e-7 at the extremes, exact AUC bins, loss.
4. top-K retrieval among candidates whose scores all round to 1.0f: ordered by logit.

Bars: the suite's existing ones -- one-step gradients rtol 2e-4, atol max(2e-6 max|want|, 1.5e-8) (4e-8 for the user / item
tables, 1e-7 under uncertainty weighting; the Star family's own: rtol 5e-4, atol max(4e-6 max|want|, its floors)); loss
2e-6 max(1, |loss|); predictions rtol 2e-5 on the normal rows, atol 2e-7.  Two additions, both reasoned:
* the SGD probe reads a gradient back as w0 - (w0 - g), quantised to the ulp of the WEIGHT (the existing floors are that ulp
  at |w| ~ 0.1); saturation.py gives the output kernel weights up to ~1e4, so half an ulp of each element's weight is added
  to its atol.
* a normal row's loss moves by 2^-24 (1 + e^|z|) per ulp of p.  The loss bars add (k / B) times the sum of that over the
  normal rows, k = ULPS[head]: twice the largest ulp distance between the device's and the oracle's predictions measured
  over the normal rows of the evaluation tests below, rounded up (profiles/saturation_heads.txt).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import saturation as sat                            # noqa: E402
from oracle import auc as oauc                      # noqa: E402
from oracle import tower as otower                  # noqa: E402

F32 = np.float32
H3 = (256, 128, 64)
B = 24
# twice the largest measured ulp distance of p on the normal evaluation rows, per head (profiles/saturation_heads.txt);
# k_tower4 has no evaluation mode: its sigmoid is k_tower's expression, and it takes k_tower's figure
ULPS = {"k_tower": 22, "k_tower4": 22, "k_graph_head": 72}
# tensors with a term of the loss of their own (the user / item tables: segments of the flat vector only when trainable)
REGULARISED = ("domain_emb", "lin_domain", "log_var", "user_emb", "item_emb", "lin_user", "lin_item")

# (id, builder, arguments): the coverage table of the issue
STEP_ROUTES = [("%s-tile%d-drop%s" % (k, t, r), "step", dict(kind=k, tile=t, dropout=r))
               for k, tiles in (("mlp", (4, 16)), ("deepfm", (4, 16)), ("pnn", (4,)), ("nfm", (4,))) for t in tiles
               for r in (0.5, 0.0)]
STEP_ROUTES += [("mlp-uncertainty-tile%d" % t, "step", dict(kind="mlp", tile=t, dropout=0.5, uncertainty=True)) for t in (4, 16)]
STEP_ROUTES += [("star-tile16", "star", {})]
GRAPH_ROUTES = [("graph-mlp", "hidden", dict(dropout=0.5)), ("graph-nfm", "fm", dict(kind="nfm", dropout=0.5)),
                ("graph-autoint", "fm", dict(kind="autoint", dropout=0.5)), ("graph-mmoe", "mtl", dict(dropout=0.5)),
                ("graph-star-pn-star-aux64", "starform", {}), ("graph-mlp-uncertainty", "hidden", dict(dropout=0.5, uncertainty=True))]
TRAINABLE_ROUTES = [("%s-trainable-tile%d" % (k, t), "step", dict(kind=k, tile=t, dropout=0.5, trainable=True))
                    for k in ("mlp", "deepfm") for t in (4, 16)]
FROZEN = STEP_ROUTES + GRAPH_ROUTES


def ids(routes):
    return [r[0] for r in routes]


def largest(g):
    return max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])


class Case(object):
    """one engine with its oracle (the existing make_problem functions), the largest domain's train split, the head that
    serves it, and the saturated parameters on both sides."""

    def __init__(self, builder, kind="mlp", tile=0, dropout=0.0, trainable=False, uncertainty=False, inference=False):
        if not torch.cuda.is_available():
            pytest.skip("no HIP device")
        from mamdr_amd import engine, synthetic
        env, spec = (engine, synthetic), None
        if builder == "step" and kind in ("mlp", "deepfm"):
            from test_gpu_parity import make_problem
            g, eng, model = make_problem(env, scale=0.05, batch=B, dropout=dropout, emb_trainable=trainable, tower=kind,
                                         uncertainty=uncertainty)
            family = "tower"
        elif builder == "step":
            from test_gpu_fmnets import make_problem
            g, eng, model = make_problem(kind + "@step", batch=B, dropout=dropout)
            family = "fm"
        elif builder == "star":
            from test_gpu_parity import make_star_problem
            g, eng, model = make_star_problem(env, False, scale=0.05, batch=B)
            family, tile = "star", 16
        elif builder == "fm":
            from test_gpu_fmnets import make_problem
            g, eng, model = make_problem(kind, batch=B, dropout=dropout)
            family = "fm"
        elif builder == "mtl":
            from test_gpu_mtl import make_problem
            g, eng, model, spec = make_problem("mmoe", batch=B, dropout=dropout)
            family = "mtl"
        elif builder == "starform":
            from test_gpu_star_forms import build, problem
            g = problem(scale=0.05, batch=B)
            eng, model, _ = build(g, "pn", "star", 64, H3, batch=B)
            family = "starform"
        elif uncertainty:
            g, eng, model = graph_mlp_uncertainty(dropout)
            family = "tower"
        else:
            from test_gpu_hidden import make_problem
            g, eng, model = make_problem("mlp", (128, 64), batch=B, dropout=dropout)
            family = "tower"
        self.g, self.eng, self.model, self.family = g, eng, model, family
        self.star = family in ("star", "starform")
        self.uncertainty = uncertainty
        self.d = largest(g)
        self.cols = g["data"]["train"][self.d]
        if builder in ("step", "star"):
            # the intended kernel: the 4-row tower k_tower4 or the 16-row one k_tower (the Star tower's only one)
            # (evaluation is k_tower's inference instance whatever the tile)
            if builder == "step" and not inference:
                eng.set_tower_tile(tile)
            if not inference:
                assert eng.tower_tile(B) == tile and eng.tower_tile(5) == tile and eng.tower_tile(1) == tile
                assert int(eng.lib.mamdr_step_path(eng.ctx, B)) in (0, 1)
            self.head = "k_tower4" if tile == 4 and not inference else "k_tower"
        else:
            self.head = "k_graph_head"
        self.prob = sat.Problem(family, model, self.cols, self.d, spec)
        _, self.guess = sat.saturate(self.prob, inference=inference)
        self.gb = model.params[self.prob.gb_name].copy()
        self.reset()

    def reset(self):
        """a test starts here: the saturated parameters as `saturate` left them, no row taken."""
        self.model.params[self.prob.gb_name][...] = self.gb
        self.taken = []
        self.load()

    def load(self):
        """the oracle's parameters onto the device, Adam slots and step count zeroed."""
        self.w0 = self.eng.pack(self.model.params)
        self.eng.set_weights(self.w0)
        self.eng.optimizer_reset()

    def pick(self, layout, step):
        gb = self.model.params[self.prob.gb_name].copy()
        step, idx, z = sat.pick(self.prob, layout, step, guess=self.guess, exclude=self.taken)
        self.taken += [int(i) for i in idx]
        if not np.array_equal(gb, self.model.params[self.prob.gb_name]):       # (the Star family's single row: bias moved)
            self.load()
        return step, idx, z

    def step(self, idx, step, optimizer, lr):
        """one training step on the rows `idx` at dropout step `step` from the loaded parameters -> (loss, weights after)."""
        eng = self.eng
        eng.set_weights(self.w0)
        eng.optimizer_reset()
        eng.set_counters(0, step)
        loss_t = torch.zeros(1, device=eng.device)
        perm = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(eng.device)
        assert eng.train_steps(self.d, perm=perm, first_step=0, n_steps=1, lr=lr, optimizer=optimizer, loss_out=loss_t,
                               batch_size=B, pass_rows=len(idx)) == 1
        return float(loss_t.cpu()[0]), eng.get_weights()

    def close(self):
        self.eng.close()


def graph_mlp_uncertainty(dropout):
    """tests/test_gpu_hidden.py:make_problem("mlp", (128, 64)) under the weighted loss (no existing make_problem builds the
    generic engine's mlp with it): the same data, seed and perturbations, log_var as tests/test_gpu_parity.py draws it."""
    from mamdr_amd import graph_engine, synthetic
    hidden = (128, 64)
    g = synthetic.generate("taobao10", batch_size=B, seed=7, scale=0.05)
    D = g["n_domain"]
    rs = np.random.RandomState(7)
    params = otower.init_params(rs, g["n_user"], g["n_item"], D, hidden=hidden)
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for n in ["b0", "b1"]:
        params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    params["gb"] = np.array([0.1], F32)
    params["log_var"] = (1.0 + rs.uniform(-0.3, 0.3, D)).astype(F32)
    eng = graph_engine.GraphEngine("mlp", g["n_user"], g["n_item"], D, B, hidden, (), dropout=dropout, uncertainty_weight=True)
    eng.bind_table("user_emb", params["user_emb"])
    eng.bind_table("item_emb", params["item_emb"])
    for split in ("train", "val"):
        for d in range(D):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
    model = otower.OracleModel({k: v.copy() for k, v in params.items()}, dropout=dropout, lr=1e-3, hidden=hidden,
                               dropout_seed=eng.dropout_seed, tower="mlp", uncertainty=True)
    assert list(eng.segments) == list(model.names), (list(eng.segments), model.names)
    eng.set_weights(eng.pack(params))
    return g, eng, model


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def dense(grads, name, like):
    g = grads.get(name)
    return np.zeros(like.size, F32) if g is None else np.asarray(otower.bigtable.densify(g), F32).ravel()


def assert_gradients(case, got, w0, grads, after):
    """`got` = w0 - after of an SGD step at lr 1, per tensor, against the oracle's `grads` at the suite's one-step bars; a
    tensor whose gradient is exactly zero in the oracle (off the task's path, an idle domain's slice, every tensor without a
    regulariser term when the whole batch is clipped) must be bit-unchanged."""
    for name in got:
        want = dense(grads, name, got[name])
        if not want.any():
            assert np.array_equal(bits(after[name]), bits(w0[name])), name
            continue
        scale = float(np.abs(want).max())
        readback = 0.5 * np.spacing(np.abs(w0[name]).astype(F32)).astype(np.float64)
        if case.star:
            if name == "domain_emb":    # constant over a single-domain batch under the norm: rounding residue on both sides
                assert np.abs(got[name]).max() < 1e-5 and scale < 1e-5
                continue
            floor = 2e-7 if "gamma" in name else (6e-8 if name.startswith("Wd") else 3e-8)
            rtol, atol = 5e-4, max(4e-6 * max(scale, 1e-3), floor)
        else:
            floor = 1e-7 if case.uncertainty else (4e-8 if name in ("user_emb", "item_emb") else 1.5e-8)
            rtol, atol = 2e-4, max(2e-6 * scale, floor)
        err = np.abs(got[name].astype(np.float64) - want)
        bad = err > np.maximum(atol, readback) + rtol * np.abs(want)
        assert not bad.any(), (name, int(bad.sum()), float(err.max()), atol, scale)


@pytest.fixture(scope="module", params=FROZEN + TRAINABLE_ROUTES, ids=ids(FROZEN + TRAINABLE_ROUTES))
def train_case(request):
    """one Case per route, shared by the training tests (pytest runs the tests of one module-scoped parameter together:
    one engine alive at a time)."""
    case = Case(request.param[1], **request.param[2])
    case.route = request.param
    yield case
    case.close()


@pytest.fixture
def case(train_case):
    train_case.reset()
    return train_case


# ---------------------------------------------------------------------------------------------------------------- 1
def test_all_saturated_batches_move_nothing_but_the_regularised_tensors(case):
    """every row outside the clip, wrong-way rows included (label 0 with p -> 1: the largest p - y there is, and exactly
    the gradient Keras zeroes).  No tolerance on the data gradient: a head that drops `inside` on a single row moves
    every kernel and bias.  (Trainable tables are regularised tensors too: they move by their l2 term alone.)"""
    route = case.route
    eng, prob = case.eng, case.prob
    step = 1
    for layout in (sat.ALL_SATURATED_5, sat.ALL_SATURATED_1):
        step, idx, z = case.pick(layout, step)
        loss, grads, _ = prob.loss_and_grads(idx, step)
        w0 = eng.unpack(case.w0)
        # one SGD step at lr 1
        got_loss, after_t = case.step(idx, step, "sgd", 1.0)
        after = eng.unpack(after_t)
        got = eng.unpack(case.w0 - after_t)
        print("%s rows %d: loss hip %.7f oracle %.7f" % (route[0], len(idx), got_loss, float(loss)))
        assert abs(got_loss - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
        for name in got:
            if name not in REGULARISED or case.star:
                assert np.array_equal(bits(after[name]), bits(w0[name])), (name, len(idx))
        assert_gradients(case, got, w0, grads, after)
        # one Adam step: zero slots, bit-unchanged weights; m = (1 - beta1) g on the regularised tensors
        _, after_t = case.step(idx, step, "adam", 1e-3)
        after, m, v = eng.unpack(after_t), eng.unpack(eng.adam_m), eng.unpack(eng.adam_v)
        for name in after:
            if name not in REGULARISED or case.star:
                assert np.array_equal(bits(after[name]), bits(w0[name])), (name, len(idx))
                assert not m[name].any() and not v[name].any(), (name, len(idx))
            else:
                want = dense(grads, name, m[name])
                floor = 1e-7 if case.uncertainty else 1.5e-8
                np.testing.assert_allclose(m[name] / F32(0.1), want, rtol=2e-4, atol=max(2e-6 * np.abs(want).max(), floor),
                                           err_msg=name)
        step += 1


# ---------------------------------------------------------------------------------------------------------------- 2
def test_mixed_batch_gradients_match_oracle(case):
    """8 normal and 16 clipped rows in one batch of 24 (one and a half 16-row tiles, six 4-row tiles, rows_pad 64 on the
    generic engine): the clipped rows contribute nothing, the normal rows everything, padding rows neither -- every
    gradient and the loss against the oracle; then the remainder row alone, saturated the wrong way."""
    route = case.route
    eng, prob = case.eng, case.prob
    step, idx, z = case.pick(sat.MIXED, 0)
    loss, grads, _ = prob.loss_and_grads(idx, step)
    normal = np.abs(z) <= sat.NORMAL_MAX
    got_loss, after_t = case.step(idx, step, "sgd", 1.0)
    w0 = eng.unpack(case.w0)
    bar = 2e-6 * max(1.0, abs(float(loss))) + sat.loss_slack(z, normal, ULPS[case.head])
    print("%s: loss hip %.7f oracle %.7f bar %.3g" % (route[0], got_loss, float(loss), bar))
    assert abs(got_loss - float(loss)) < bar
    assert_gradients(case, eng.unpack(case.w0 - after_t), w0, grads, eng.unpack(after_t))
    step, idx, z = case.pick(sat.ALL_SATURATED_1, step + 1)
    loss, grads, _ = prob.loss_and_grads(idx, step)
    got_loss, after_t = case.step(idx, step, "sgd", 1.0)
    w0 = eng.unpack(case.w0)
    assert abs(got_loss - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
    assert_gradients(case, eng.unpack(case.w0 - after_t), w0, grads, eng.unpack(after_t))


# ---------------------------------------------------------------------------------------------------------------- 3
EVAL_ROUTES = [("mlp-eval", "step", dict(kind="mlp", tile=0)), ("deepfm-eval", "step", dict(kind="deepfm", tile=0)),
               ("graph-mlp-eval", "hidden", {}), ("graph-nfm-eval", "fm", dict(kind="nfm")),
               ("graph-autoint-eval", "fm", dict(kind="autoint")), ("graph-mmoe-eval", "mtl", {})]


@pytest.mark.parametrize("route", EVAL_ROUTES, ids=ids(EVAL_ROUTES))
def test_evaluation_of_saturated_rows(route):
    """evaluate(want_preds=True) on a bound split of 24 rows of the same classes: k_tower's and k_graph_head's inference
    branch -- p == 1.0f, p below 1e-7, the two outermost AUC bins that are reached (499, 1), the clipped loss."""
    case = Case(route[1], inference=True, **route[2])
    eng, prob = case.eng, case.prob
    idx, z = sat.pick_eval(prob, case.cols, sat.MIXED)
    cols = {k: np.ascontiguousarray(v[idx]) for k, v in case.cols.items()}
    eng.bind_domain_data(case.d, "val", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    loss, auc, hist, preds = eng.evaluate(case.d, "val", want_preds=True)
    want_loss, want, z2 = prob.evaluate(cols, eng.eval_batch)
    assert np.array_equal(z, z2)
    cls = sat.classify(z)
    normal = cls == "N"
    ulps = int(sat.ulp_distance(preds[normal], want[normal]).max())
    print("SATURATION_ULPS %s %s max ulp distance of p over the normal rows: %d" % (route[0], case.head, ulps))
    np.testing.assert_allclose(preds[~normal], want[~normal], rtol=0, atol=2e-7)
    np.testing.assert_allclose(preds[normal], want[normal], rtol=2e-5, atol=2e-7)
    assert np.all(preds[cls == "XH"] == F32(1.0)) and np.all(preds[cls == "H"] == F32(1.0))
    assert np.all(preds[cls == "XL"] < 1e-7) and np.all(preds[cls == "XL"] >= 0)       # 0 or a denormal: no bits compared
    assert np.all(preds[cls == "L"] < 1e-7) and np.all(preds[cls == "L"] > 0)
    # AUC bins: the number of thresholds strictly below p, exact against the oracle's predictions
    thr = oauc.thresholds(500)
    bins = np.sum(thr[None, :] < want[:, None], axis=1)
    assert np.all(bins[cls == "XH"] == 499) and np.all(bins[cls == "XL"] == 1)
    want_hist = np.zeros((2, 501), np.int64)
    np.add.at(want_hist, ((cols["label"] != 0).astype(int), bins), 1)
    assert np.array_equal(hist, want_hist) and int(hist.sum()) == B
    tp, fp, tn, fn = oauc.confusion_counts(cols["label"], want, thr)
    from mamdr_amd.engine import auc_from_histogram
    _, counts = auc_from_histogram(hist)
    for a, b in zip((tp, fp, tn, fn), counts):
        assert np.array_equal(a, b)
    bar = 2e-6 * max(1.0, abs(float(want_loss))) + sat.loss_slack(z, normal, ULPS[case.head])
    print("%s: loss hip %.7f oracle %.7f bar %.3g" % (route[0], loss, float(want_loss), bar))
    assert abs(loss - float(want_loss)) < bar
    assert ulps * 2 <= ULPS[case.head], (ulps, ULPS[case.head])       # the figure the loss bars rest on still holds
    case.close()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_topk_under_a_saturated_tower_is_ordered_by_logit():
    """mamdr_recommend ranks by logit, not by score: candidates whose scores all round to 1.0f come back in the oracle's
    logit order (compared on pairs whose oracle logits differ by more than 1e-4 max|logit|), every score 1.0f."""
    import test_gpu_recommend as rec
    g = rec.gen()
    uids, doms = rec.queries()
    d = int(doms[1])
    model = otower.OracleModel(rec.make_params(False), dropout=0.0, tower="mlp")
    prob = sat.Problem("tower", model, g["data"]["train"][d], d)
    sat.saturate(prob, inference=True)
    eng, _ = rec.make_engine("mlp", False, params=model.params)
    items = np.arange(g["n_item"], dtype=np.int32)
    checked = 0
    for u, dq in zip(uids, doms):
        with sat.logits_seen() as seen:
            model.predict(np.full(items.size, u, np.int32), items, np.full(items.size, dq, np.int32))
        z = seen[0].astype(np.float64)
        cand = items[(z >= sat.SAT_MIN) & (z <= sat.EXT_MAX)][:64]
        if cand.size < 8:
            continue
        got, scores = eng.recommend([u], [dq], int(cand.size), candidates=cand)
        got, scores = got[0], scores[0]
        assert sorted(got.tolist()) == sorted(cand.tolist())
        assert np.all(scores == F32(1.0))
        zo = z[got]                                     # the oracle's logits in the returned order: descending, up to the gap
        gap = 1e-4 * np.abs(z[cand]).max()
        later_max = np.maximum.accumulate(zo[::-1])[::-1]
        assert np.all(later_max[1:] - zo[:-1] <= gap), (u, zo)
        assert np.unique(np.round(zo, 3)).size > cand.size // 2        # distinct logits: the order says something
        checked += 1
    assert checked >= 3
    eng.close()
