"""GPU parity of the multi-task towers (shared_bottom / mmoe / ple): the generic-layer HIP
engine (csrc/graph_engine.hip through the `mamdr_graph_*` C ABI) against oracle/mtl.py -- the restatement of deepctr's
SharedBottom / MMOE / PLE under model_zoo/DeepMTLCTR/deep_mtl_ctr.py's per-domain models (parity unpinned: deepctr is not
in the reference tree; the oracle's gradients are held to float64 autograd in tests/test_oracle_crosscheck.py).

Bars: gradients of one step rtol 2e-4 (fp32 contractions in another order), loss 2e-6, untouched tensors bit-unchanged,
evaluation predictions rtol 2e-5 with exact integer AUC counts, per-domain AUC within 1e-3 after alternate training.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle_jobs                      # noqa: E402
from ensemble import Ensemble, TWIN_SEEDS      # noqa: E402
from keras_variables import MTL_SHAPES  # noqa: E402
from oracle import auc as oauc          # noqa: E402
from oracle import mtl as omtl          # noqa: E402
from oracle import rng as orng          # noqa: E402

F32 = np.float32

# (expert_hidden, tower_hidden, gate_hidden, num_experts, shared_expert_num, specific_expert_num) per kind
SHAPES = MTL_SHAPES


# the reference's own shapes: config/Taobao-10/{shared_bottom,mmoe,ple}.json (batch_size 1024, 10 domains)
CONFIG_SHAPES = {
    "shared_bottom": ((512, 256, 128), (64,), (), 0, 0, 0),
    "mmoe": ((512, 256, 128), (64,), (64,), 2, 0, 0),
    "ple": ((256,), (64,), (64,), 0, 2, 10),
}


def make_problem(kind, batch=256, dropout=0.5, scale=0.05, seed=7, n_domain=4, emb_trainable=False, shapes=None):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import graph_engine, synthetic
    eh, th, gh, ne, se, sp = (shapes or SHAPES)[kind]
    shape = dict(synthetic.SHAPES["taobao10"], n_domain=n_domain)
    g = synthetic.generate(shape, batch_size=batch, seed=seed, scale=scale)
    D = g["n_domain"]
    spec = omtl.Spec(kind, D, eh, th, gh, num_experts=ne, shared_expert_num=se, specific_expert_num=sp)
    rs = np.random.RandomState(seed)
    params = omtl.init_params(rs, spec, g["n_user"], g["n_item"])
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    for n in params:      # off the special initial values (zero biases, tiny domain table)
        if "/b" in n or n.endswith("/gb") or n == "domain_emb":
            params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    eng = graph_engine.GraphEngine(kind, g["n_user"], g["n_item"], D, batch, eh, th, gh, num_experts=ne,
                                   shared_expert_num=se, specific_expert_num=sp, dropout=dropout, emb_trainable=emb_trainable)
    if not emb_trainable:
        eng.bind_table("user_emb", params["user_emb"])
        eng.bind_table("item_emb", params["item_emb"])
    for split in ("train", "val", "test"):
        for d in range(D):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
    plan = spec.tensors(emb_trainable, g["n_user"], g["n_item"])
    assert list(eng.segments) == [n for n, _ in plan]     # same tensors, same order as the oracle's flat vector
    for n, shp in plan:
        assert eng.segments[n][1] == int(np.prod(shp)), n
    eng.set_weights(eng.pack(params))
    model = omtl.OracleMTL({k: v.copy() for k, v in params.items()}, spec, emb_trainable=emb_trainable, dropout=dropout,
                           lr=1e-3, dropout_seed=eng.dropout_seed)
    return g, eng, model, spec


def assert_adam_close(got, want, n_steps, lr, name, max_frac=2e-3):
    """as tests/test_gpu_parity.py: Adam normalises every update to ~lr, a relu unit within rounding of its kink may gate
    differently on the two paths; all but `max_frac` of the elements within 5 % of k * lr, none beyond 2 k lr."""
    diff = np.abs(np.asarray(got, F32).ravel() - np.asarray(want, F32).ravel())
    bound = 0.05 * n_steps * lr
    assert float(np.mean(diff > bound)) <= max_frac, (name, float(np.mean(diff > bound)), float(diff.max()))
    assert diff.max() <= 2.02 * n_steps * lr, (name, float(diff.max()))
    assert float(np.median(diff)) < 0.002 * n_steps * lr, (name, float(np.median(diff)))


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe", "ple"])
@pytest.mark.parametrize("dropout", [0.5, 0.0])
def test_one_step_gradients_match_oracle(kind, dropout):
    g, eng, model, spec = make_problem(kind, dropout=dropout)
    D = g["n_domain"]
    for d in (1, 3):
        cols = g["data"]["train"][d]
        n = cols["uid"].shape[0]
        perm = orng.shuffle_perm(n, 10000, seed=11 + d)
        perm_t = torch.from_numpy(perm).to(eng.device)
        n_step = -(-n // 256)
        for step in (0, n_step - 1):          # a full batch and the final (partial) batch
            idx = perm[step * 256:(step + 1) * 256]
            masks = omtl.train_masks(spec, model.seed, model.step, len(idx), dropout) if dropout > 0 else None
            loss, grads, _ = omtl.loss_and_grads(model.params, spec, d, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx],
                                                 cols["label"][idx], masks, dropout, False, model.frozen_sumsq())
            loss_t = torch.zeros(1, device=eng.device)
            w0 = eng.get_weights()
            eng.train_steps(d, perm=perm_t, first_step=step, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
            got = eng.unpack(w0 - eng.get_weights())
            after = eng.get_weights().cpu().numpy()
            eng.set_weights(w0)               # undo the lr = 1 step; the dropout counter advanced by 1
            model.step += 1
            assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
            for name in eng.segments:
                if name in grads:
                    want = grads[name].ravel()
                    scale = max(np.abs(want).max(), 1e-3)
                    # (the gradient is read back as w0 - (w0 - g): quantised to the weights' ulp, 7.5e-9 at |w| ~ 0.1)
                    np.testing.assert_allclose(got[name], want, rtol=2e-4, atol=max(2e-6 * scale, 1.5e-8), err_msg=name)
                else:                         # not on task d's path: untouched, bit for bit
                    off, cnt = eng.segments[name]
                    assert np.array_equal(after[off:off + cnt], w0.cpu().numpy()[off:off + cnt]), name
    eng.close()


# layer widths that are multiples of 64 but not of the 128-deep stages of the 32 x 32 tiles (their zero-filled tails), a
# three-layer gate, three experts: nothing a reference config uses, everything mamdr_graph_create accepts
ODD_SHAPES = {
    "shared_bottom": ((192, 320), (192, 64), (), 0, 0, 0),
    "mmoe": ((320, 192), (64,), (192, 64, 64), 3, 0, 0),
    "ple": ((192,), (320, 64), (64,), 0, 1, 3),
}


# 16 experts of three layers per task: 48 weight gradients + gate + tower, more than one queue of the backward pass holds
# (MAX_WQ = 40): the queue is flushed in mid-step and the optimiser step falls back to its own launch for that step
MANY_SHAPES = {"ple": ((64, 64, 64), (64,), (64,), 0, 2, 14)}


@pytest.mark.parametrize("kind,shapes,batch", [(k, sh, b) for sh, b in (("config", 1024), ("odd", 448))
                                               for k in ("shared_bottom", "mmoe", "ple")] + [("ple", "many", 256)])
def test_config_shapes_at_batch_1024(kind, shapes, batch):
    """the reference's Taobao-10 multi-task configs as configured: their layer widths / expert counts, 10 domains, batch
    size 1,024 (config/Taobao-10/*.json) -- one-step gradients of every tensor on task d's path and the loss against the
    oracle on a full batch, everything off the path bit-unchanged, then three Adam steps.  "odd": widths of 192 / 320
    (reduction lengths that end inside a 128-deep stage) at a batch of 448 rows (7 tiles of 64)."""
    g, eng, model, spec = make_problem(kind, batch=batch, dropout=0.5, scale=0.5, n_domain=10,
                                       shapes={"config": CONFIG_SHAPES, "odd": ODD_SHAPES, "many": MANY_SHAPES}[shapes])
    d = max(range(10), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    assert n >= 3 * batch
    perm = orng.shuffle_perm(n, 10000, seed=5)
    perm_t = torch.from_numpy(perm).to(eng.device)
    idx = perm[:batch]
    masks = omtl.train_masks(spec, model.seed, model.step, batch, 0.5)
    loss, grads, _ = omtl.loss_and_grads(model.params, spec, d, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx],
                                         cols["label"][idx], masks, 0.5, False, model.frozen_sumsq())
    loss_t = torch.zeros(1, device=eng.device)
    w0 = eng.get_weights()
    eng.train_steps(d, perm=perm_t, first_step=0, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
    got = eng.unpack(w0 - eng.get_weights())
    after = eng.get_weights().cpu().numpy()
    eng.set_weights(w0)
    model.step += 1
    assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
    for name in eng.segments:
        if name in grads:
            want = grads[name].ravel()
            scale = max(np.abs(want).max(), 1e-3)
            np.testing.assert_allclose(got[name], want, rtol=2e-4, atol=max(2e-6 * scale, 1.5e-8), err_msg=name)
        else:
            off, cnt = eng.segments[name]
            assert np.array_equal(after[off:off + cnt], w0.cpu().numpy()[off:off + cnt]), name
    eng.train_steps(d, perm=perm_t, first_step=0, n_steps=3, lr=1e-3)
    model.train_pass(d, cols, perm, batch, max_steps=3)
    got = eng.unpack(eng.get_weights())
    for name in grads:
        assert_adam_close(got[name], model.params[name], 3, 1e-3, name)
    eng.close()


def test_mixed_domain_ids_in_one_batch():
    """the domain table's gradient is a segment sum over the batch's domain ids: exact for any mix of ids."""
    g, eng, model, spec = make_problem("mmoe", dropout=0.5)
    d = 2
    cols = {k: v.copy() for k, v in g["data"]["train"][d].items()}
    cols["domain"] = (np.arange(cols["domain"].shape[0]) % g["n_domain"]).astype(np.int32)
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    idx = np.arange(256)
    masks = omtl.train_masks(spec, model.seed, 0, 256, 0.5)
    _, grads, _ = omtl.loss_and_grads(model.params, spec, d, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx],
                                      cols["label"][idx], masks, 0.5, False, model.frozen_sumsq())
    w0 = eng.get_weights()
    eng.train_steps(d, first_step=0, n_steps=1, lr=1.0, optimizer="sgd")
    got = eng.unpack(w0 - eng.get_weights())
    want = grads["domain_emb"].ravel()
    np.testing.assert_allclose(got["domain_emb"], want, rtol=2e-4, atol=max(2e-6 * np.abs(want).max(), 1.5e-8))
    eng.close()


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe", "ple"])
def test_adam_steps_across_domains_and_eval(kind):
    """Adam steps on two domains in turn (ONE optimizer object: shared beta powers, per-variable slots, variables off the
    path neither move nor decay), then evaluation: predictions, loss, exact AUC counts."""
    g, eng, model, spec = make_problem(kind, dropout=0.5)
    n_steps = 0
    for d in (0, 2, 0):
        cols = g["data"]["train"][d]
        perm = orng.shuffle_perm(cols["uid"].shape[0], 10000, seed=3 + d)
        k = min(3, -(-perm.shape[0] // 256))
        eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), n_steps=k, lr=1e-3)
        model.lr = 1e-3
        model.train_pass(d, cols, perm, 256, max_steps=k)
        n_steps += k
    assert int(eng.lib.mamdr_graph_optimizer_steps(eng.ctx)) == n_steps == model.t
    got = eng.unpack(eng.get_weights())
    for name in eng.segments:
        assert_adam_close(got[name], model.params[name], n_steps, 1e-3, name)
    # task 1's and task 3's own blocks never moved
    for name in eng.segments:
        if name.split("/")[0] in ("tower_1", "head_1", "gate_3", "task_3_expert_0"):
            assert np.array_equal(got[name], model.params[name].ravel()), name
    for d in (0, 3):
        cols = g["data"]["val"][d]
        loss, auc, hist, preds = eng.evaluate(d, "val", want_preds=True)
        loss_o, preds_o = model.evaluate(d, cols, 256)
        np.testing.assert_allclose(preds, preds_o, rtol=3e-3, atol=3e-5)      # weights differ by the Adam-step noise above
        assert abs(loss - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))
        # exact integer confusion counts of the HIP predictions (utils/metrics_utils.py:297-354)
        tp, fp, tn, fn = oauc.confusion_counts(cols["label"], preds, oauc.thresholds(500))
        from mamdr_amd.engine import auc_from_histogram
        got_auc, (tp_g, fp_g, tn_g, fn_g) = auc_from_histogram(hist)
        assert np.array_equal(tp_g, tp) and np.array_equal(fp_g, fp) and np.array_equal(tn_g, tn) and np.array_equal(fn_g, fn)
        assert got_auc == auc
    eng.close()


def test_eval_predictions_match_oracle_at_equal_weights():
    for kind in ("shared_bottom", "mmoe", "ple"):
        g, eng, model, spec = make_problem(kind, dropout=0.5)
        for d in (1, 2):
            cols = g["data"]["test"][d]
            loss, auc, hist, preds = eng.evaluate(d, "test", want_preds=True)
            loss_o, preds_o = model.evaluate(d, cols, 256)
            np.testing.assert_allclose(preds, preds_o, rtol=2e-5, atol=2e-7)
            assert abs(loss - float(loss_o)) < 2e-6 * max(1.0, abs(float(loss_o)))
            assert abs(auc - float(oauc.auc500(cols["label"], preds_o, 256))) < 1e-4
        eng.close()


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe", "ple"])
def test_alternate_training_auc_parity(kind):
    """DeepMTLCTR.train (deep_mtl_ctr.py:69-96): epochs of one full pass per domain through that domain's model, in a
    shuffled order; same order / shuffles / dropout masks on both sides.  After the first epoch: per-domain validation AUC
    within north_star's plain 1e-3.  After four: the summation order of the batch reductions is the kernels' own and fp32
    training amplifies such last-bit differences (mmoe: up to 1e-3 on this problem after 16 passes), so the HIP run must not
    be an outlier of an ensemble of six oracle runs whose weights differ by one rounding per pass (round 6, tests/ensemble.py;
    rounds 3 - 5 asserted 1e-3 plus twice one twin's shift)."""
    g, eng, model, spec = make_problem(kind, dropout=0.5, scale=0.15)
    D = g["n_domain"]
    sizes = [g["data"]["train"][d]["uid"].shape[0] for d in range(D)]
    order = [[2, 0, 3, 1], [1, 3, 0, 2], [0, 1, 2, 3], [3, 2, 1, 0]]
    LR = 2e-3               # (the configs' 1e-4 needs tens of epochs; the comparison wants a model that has learnt)
    def shaken(params, rs):           # every trainable tensor changed by one fp32 rounding (tests/ensemble.py)
        return {k: oracle_jobs.perturbed(v, rs, 2e-7) if v.dtype == F32 and "emb" not in k else v.copy() for k, v in params.items()}
    twins, twin_rs = [], []
    for sd in TWIN_SEEDS:
        twins.append(omtl.OracleMTL(shaken(model.params, np.random.RandomState(sd)), spec, emb_trainable=False, dropout=0.5, lr=LR,
                                    dropout_seed=eng.dropout_seed))
        twin_rs.append(np.random.RandomState(sd + 7919))
    model.lr = LR
    k = 0
    for e, seq in enumerate(order):
        for d in seq:
            k += 1
            perm = orng.shuffle_perm(sizes[d], 10000, seed=500 + k)
            eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=LR)
            model.train_pass(d, g["data"]["train"][d], perm, 256)
            for twin, rs in zip(twins, twin_rs):          # ... and again after every pass
                twin.train_pass(d, g["data"]["train"][d], perm, 256)
                for n_, v in twin.params.items():
                    if v.dtype == F32 and "emb" not in n_:
                        v[...] = oracle_jobs.perturbed(v, rs, 2e-7)
        if e == 0:      # after ONE epoch the rounding-level differences have not been amplified yet: the plain 1e-3 bar
            for d in range(D):
                _, a1 = eng.evaluate(d, "val")
                _, p1 = model.evaluate(d, g["data"]["val"][d], 256)
                o1 = float(oauc.auc500(g["data"]["val"][d]["label"], p1, 256))
                print("%s domain %d after the first epoch: AUC hip %.5f oracle %.5f" % (kind, d, a1, o1))
                assert abs(a1 - o1) <= 1e-3, (d, a1, o1)
    aucs, got, tw = [], [], [[] for _ in twins]
    for d in range(D):
        _, auc_g = eng.evaluate(d, "val")
        _, preds = model.evaluate(d, g["data"]["val"][d], 256)
        auc_o = float(oauc.auc500(g["data"]["val"][d]["label"], preds, 256))
        for j, twin in enumerate(twins):
            _, preds_t = twin.evaluate(d, g["data"]["val"][d], 256)
            tw[j].append(float(oauc.auc500(g["data"]["val"][d]["label"], preds_t, 256)))
        print("%s domain %d: AUC hip %.5f oracle %.5f (perturbed oracles %s)" % (kind, d, auc_g, auc_o, " ".join("%.5f" % t[d] for t in tw)))
        aucs.append(auc_o)
        got.append(auc_g)
    # end of training: not an outlier of the ensemble of six oracle runs (no factor on a single draw; tests/ensemble.py)
    ens = Ensemble([None] * (1 + len(twins)))
    ens.check("val", dict(enumerate(got)), [dict(enumerate(m)) for m in [aucs] + tw])
    ens.aggregate(kind)
    assert np.mean(aucs) > 0.6
    eng.close()


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe", "ple"])
@pytest.mark.parametrize("emb_trainable", [False, True])
def test_launch_plans_are_bitwise_twins(kind, emb_trainable, monkeypatch):
    """the engine's launch plans of round 4 against the plans they replaced, same seeds: the optimiser step inside the tail
    launch vs a k_graph_adam launch of its own (MAMDR_GRAPH_NO_TAIL_OPT=1) must leave identical bits (the same arithmetic per
    element); a pair of weight-gradient launches per layer (MAMDR_GRAPH_NO_DEFER=1: other splits of the batch rows) and
    64 x 64 tiles everywhere (MAMDR_GRAPH_TILE32_BELOW=0: another summation order) agree to rounding.  Adam and SGD steps
    on three domains, then accumulate-only steps (the meta passes)."""
    def run(env):
        for k in ("MAMDR_GRAPH_NO_TAIL_OPT", "MAMDR_GRAPH_NO_DEFER", "MAMDR_GRAPH_TILE32_BELOW"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g, eng, model, spec = make_problem(kind, batch=256, dropout=0.5, scale=0.1, emb_trainable=emb_trainable)
        acc = eng.new_vector()
        eng.bind_accumulator(acc)
        for d, opt, lr in ((0, "adam", 1e-3), (2, "adam", 1e-3), (1, "sgd", 0.01), (0, "adam", 1e-3)):
            n = g["data"]["train"][d]["uid"].shape[0]
            perm = torch.from_numpy(orng.shuffle_perm(n, 10000, seed=3 + d)).to(eng.device)
            eng.train_steps(d, perm=perm, first_step=0, n_steps=min(3, -(-n // 256)), lr=lr, optimizer=opt)
        n = g["data"]["train"][3]["uid"].shape[0]
        perm = torch.from_numpy(orng.shuffle_perm(n, 10000, seed=9)).to(eng.device)
        eng.train_steps(3, perm=perm, first_step=0, n_steps=2, lr=1e-3, optimizer="accumulate")
        out = (eng.get_weights().cpu().numpy().copy(), acc.cpu().numpy().copy(), eng._adam_m.cpu().numpy().copy(),
               eng._adam_v.cpu().numpy().copy())
        eng.close()
        return out

    base = run({})
    twin = run({"MAMDR_GRAPH_NO_TAIL_OPT": "1"})
    for a, b, what in zip(base, twin, ("weights", "accumulator", "adam m", "adam v")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    assert np.abs(base[1]).max() > 0
    for env in ({"MAMDR_GRAPH_NO_DEFER": "1"}, {"MAMDR_GRAPH_TILE32_BELOW": "0"}):
        other = run(env)
        from test_gpu_parity import assert_adam_close
        assert_adam_close(other[0], base[0], 11, 1e-3, str(env), max_frac=2e-3)
        # (gradients taken at weights that differ by the Adam noise above: compared in the L2 norm)
        assert np.linalg.norm(other[1] - base[1]) < 5e-2 * np.linalg.norm(base[1]), env


def test_invalid_configurations_say_so():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import _lib as L
    from mamdr_amd import graph_engine
    with pytest.raises(L.MamdrError):
        graph_engine.GraphEngine("mmoe", 100, 100, 3, 256, (100,), (64,), (64,), num_experts=2)       # width not a multiple of 64
    with pytest.raises(L.MamdrError):
        graph_engine.GraphEngine("mmoe", 100, 100, 3, 256, (128,), (64,), (), num_experts=2)          # gated tower without a gate DNN


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe"])
def test_trainable_tables_gradients_and_adam(kind):
    """the Amazon configurations of these towers train their tables (load_pretrain_emb false): scatter-add of the row
    gradients (rows repeated inside a batch summed in batch order) + the dense regulariser gradient on EVERY row, TF1's
    dense Adam over the whole tables; one SGD step at lr 1 shows every gradient, then Adam steps on two domains."""
    g, eng, model, spec = make_problem(kind, dropout=0.5, scale=0.1, emb_trainable=True)
    assert "user_emb" in eng.segments and eng.segments["user_emb"][0] == 0
    d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    cols = g["data"]["train"][d]
    perm = orng.shuffle_perm(cols["uid"].shape[0], 10000, seed=4)
    perm_t = torch.from_numpy(perm).to(eng.device)
    idx = perm[:256]
    assert len(np.unique(cols["uid"][idx])) < 256          # repeated rows exercise the ordered segment sum
    masks = omtl.train_masks(spec, model.seed, model.step, 256, 0.5)
    loss, grads, _ = omtl.loss_and_grads(model.params, spec, d, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx],
                                         cols["label"][idx], masks, 0.5, True)
    w0 = eng.get_weights()
    loss_t = torch.zeros(1, device=eng.device)
    eng.train_steps(d, perm=perm_t, first_step=0, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
    got = eng.unpack(w0 - eng.get_weights())
    eng.set_weights(w0)
    model.step += 1
    assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
    for name, want in grads.items():
        want = want.ravel()
        # (read back as w0 - (w0 - g): quantised to the weights' ulp -- 3e-8 for the largest table entries, |w| up to 0.5)
        floor = 4e-8 if name in ("user_emb", "item_emb") else 1.5e-8
        np.testing.assert_allclose(got[name], want, rtol=2e-4, atol=max(2e-6 * max(np.abs(want).max(), 1e-3), floor), err_msg=name)
    # untouched rows still move by the regulariser: g = 2 l2 w
    untouched = np.setdiff1d(np.arange(g["n_user"]), cols["uid"][idx])[:5]
    for r in untouched:
        np.testing.assert_allclose(got["user_emb"][r * 128:(r + 1) * 128], 2e-5 * model.params["user_emb"][r], rtol=1e-3, atol=2e-8)
    n_steps = 0
    for dd in (d, (d + 1) % g["n_domain"]):
        c2 = g["data"]["train"][dd]
        pm = orng.shuffle_perm(c2["uid"].shape[0], 10000, seed=9 + dd)
        k = min(3, -(-pm.shape[0] // 256))
        eng.train_steps(dd, perm=torch.from_numpy(pm).to(eng.device), n_steps=k, lr=1e-3)
        model.lr = 1e-3
        model.train_pass(dd, c2, pm, 256, max_steps=k)
        n_steps += k
    got = eng.unpack(eng.get_weights())
    for name in eng.segments:
        assert_adam_close(got[name], model.params[name], n_steps, 1e-3, name)
    loss_g, auc_g = eng.evaluate(d, "val")
    loss_o, preds = model.evaluate(d, g["data"]["val"][d], 256)
    assert abs(loss_g - float(loss_o)) < 2e-3 * max(1.0, abs(float(loss_o)))
    eng.close()


@pytest.mark.parametrize("kind", ["shared_bottom", "mmoe", "ple"])
def test_alternate_training_teacher_forced(kind):
    """the chaos-free counterpart of test_alternate_training_auc_parity (round 6, tests/teacher.py): the same four epochs of
    one full pass per domain (deep_mtl_ctr.py:69-96), but EVERY pass is run on the generic-layer engine from the ORACLE's
    state at that point -- every tensor, the Adam slots, the optimizer's step count with TF's running beta powers
    (mamdr_graph_set_counters), the dropout position -- and its per-step losses and end state are compared with the oracle's:
    no self-divergence term.  Bars as tests/test_gpu_teacher.py (k lr = steps x 2e-3): first-step loss 2e-5, any step 2e-4,
    <= 2e-3 of a tensor's elements beyond 5 % of k lr (this file's assert_adam_close), none beyond 2.02 k lr, median
    <= 0.002 k lr, slots m / v relative L2 0.1 / 5e-3; both launch paths of a pass (losses written or not) end in the same bits."""
    import teacher
    from teacher_bars import BARS
    g, eng, model, spec = make_problem(kind, dropout=0.5, scale=0.15)
    D = g["n_domain"]
    sizes = [g["data"]["train"][d]["uid"].shape[0] for d in range(D)]
    order = [[2, 0, 3, 1], [1, 3, 0, 2], [0, 1, 2, 3], [3, 2, 1, 0]]
    LR = 2e-3
    model.lr = LR
    bars = dict(BARS, frac=2e-3)
    ls = teacher.LockStep(model, model, eng, g["data"]["train"], LR, bars, chunk=1 << 20,
                          slots_of=lambda m: (m.m, m.v), t_of=lambda m: int(m.t),
                          oracle_pass=lambda d, data, perm, bs: model.train_pass(d, data, perm, bs))
    k = 0
    for seq in order:
        for d in seq:
            k += 1
            perm = orng.shuffle_perm(sizes[d], 10000, seed=500 + k)
            ls.run_pass(d, g["data"]["train"][d], perm, 256)
    out = ls.summary()
    print("%s alternate training teacher-forced: %d passes / %d steps; worst first-step loss rel %.1e, any step %.1e; weights frac "
          "%.1e max %.3f k lr median %.5f k lr; slots %.1e / %.1e" % (kind, out["passes"], out["steps"], out["loss_first"],
                                                                      out["loss_rel"], out["frac"], out["max_klr"], out["med_klr"],
                                                                      out["m_rel"], out["v_rel"]))
    for v in ls.bad[:10]:
        print("  VIOLATION", v)
    assert not ls.bad, "%d violations (first: %r)" % (len(ls.bad), ls.bad[0])
    assert out["passes"] == 16 and out["steps"] >= 40
    eng.close()


def test_environment_of_one_context_does_not_leak_into_the_next(monkeypatch):
    """MAMDR_GRAPH_TILE32_BELOW is read at EVERY mamdr_graph_create (round 6): a context created without it runs the default
    tile plan again -- the same bits as before -- although a context with MAMDR_GRAPH_TILE32_BELOW=0 (64 x 64 tiles: another
    summation order) lived in the process in between.  (It used to stay in force for the rest of the process: the end-to-end
    runs of a session that had run test_launch_plans_are_bitwise_twins differed from a fresh process's at rounding level.)"""
    def run():
        g, eng, model, spec = make_problem("mmoe", batch=256, dropout=0.5, scale=0.1)
        for d in (0, 1, 2):
            eng.train_steps(d, perm=None, first_step=0, n_steps=2, lr=1e-3)
        out = eng.get_weights().cpu().numpy().copy()
        eng.close()
        return out
    monkeypatch.delenv("MAMDR_GRAPH_TILE32_BELOW", raising=False)
    a = run()
    monkeypatch.setenv("MAMDR_GRAPH_TILE32_BELOW", "0")
    b = run()
    monkeypatch.delenv("MAMDR_GRAPH_TILE32_BELOW", raising=False)
    c = run()
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))       # (the switch does change the summation order)
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)
