"""GPU parity of the mlp / wdl / deepfm towers at an embedding width OTHER than the reference configs' 128
(model_zoo/DeepCTR/deepctr.py:95-102 hands user_dim / item_dim / domain_dim to SparseFeat(embedding_dim=...) and the
DNN takes whatever 3 * dim it gets).  The step kernels are built for 128; every other accepted width (multiples of 32
from 32 to 256) runs on the generic-layer engine (kinds MAMDR_GRAPH_MLP / _WDL / _DEEPFM) against oracle/tower.py,
which is width-agnostic.  Bars are tests/test_gpu_hidden.py's, unchanged: loss 2e-6, one-step gradients rtol 2e-4
with that file's atol, an Adam pass of 20+ steps within its rounding-level displacement bar, evaluation loss / AUC-500
and the integer histogram, and the registry's routing through run.py.
"""
import copy
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import auc as oauc          # noqa: E402
from oracle import rng as orng          # noqa: E402
from oracle import tower as otower      # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [32, 64, 256]
KINDS = ["mlp", "wdl", "deepfm"]


def make_problem(kind, emb_dim, hidden, batch=256, dropout=0.5, scale=0.05, seed=7, emb_trainable=False):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import graph_engine, synthetic
    g = synthetic.generate("taobao10", batch_size=batch, seed=seed, scale=scale, emb_dim=emb_dim)
    D = g["n_domain"]
    rs = np.random.RandomState(seed)
    params = otower.init_params(rs, g["n_user"], g["n_item"], D, emb_dim=emb_dim, hidden=hidden)
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    assert params["user_emb"].shape[1] == emb_dim
    params["domain_emb"] = (rs.standard_normal(params["domain_emb"].shape) * 0.05).astype(F32)
    for n in ["b%d" % l for l in range(len(hidden))] + ["lin_domain", "lin_user", "lin_item"]:
        params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    params["gb"] = np.array([0.1], F32)
    if not emb_trainable:           # frozen linear tables stay at their zero initialisation (deepctr: same feature column)
        params["lin_user"][...] = 0
        params["lin_item"][...] = 0
    eng = graph_engine.GraphEngine(kind, g["n_user"], g["n_item"], D, batch, hidden, (), dropout=dropout,
                                   emb_trainable=emb_trainable, emb_dim=emb_dim)
    if not emb_trainable:
        eng.bind_table("user_emb", params["user_emb"])
        eng.bind_table("item_emb", params["item_emb"])
    for split in ("train", "val"):
        for d in range(D):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
    model = otower.OracleModel({k: v.copy() for k, v in params.items()}, emb_trainable=emb_trainable, dropout=dropout, lr=1e-3,
                               hidden=hidden, dropout_seed=eng.dropout_seed, tower=kind)
    # the flat layout IS the oracle's at that width (Keras trainable_weights order)
    assert list(eng.segments) == list(model.names), (list(eng.segments), model.names)
    for name in model.names:
        assert eng.segments[name][1] == model.params[name].size, (name, eng.shapes[name], model.params[name].shape)
    eng.set_weights(eng.pack(params))
    return g, eng, model


def largest_domain(g):
    return max(range(10), key=lambda k: g["data"]["train"][k]["uid"].shape[0])


def pass_sha256(kind, emb_trainable):
    """sha256 of the flat vector after one Adam pass (dropout on, 20+ steps) over the largest domain at E = 128,
    hidden [128, 64]: the generic engine's path as it was before it learnt other widths."""
    g, eng, _ = make_problem(kind, 128, (128, 64), scale=0.2, emb_trainable=emb_trainable)
    d = largest_domain(g)
    n = g["data"]["train"][d]["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=5)
    n_steps = eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=1e-3)
    assert n_steps >= 20
    digest = hashlib.sha256(eng.get_weights().cpu().numpy().tobytes()).hexdigest()
    eng.close()
    return digest


def assert_one_step(eng, model, cols, d, perm, batch, steps, emb_trainable, hidden):
    """SGD steps with lr 1 read back as gradients (tests/test_gpu_hidden.py's check and bars)."""
    perm_t = torch.from_numpy(perm).to(eng.device)
    for step in steps:
        idx = perm[step * batch:(step + 1) * batch]
        model.step = step
        masks = otower.train_masks(model.seed, model.step, len(idx), hidden, 0.5)
        loss, grads, _ = otower.loss_and_grads(model.params, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx],
                                               cols["label"][idx], masks, 0.5, emb_trainable, model.frozen_sumsq(), model.deepfm)
        loss_t = torch.zeros(1, device=eng.device)
        w0 = eng.get_weights()
        eng.set_counters(0, step)           # the dropout stream's position = the step's index in the pass
        eng.train_steps(d, perm=perm_t, first_step=step, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t, batch_size=batch)
        got = eng.unpack(w0 - eng.get_weights())
        eng.set_weights(w0)
        print("step %d rows %d loss hip %.8f oracle %.8f" % (step, len(idx), float(loss_t.cpu()[0]), float(loss)))
        assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
        assert sorted(grads) == sorted(model.names)
        for name, want in grads.items():
            want = np.asarray(want.dense() if hasattr(want, "dense") else want).ravel()
            floor = 4e-8 if name in ("user_emb", "item_emb") else 1.5e-8       # read back as w0 - (w0 - g): the weights' ulp
            np.testing.assert_allclose(got[name], want, rtol=2e-4, atol=max(2e-6 * max(np.abs(want).max(), 1e-3), floor),
                                       err_msg=name)


def assert_displacement(got, want, start, names, what="weights"):
    """tests/test_gpu_hidden.py's rounding-level displacement bar of an Adam pass, tensor by tensor."""
    for name in names:
        a, o, s = np.asarray(got[name]).ravel(), np.asarray(want[name]).ravel(), np.asarray(start[name]).ravel()
        nrm = float(np.linalg.norm(o - s))
        err = float(np.linalg.norm(a - o))
        print("%s %s: err %.3e displacement %.3e" % (what, name, err, nrm))
        assert err <= 3e-2 * nrm + 1e-6 * float(np.linalg.norm(s)) + 1e-7, (what, name, err, nrm)


@pytest.mark.parametrize("hidden", [(256, 128, 64), (128, 64)], ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("emb_dim", WIDTHS)
def test_one_step_gradients_match_oracle(emb_dim, kind, hidden):
    """first-step loss and every gradient tensor, frozen tables: a full batch of mixed domain ids and the pass's short
    last one."""
    g, eng, model = make_problem(kind, emb_dim, hidden)
    d = largest_domain(g)
    cols = {k: v.copy() for k, v in g["data"]["train"][d].items()}
    cols["domain"] = (np.arange(cols["domain"].shape[0]) % 3).astype(np.int32)      # mixed domain ids in one batch
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    n = cols["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=11)
    assert_one_step(eng, model, cols, d, perm, 256, (0, -(-n // 256) - 1), False, hidden)
    eng.close()


@pytest.mark.parametrize("kind", ["mlp", "deepfm"])
@pytest.mark.parametrize("emb_dim", WIDTHS)
def test_trainable_tables_match_oracle(emb_dim, kind):
    """trainable tables: one-step table gradients with user ids that repeat inside the batch (the deterministic reduce
    sums them in batch order), then an Adam pass of 20+ steps -- every table row, touched by a batch or only moved by
    the regulariser's dense step, with both Adam slots, against OracleModel."""
    hidden = (128, 64)
    g, eng, model = make_problem(kind, emb_dim, hidden, scale=0.2, emb_trainable=True)
    d = largest_domain(g)
    cols = {k: v.copy() for k, v in g["data"]["train"][d].items()}
    n = cols["uid"].shape[0]
    users = np.unique(cols["uid"])
    cols["uid"] = users[np.arange(n) % max(1, users.shape[0] // 40)].astype(np.int32)      # ~40 occurrences per user id
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    perm = orng.shuffle_perm(n, 10000, seed=5)
    first = perm[:256]
    assert np.unique(cols["uid"][first]).shape[0] < 256 and np.unique(cols["pid"][first]).shape[0] <= 256
    assert_one_step(eng, model, cols, d, perm, 256, (0,), True, hidden)
    model.step = 0
    eng.set_counters(0, 0)
    w0 = eng.unpack(eng.get_weights())
    n_steps = eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=1e-3)
    assert n_steps == -(-n // 256) and n_steps >= 20
    model.train_pass(cols, perm, 256)
    touched = np.zeros(g["n_user"], bool)
    touched[cols["uid"]] = True
    assert touched.any() and not touched.all()          # rows the batches touch and rows only the dense step moves
    assert_displacement(eng.unpack(eng.get_weights()), model.params, w0, model.names)
    zeros = {k: np.zeros_like(v) for k, v in w0.items()}
    assert_displacement(eng.unpack(eng.adam_m), model.opt.m, zeros, model.names, "adam m")
    assert_displacement(eng.unpack(eng.adam_v), model.opt.v, zeros, model.names, "adam v")
    got_u = eng.unpack(eng.get_weights())["user_emb"].reshape(g["n_user"], emb_dim)
    for rows, what in ((touched, "touched"), (~touched, "untouched")):
        o, s, a = model.params["user_emb"][rows], w0["user_emb"].reshape(g["n_user"], emb_dim)[rows], got_u[rows]
        assert np.linalg.norm(a - o) <= 3e-2 * np.linalg.norm(o - s) + 1e-6 * np.linalg.norm(s) + 1e-7, what
    eng.close()


@pytest.mark.parametrize("emb_trainable", [False, True], ids=["frozen", "trainable"])
def test_ragged_pass_at_width_32(emb_trainable):
    """E = 32 is where a wave of the gather serves four rows: batches of 200 rows (no multiple of 64: padding rows inside
    a wave's group of rows) and a pass whose last batch is ONE row."""
    hidden, batch = (128, 64), 200
    g, eng, model = make_problem("deepfm", 32, hidden, batch=batch, scale=0.2, emb_trainable=emb_trainable)
    d = largest_domain(g)
    n = 20 * batch + 1
    cols = {k: v[:n].copy() for k, v in g["data"]["train"][d].items()}
    assert cols["uid"].shape[0] == n
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    perm = orng.shuffle_perm(n, 10000, seed=3)
    assert_one_step(eng, model, cols, d, perm, batch, (0, 20), emb_trainable, hidden)
    model.step = 0
    eng.set_counters(0, 0)
    w0 = eng.unpack(eng.get_weights())
    assert eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=1e-3) == 21
    model.train_pass(cols, perm, batch)
    assert_displacement(eng.unpack(eng.get_weights()), model.params, w0, model.names)
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("emb_dim", WIDTHS)
def test_evaluation_matches_oracle(emb_dim, kind):
    """mamdr_graph_eval_domain at equal weights: loss, predictions (d_pred_out) and the integer histogram behind AUC-500."""
    from mamdr_amd.engine import auc_from_histogram
    g, eng, model = make_problem(kind, emb_dim, (128, 64))
    for d in (1, 5):
        c = g["data"]["val"][d]
        loss, auc, hist, preds = eng.evaluate(d, "val", want_preds=True)
        loss_o, preds_o = model.evaluate(c, 256)
        print("eval d%d loss hip %.8f oracle %.8f" % (d, loss, float(loss_o)))
        np.testing.assert_allclose(preds, preds_o, rtol=2e-5, atol=2e-7)
        assert abs(loss - float(loss_o)) < 2e-6 * max(1.0, abs(float(loss_o)))
        assert abs(auc - float(oauc.auc500(c["label"], preds_o, 256))) < 1e-4
        tp, fp, tn, fn = oauc.confusion_counts(c["label"], preds, oauc.thresholds(500))
        got_auc, (tp_g, fp_g, tn_g, fn_g) = auc_from_histogram(hist)
        assert np.array_equal(tp_g, tp) and np.array_equal(fp_g, fp) and np.array_equal(tn_g, tn) and np.array_equal(fn_g, fn)
        assert got_auc == auc
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("emb_dim", WIDTHS)
def test_adam_pass_and_evaluation_match_oracle(emb_dim, kind):
    """one pass of TF1 Adam steps (dropout on, frozen tables) over the largest domain, then evaluation: the displacement of
    every tensor against the oracle's, loss and AUC-500 (tests/test_gpu_hidden.py's test at another width)."""
    g, eng, model = make_problem(kind, emb_dim, (128, 64), scale=0.2)
    d = largest_domain(g)
    c = g["data"]["train"][d]
    n = c["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=5)
    w0 = eng.unpack(eng.get_weights())
    n_steps = eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=1e-3)
    assert n_steps == -(-n // 256) and n_steps >= 20
    model.train_pass(c, perm, 256)
    assert_displacement(eng.unpack(eng.get_weights()), model.params, w0, model.names)
    for dv in (d, (d + 1) % 10):
        loss_g, auc_g = eng.evaluate(dv, "val")
        loss_o, preds = model.evaluate(g["data"]["val"][dv], 256)
        auc_o = float(oauc.auc500(g["data"]["val"][dv]["label"], preds, 256))
        assert abs(loss_g - float(loss_o)) < 1e-4 * max(1.0, abs(float(loss_o))), (loss_g, float(loss_o))
        assert abs(auc_g - auc_o) <= 1e-3, (auc_g, auc_o)
    eng.close()


# sha256 of the flat vector after pass_sha256's Adam pass, recorded from the library as it was before the generic engine
# took other widths (same synthetic data, same device generation): the 128-wide path did not move
PARENT_SHA256 = {
    ("mlp", False): "6bda93877af262d8382d2bf62a6dd7abe8238ff110a3388b792d7f78a70c5783",
    ("wdl", False): "3703c97751306bd572ac049aba8541bae97c4301d3c25fde1965bdc692bd30b7",
    ("deepfm", False): "5b5bc9cae3eb6f7487e57be0228826fe2bc89b0c5c2e5b9f0144c224748fd960",
    ("mlp", True): "4446963c58811c130bf2d46fe1c007c1967f545088fcf8aafe446c3a396f8fc1",
    ("deepfm", True): "51da132e6cfa08eb7ce6dfb71d8edc255fbda5fbc27f52209eeeae41fc09bccd",
}


@pytest.mark.parametrize("kind,emb_trainable", sorted(PARENT_SHA256), ids=lambda v: str(v))
def test_width_128_is_bit_identical_to_before(kind, emb_trainable):
    assert pass_sha256(kind, emb_trainable) == PARENT_SHA256[(kind, emb_trainable)]


@pytest.mark.parametrize("name", ["mlp_meta_mamdr_finetune", "mlp_meta_domain_negotiation"])
def test_run_config_at_width_64(tmp_path, name):
    """run.py's entry on the shipped 64-wide config (MAMDR and DN): the registry routes the tower onto the generic-layer
    engine although hidden_dim is [256, 128, 64], the dataset layer generates 64-wide tables, the wrappers run unchanged."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, graph_engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "emb64", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name)
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic_scale=0.1)
    built = []
    avg_loss, avg_auc, domain_loss, domain_auc = cli.main(cfg, on_model=built.append)
    eng = built[0].model
    assert isinstance(eng, graph_engine.GraphEngine) and eng.kind == "mlp"
    assert eng.shapes["domain_emb"] == (10, 64) and eng.shapes["W0"] == (192, 256) and eng.tables["user_emb"].shape[1] == 64
    assert len(domain_auc) == 10 and np.isfinite(avg_loss)
    assert avg_auc > 0.6, (name, avg_auc)          # the tower learns the planted signal
