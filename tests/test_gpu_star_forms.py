"""GPU parity of the Star family on the generic-layer engine (kind "star", MAMDR_GRAPH_STAR; csrc/graph_engine.hip):
norm none / pn / bn, dense dense / star, the auxiliary network, 1 - 4 hidden layers (model_zoo/Star/star.py:70-96).

The twin form (pn + star, no auxiliary network, [256, 128, 64]) is held to the FROZEN oracle/star.py and to the step kernels'
TowerEngine(tower="star"); every other form to tests/star_forms_ref.StarForms, whose own distance to float64 autograd is
pinned in tests/test_star_forms_ref.py.  Bars are the project's existing ones for the Star tower (tests/test_gpu_parity.py::
test_star_step_at_8192_rows, tests/test_gpu_hidden.py): one-step gradients rtol 5e-4, atol max(4e-6 max|w|, floor); loss 2e-6;
moving statistics rtol 1e-4 (atol 1e-6 mean, 1e-7 variance), steps exact; predictions rtol 5e-4, atol 5e-5; evaluation loss
1e-4; AUC-500 1e-3; the Adam-pass displacement bar of test_gpu_hidden.py.  The floors are the readback ulp of the SGD probe
(g = w0 - (w0 - g)): 2e-7 for the gamma tensors (values about one: `pn_gamma*` there, `bn_gamma` is the same kind of tensor),
6e-8 for tables and specific kernels, 3e-8 otherwise.  One synthetic problem is generated per module.
"""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import star_forms_ref as sref                       # noqa: E402
from oracle import auc as oauc                      # noqa: E402
from oracle import rng as orng                      # noqa: E402
from oracle import star as ostar                    # noqa: E402
from test_star_forms_ref import perturbed           # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H3 = (256, 128, 64)
FORMS = [("pn", "star", 64, H3), ("bn", "dense", 0, H3), ("bn", "star", 64, H3), ("pn", "dense", 64, H3),
         ("none", "star", 0, H3), ("none", "dense", 64, H3), ("pn", "star", 64, (128, 64)),
         ("pn", "star", 64, (256, 128, 64, 64)), ("pn", "star", 128, (256, 128))]
_PROBLEMS = {}


def problem(scale=0.2, batch=256):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import synthetic
    key = (scale, batch)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = synthetic.generate("taobao10", batch_size=batch, seed=11, scale=scale)
    return _PROBLEMS[key]


def bind(eng, g, p, emb_trainable):
    if not emb_trainable:
        eng.bind_table("user_emb", p["user_emb"])
        eng.bind_table("item_emb", p["item_emb"])
    for split in ("train", "val"):
        for d in range(g["n_domain"]):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])


def build(g, norm, dense, aux, hidden, emb_trainable=False, batch=256, seed=11):
    from mamdr_amd import graph_engine
    rs = np.random.RandomState(seed)
    p = perturbed(rs, g["n_user"], g["n_item"], g["n_domain"], norm, dense, aux, hidden)
    p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    eng = graph_engine.GraphEngine("star", g["n_user"], g["n_item"], g["n_domain"], batch, hidden, (), dropout=0.0,
                                   emb_trainable=emb_trainable, norm=norm, dense=dense, auxiliary_dim=aux)
    bind(eng, g, p, emb_trainable)
    model = sref.StarForms({k: v.copy() for k, v in p.items()}, norm, dense, aux, emb_trainable=emb_trainable)
    assert list(eng.segments) == list(model.names), (list(eng.segments), model.names)
    eng.set_weights(eng.pack(p))
    return eng, model, p


def floor_of(name):
    return 2e-7 if "gamma" in name else (6e-8 if name in ("user_emb", "item_emb") or name.startswith("Wd") else 3e-8)


def check_grads(eng, got, grads, params, residue_domain_row):
    want = eng.pack({**{k: np.zeros_like(v) for k, v in params.items() if k in eng.segments}, **grads}).cpu().numpy()
    for name, (off, cnt) in eng.segments.items():
        w, a = want[off:off + cnt], got[off:off + cnt]
        if name == "domain_emb" and residue_domain_row:     # constant over a single-domain batch under a norm: rounding residue
            assert np.abs(a).max() < 1e-5 and np.abs(w).max() < 1e-5
            continue
        np.testing.assert_allclose(a, w, rtol=5e-4, atol=max(4e-6 * max(np.abs(w).max(), 1e-3), floor_of(name)), err_msg=name)
        if name[:2] in ("Wd", "bd") or name in ("pn_gamma_spec", "pn_beta_spec", "aux_W", "aux_b"):
            D = eng.n_domain                        # the other domains' slices: EXACT zeros
            a2, w2 = a.reshape(D, -1), w.reshape(D, -1)
            idle = [j for j in range(D) if not w2[j].any()]
            assert len(idle) >= D - 2 and not a2[idle].any(), name


def check_state(eng, model, domain_cols=True):
    """domain_cols False: after an Adam pass from zero slots over single-domain batches the domain row itself is Adam's
    normalised rounding residue (see `displacement`), and its batch mean -- the row -- with it: the user / item columns
    are compared."""
    aux = eng.aux_state()
    if model.norm == "none":
        assert aux == {} and eng.aux is None
        return
    if model.norm == "pn":
        np.testing.assert_array_equal(aux["steps"], model.state["steps"])
    n = 384 if domain_cols else 256
    np.testing.assert_allclose(aux["mov_mean"][..., :n], model.state["mov_mean"][..., :n], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(aux["mov_var"], model.state["mov_var"], rtol=1e-4, atol=1e-7)


def fit_reference(model, grads, batch, residue_domain_row):
    """the reference is fit to judge THIS batch only where it keeps its own bar against float64 autograd (relative L2
    distance 2e-6 per tensor: tests/test_oracle_crosscheck.py::_check_grads, tests/test_star_forms_ref.py).  A relu whose
    pre-activation lies within fp32 rounding of zero can open on one side and stay shut on the other; the gradient is
    discontinuous there and a numpy-fp32 statement that lands on the wrong side is off by 1e-3 of a tensor, whatever the
    device does.  On such a batch the float64 gradient (rounded to fp32) is the reference, at the same bars."""
    from oracle import tower as otower
    names = list(model.names)
    _, g64, _, _ = sref.loss_and_grads64(model.params, names, *batch, model.norm, model.dense, model.auxiliary_dim)
    unfit = []
    for n in names:
        if n == "domain_emb" and residue_domain_row:
            continue
        a, w = np.asarray(otower.bigtable.densify(grads[n]), np.float64), np.asarray(g64[n], np.float64)
        rel = np.linalg.norm(a - w) / max(np.linalg.norm(w), 1e-30)
        if rel >= 2e-6:
            unfit.append((n, float(rel)))
    if not unfit:
        return grads
    print("reference off its own bar on this batch (a relu at its kink): %r -> float64 autograd judges" % (unfit,))
    return {n: (grads[n] if n == "domain_emb" and residue_domain_row else np.asarray(g64[n], F32)) for n in names}


def probe_steps(eng, model, cols, d, batch, steps, perm, residue_domain_row):
    """SGD probe (lr 1) of the listed steps of a pass against the reference's hand-derived gradients; the moving
    statistics move on both sides."""
    perm_t = torch.from_numpy(perm).to(eng.device)
    for step in steps:
        idx = perm[step * batch:(step + 1) * batch]
        loss, grads, _, c = model.loss_and_grads(cols["uid"][idx], cols["pid"][idx], cols["domain"][idx], cols["label"][idx])
        grads = fit_reference(model, grads, (cols["uid"][idx], cols["pid"][idx], cols["domain"][idx], cols["label"][idx]),
                              residue_domain_row)
        if model.norm != "none":
            sref.update_moving(model.state, model.norm, c["d"], c["mean"], c["var"])
        w0 = eng.get_weights()
        loss_t = torch.zeros(1, device=eng.device)
        eng.train_steps(d, perm=perm_t, first_step=step, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
        got = (w0 - eng.get_weights()).cpu().numpy()
        eng.set_weights(w0)
        print("step %d: loss hip %.7f ref %.7f" % (step, float(loss_t.cpu()[0]), float(loss)))
        assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
        check_grads(eng, got, grads, model.params, residue_domain_row)
        check_state(eng, model)


def largest(g):
    return max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])


def displacement(eng, model, w0):
    got = eng.unpack(eng.get_weights())
    for name in model.names:
        if name == "domain_emb" and model.norm != "none":
            continue        # (single-domain batches under a norm: Adam normalises its rounding-residue gradient -- not
                            # comparable, as in tests/test_gpu_parity.py's Star pass)
        a, o, s = np.asarray(got[name]).ravel(), model.params[name].ravel(), np.asarray(w0[name]).ravel()
        nrm, err = float(np.linalg.norm(o - s)), float(np.linalg.norm(a - o))
        assert err <= 3e-2 * nrm + 1e-6 * float(np.linalg.norm(s)) + 1e-7, (name, err, nrm)


def evaluate_both(eng, model, g, dv, batch=256):
    loss_g, auc_g, _, preds_g = eng.evaluate(dv, "val", want_preds=True)
    loss_o, preds = model.evaluate(g["data"]["val"][dv], batch)
    auc_o = float(oauc.auc500(g["data"]["val"][dv]["label"], preds, batch))
    np.testing.assert_allclose(preds_g, preds, rtol=5e-4, atol=5e-5)
    assert abs(loss_g - float(loss_o)) < 1e-4 * max(1.0, abs(float(loss_o))), (loss_g, float(loss_o))
    assert abs(auc_g - auc_o) <= 1e-3, (auc_g, auc_o)


# ------------------------------------------------------------------ 1. the twin of the step kernels' Star
@pytest.mark.parametrize("emb_trainable", [False, True])
def test_twin_matches_the_frozen_oracle_and_the_step_kernels(emb_trainable):
    from mamdr_amd import engine
    g = problem()
    eng, _, p = build(g, "pn", "star", 0, H3, emb_trainable)
    meta, rest = ostar.param_names(emb_trainable)
    assert tuple(eng.segments) == meta + rest
    model = ostar.OracleStar({k: v.copy() for k, v in p.items()}, emb_trainable=emb_trainable, lr=1e-3)
    model.norm, model.dense, model.auxiliary_dim = "pn", "star", 0
    model.loss_and_grads = lambda u, i, dm, y: ostar.loss_and_grads(model.params, model.state, u, i, dm, y, emb_trainable)
    step_eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 256, dropout=0.0, emb_trainable=emb_trainable,
                                  tower="star")
    bind(step_eng, g, p, emb_trainable)
    step_eng.set_weights(step_eng.pack(p))
    d = largest(g)
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=4)
    n_step = -(-n // 256)
    probe_steps(eng, model, cols, d, 256, (0, n_step - 1), perm, True)
    # the two HIP implementations on the same steps (a fresh generic-layer engine: the same history of moving statistics):
    # same bars, the step kernels' gradients as the reference
    perm_t = torch.from_numpy(perm).to(eng.device)
    eng_a, eng = eng, build(g, "pn", "star", 0, H3, emb_trainable)[0]
    # (both gradients are read through the accumulator: two SGD probes would each add the weights' readback ulp)
    for step in (0, n_step - 1):
        acc_s, acc_g = step_eng.new_vector(), eng.new_vector()
        step_eng.bind_accumulator(acc_s)
        eng.bind_accumulator(acc_g)
        step_eng.train_steps(d, perm=perm_t, first_step=step, n_steps=1, optimizer="accumulate")
        eng.train_steps(d, perm=perm_t, first_step=step, n_steps=1, optimizer="accumulate")
        check_grads(eng, acc_g.cpu().numpy(), step_eng.unpack(acc_s), p, True)
    a, b = eng.aux_state(), step_eng.aux_state()
    np.testing.assert_array_equal(a["steps"], b["steps"])
    np.testing.assert_allclose(a["mov_mean"], b["mov_mean"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(a["mov_var"], b["mov_var"], rtol=1e-4, atol=1e-7)
    eng.close()
    eng = eng_a
    # an Adam pass, then evaluation on the pass's domain and on another one
    w0 = eng.unpack(eng.get_weights())
    n_steps = eng.train_steps(d, perm=perm_t, lr=1e-3)
    assert n_steps >= 20
    model.train_pass(cols, perm, 256)
    displacement(eng, model, w0)
    check_state(eng, model, domain_cols=False)
    for dv in (d, (d + 1) % 10):
        evaluate_both(eng, model, g, dv)
    step_eng.close()
    eng.close()


# ------------------------------------------------------------------ 2. every form, one-step gradients of every tensor
@pytest.mark.parametrize("norm,dense,aux,hidden,emb_trainable",
                         [f + (False,) for f in FORMS] + [f + (True,) for f in FORMS[:2]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forms_one_step_gradients(norm, dense, aux, hidden, emb_trainable):
    g = problem()
    eng, model, _ = build(g, norm, dense, aux, hidden, emb_trainable)
    d = largest(g)
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=4)
    probe_steps(eng, model, cols, d, 256, (0, -(-n // 256) - 1), perm, norm != "none")
    eng.close()


@pytest.mark.parametrize("emb_trainable", [False, True])
def test_pn_star_aux_at_8192_rows(emb_trainable):
    g = problem(scale=1.0, batch=8192)
    eng, model, _ = build(g, "pn", "star", 64, H3, emb_trainable, batch=8192)
    d = largest(g)
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    assert n > 8192
    perm = orng.shuffle_perm(n, 10000, seed=4)
    probe_steps(eng, model, cols, d, 8192, (0, -(-n // 8192) - 1), perm, True)
    eng.close()


# ------------------------------------------------------------------ 3. the first row's domain serves the whole batch
@pytest.mark.parametrize("norm,dense,aux", [("pn", "star", 64), ("bn", "dense", 0)])
def test_first_row_rule_on_a_mixed_batch(norm, dense, aux):
    g = problem()
    eng, model, _ = build(g, norm, dense, aux, H3)
    d = largest(g)
    cols = {k: v.copy() for k, v in g["data"]["train"][d].items()}
    cols["domain"] = ((np.arange(cols["domain"].shape[0]) * 7 + 2) % g["n_domain"]).astype(np.int32)
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    n = cols["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=9)
    assert len(set(cols["domain"][perm[:256]].tolist())) > 3
    probe_steps(eng, model, cols, d, 256, (0, 3), perm, False)         # the domain rows carry real gradients here
    if norm == "pn":        # the moving statistics of the first rows' domains moved, nobody else's
        moved = {int(cols["domain"][perm[0]]), int(cols["domain"][perm[3 * 256]])}
        steps = eng.aux_state()["steps"]
        assert {j for j in range(g["n_domain"]) if steps[j] > 0} == moved
    eng.close()


# ------------------------------------------------------------------ 4. Adam pass, idle slices, evaluation on the moving statistics
@pytest.mark.parametrize("norm,dense,aux,hidden", FORMS[:3], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forms_adam_pass_and_evaluation(norm, dense, aux, hidden):
    g = problem()
    eng, model, p = build(g, norm, dense, aux, hidden)
    d = largest(g)
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=5)
    # seeded slots: the idle domains' slices must DECAY (zero gradient, still the Adam step), not freeze
    rs = np.random.RandomState(3)
    m0 = {k: (rs.standard_normal(v.shape) * 1e-3).astype(F32) for k, v in p.items() if k in eng.segments}
    v0 = {k: rs.uniform(1e-7, 1e-5, v.shape).astype(F32) for k, v in p.items() if k in eng.segments}
    eng.adam_m.copy_(eng.pack(m0))
    eng.adam_v.copy_(eng.pack(v0))
    for k in model.names:
        model.opt.m[k][...], model.opt.v[k][...] = m0[k], v0[k]
    w0 = eng.unpack(eng.get_weights())
    n_steps = eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), lr=1e-3)
    assert n_steps >= 20
    model.train_pass(cols, perm, 256)
    displacement(eng, model, w0)
    got = eng.unpack(eng.get_weights())
    for name in ("Wd0", "aux_W", "pn_gamma_spec"):
        if name in got:
            idle = (d + 1) % g["n_domain"]
            a = got[name].reshape(p[name].shape)[idle]
            assert np.any(a != p[name][idle]), name
            # (no data reaches an idle slice: both sides run the same fp32 Adam statements on it; what may differ is the
            # rounding of sqrt / division in a step of ~lr -- far below two ulps of the weight over the pass)
            np.testing.assert_allclose(a, model.params[name][idle], rtol=0, atol=2e-7 * max(1.0, np.abs(a).max()), err_msg=name)
    check_state(eng, model)
    for dv in (d, (d + 1) % 10):        # (the other domain: pn's initial moving statistics, bn's trained pair)
        evaluate_both(eng, model, g, dv)
    eng.close()


# ------------------------------------------------------------------ 5. the meta passes' accumulate mode
@pytest.mark.parametrize("norm,dense,aux", [("pn", "star", 64), ("bn", "dense", 0)])
def test_accumulate_equals_the_probe_and_moves_only_the_statistics(norm, dense, aux):
    g = problem()
    eng, model, _ = build(g, norm, dense, aux, H3)
    d = largest(g)
    cols = g["data"]["train"][d]
    perm = orng.shuffle_perm(cols["uid"].shape[0], 10000, seed=6)
    perm_t = torch.from_numpy(perm).to(eng.device)
    w0 = eng.get_weights()
    acc = eng.new_vector()
    eng.bind_accumulator(acc)
    eng.train_steps(d, perm=perm_t, first_step=0, n_steps=2, optimizer="accumulate")
    assert torch.equal(eng.get_weights(), w0)
    want = np.zeros(sum(model.params[k].size for k in model.names), F32)
    for s in range(2):
        idx = perm[s * 256:(s + 1) * 256]
        model.accumulate_on_batch(want, cols["uid"][idx], cols["pid"][idx], cols["domain"][idx], cols["label"][idx])
    grads, off = {}, 0
    for k in model.names:
        grads[k] = want[off:off + model.params[k].size]
        off += model.params[k].size
    check_grads(eng, acc.cpu().numpy(), grads, model.params, True)
    check_state(eng, model)                 # the layer ran in training mode: the statistics DID move
    assert eng.aux_state()["mov_mean"].any()
    eng.close()


# ------------------------------------------------------------------ 6. determinism
def test_two_engines_take_identical_steps():
    g = problem()
    d = largest(g)
    n = g["data"]["train"][d]["uid"].shape[0]
    perm = orng.shuffle_perm(n, 10000, seed=8)
    out = []
    for _ in range(2):
        eng, _, _ = build(g, "pn", "star", 64, H3, emb_trainable=True)
        eng.train_steps(d, perm=torch.from_numpy(perm).to(eng.device), first_step=0, n_steps=20, lr=1e-3)
        out.append((eng.get_weights().cpu().numpy().tobytes(), eng.aux.cpu().numpy().tobytes()))
        eng.close()
    assert out[0] == out[1]


# ------------------------------------------------------------------ 7. state errors
def test_step_before_bind_aux_is_a_state_error():
    from mamdr_amd import _lib as L
    g = problem()
    eng, _, _ = build(g, "bn", "dense", 0, H3)
    assert int(eng.lib.mamdr_graph_aux_count(eng.ctx)) == 2 * 384
    # an argument check on the host side of the ABI: a second context whose aux was never bound
    import ctypes as C
    cfg = L.GraphConfig(L.ABI_VERSION, L.GRAPH_STAR, g["n_user"], g["n_item"], g["n_domain"], 128, 256, 0, 3,
                        (C.c_int32 * 4)(256, 128, 64, 0), 0, (C.c_int32 * 4)(), 0, (C.c_int32 * 4)(), 0, 0, 0, 0.0, 0.0, 0.9, 0.999,
                        1e-8, 0.0, 0, L.STAR_NORMS["bn"], L.STAR_DENSES["dense"], 0)
    h = C.c_void_p()
    L.check(eng.lib.mamdr_graph_create(C.byref(cfg), C.c_void_p(eng.stream.cuda_stream), C.byref(h)), graph=True)
    from mamdr_amd.engine import _ptr
    w, m, v = eng.new_vector(), eng.new_vector(), eng.new_vector()
    L.check(eng.lib.mamdr_graph_bind_state(h, _ptr(w), _ptr(m), _ptr(v)), graph=True)
    for name in ("user_emb", "item_emb"):
        L.check(eng.lib.mamdr_graph_bind_table(h, {"user_emb": L.SEG_USER_EMB, "item_emb": L.SEG_ITEM_EMB}[name],
                                               _ptr(eng.tables[name]), eng.tables[name].shape[0]), graph=True)
    c = eng.data[(0, "train")]
    L.check(eng.lib.mamdr_graph_bind_domain_data(h, 0, L.SPLIT_TRAIN, _ptr(c["uid"]), _ptr(c["pid"]), _ptr(c["domain"]),
                                                 _ptr(c["label"]), c["uid"].shape[0]), graph=True)
    before = int(eng.lib.mamdr_graph_launch_count())
    with pytest.raises(L.MamdrError) as ei:
        L.check(eng.lib.mamdr_graph_train_steps(h, 0, _ptr(None), 0, 1, 256, 1024, L.OPT_ADAM, 1e-3, _ptr(None)), graph=True)
    assert ei.value.code == L.ESTATE and int(eng.lib.mamdr_graph_launch_count()) == before
    aux = torch.zeros(2 * 384, device=eng.device)
    aux[384:] = 1.0
    L.check(eng.lib.mamdr_graph_bind_aux(h, _ptr(aux)), graph=True)
    L.check(eng.lib.mamdr_graph_train_steps(h, 0, _ptr(None), 0, 1, 256, 1024, L.OPT_ADAM, 1e-3, _ptr(None)), graph=True)
    torch.cuda.synchronize()
    assert aux[:384].abs().sum().item() > 0
    eng.lib.mamdr_graph_destroy(h)
    eng.close()


# ------------------------------------------------------------------ 8. run.py's entry
@pytest.mark.parametrize("name", ["star", "star_meta_mamdr"])
def test_run_config_with_the_auxiliary_network(tmp_path, name):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import cli, graph_engine
    with open(os.path.join(ROOT, "config", "Taobao-10", "star_aux", "star_taobao.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    assert cfg["model"]["auxiliary_net"] is True and cfg["train"]["meta_parms"] == ["emb", "kernel_shared", "bias_shared"]
    cfg["model"].update(name=name)
    cfg["train"].update(epoch=3, patience=1, sample_num=2, meta_learning_rate=0.5,
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic="taobao10", synthetic_scale=0.1)
    built = []
    avg_loss, avg_auc, domain_loss, domain_auc = cli.main(cfg, on_model=built.append)
    eng = built[0].model
    assert isinstance(eng, graph_engine.GraphEngine) and eng.kind == "star" and eng.auxiliary_dim == 64
    if name != "star":      # theta / phi = the Star filter's prefix; aux_W trains outside of it
        assert eng.meta_off == 0 and not eng.meta_holes
        assert eng.n_meta == eng.segments["bs2"][0] + eng.segments["bs2"][1]
        assert eng.segments["aux_W"][0] >= eng.n_meta
    assert len(domain_auc) == 10 and np.isfinite(avg_loss)
    assert avg_auc > 0.6, (name, avg_auc)
