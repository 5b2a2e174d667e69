"""Every step path of the library at dropout != 1/2 and l2_emb != l2_linear, against the oracles.

`dropout`, `l2_emb` and `l2_linear` cross the C ABI into every training step.  Every other GPU file runs them where distinct
quantities coincide (rate 1/2: drop rate == keep probability, scale 2 exact; l2_emb == l2_linear == 1e-5), so a kernel that
reads keep where rate belongs, or one l2 weight for the other, passes them all.  Here the rates are 0.25 and 0.75 and the
pair is (1e-5, 3e-5); tests/test_config_scalars_host.py shows on the CPU that this file's comparison
(tests/config_scalars.py) rejects each such confusion on every tensor that carries the term -- and accepts the swap at the
defaults.

Per case (tests/config_scalars.py's bars):
  a  one SGD step at lr 1 on the pass's full first batch and on its partial last one: every gradient and the training loss
     against the oracle; tensors off the path bit-unchanged
  b  one Adam step from zero slots at step count 0, both slots read through the accessor that brings lagging table rows up
     to date: m against (1 - beta1) g, v against (1 - beta2) g^2, every element -- table rows the batch never touched
     included, whose whole gradient is the regulariser (the only place the regulariser inside the Adam-path table kernels
     meets the oracle: Adam's normalised weight update hides its size)
  c  one accumulate step: the accumulator is the oracle's dropout-free gradient whatever the rate, weights and slots keep
     their bits, the dropout counter advances by one
  d  evaluate on the val split: the loss carries both regularisers, predictions within rtol 2e-5

Each case names the path it is meant to reach and asserts what the library lets a caller observe of it: the step path
(`step_kernel_names`), the tower tile (`tower_tile`), lazy rows against the dense sweep (`mamdr_table_flushes`), the
generic-layer engine's launches per step (`mamdr_graph_launch_count`), different bits under the other tile plan.
MAMDR_NO_TAILFUSE has no query: the case asserts that the library's switch table knows the name it sets.
Every switch is read at context creation, set for the one constructor call and removed afterwards.
"""
import contextlib
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import config_scalars as cs             # noqa: E402

F32 = np.float32
DURATIONS = []


@pytest.fixture(scope="module", autouse=True)
def _print_durations():
    yield
    for what, secs in DURATIONS:
        print("CONFIG_SCALARS %-60s %6.2f s" % (what, secs))
    print("CONFIG_SCALARS total %.1f s over %d case runs" % (sum(s for _, s in DURATIONS), len(DURATIONS)))


@contextlib.contextmanager
def switches(env):
    from mamdr_amd import _lib as L
    known = {row[0] for row in L.env_switches()}
    assert set(env) <= known, (sorted(env), "not in the library's switch table")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _host(x):
    return x.detach().cpu().numpy().copy()


def make_engine(P, where, env=None, tower_tile=None):
    """where "step": mamdr_create (TowerEngine); "graph": mamdr_graph_create (GraphEngine).  The oracle's tensors are the
    engine's, name for name (PNN on the step kernels keeps W0's last three rows in a segment of its own)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine, graph_engine
    g = P.g
    common = dict(dropout=P.rate, emb_trainable=P.emb_trainable, l2_emb=P.l2[0], l2_linear=P.l2[1])
    with switches(env or {}):
        if where == "step":
            eng = engine.TowerEngine(g["n_user"], g["n_item"], P.D, cs.BATCH, tower=P.kind, uncertainty_weight=P.uncertainty,
                                     tower_tile=tower_tile, **common)
        elif P.family == "mtl":
            eh, th, gh, ne, se, sp = cs.MTL_SHAPES[P.kind]
            eng = graph_engine.GraphEngine(P.kind, g["n_user"], g["n_item"], P.D, cs.BATCH, eh, th, gh, num_experts=ne,
                                           shared_expert_num=se, specific_expert_num=sp, **common)
        else:
            eng = graph_engine.GraphEngine(P.kind, g["n_user"], g["n_item"], P.D, cs.BATCH, P.hidden, (), emb_dim=P.emb_dim,
                                           uncertainty_weight=P.uncertainty, **common)
    if not P.emb_trainable:
        eng.bind_table("user_emb", P.params["user_emb"])
        eng.bind_table("item_emb", P.params["item_emb"])
    for split in ("train", "val"):
        for d in range(P.D):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
    assert sorted(set(eng.segments) - {"W0x"}) == sorted(P.names), (list(eng.segments), P.names)
    eng.set_weights(eng.pack(P.params))
    return eng


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def run_case(P, eng, what):
    """steps a - d of the module docstring on one context; -> the gradients read back from the first SGD step."""
    t_start = time.perf_counter()
    dev = eng.device
    perm_t = torch.from_numpy(P.perm).to(dev)
    w0 = eng.get_weights().clone()
    p0 = eng.unpack(w0)
    floors = {n: cs.ulp_floor(p0[n]) for n in P.names}
    first = None
    # a. one SGD step at lr 1: a full batch, the pass's partial last batch
    for step in (0, P.n_step - 1):
        loss, want = P.grads(step, step)
        eng.set_counters(0, step)
        loss_t = torch.zeros(1, device=dev)
        eng.train_steps(P.d, perm=perm_t, first_step=step, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
        after = eng.get_weights().clone()
        got = eng.unpack(w0 - after)
        p1 = eng.unpack(after)
        eng.set_weights(w0)
        assert eng.counters()[1] == step + 1
        cs.assert_matches({n: got[n] for n in want}, want, float(loss_t.cpu()[0]), loss, floors, "%s SGD step %d" % (what, step))
        for n in P.names:
            if n not in want:           # off the path of this task's model
                assert same_bits(p1[n], p0[n]), (what, n)
        first = first or got
    # b. one Adam step from zero slots at step count 0, at a dropout position of its own
    ds = 5
    _, want = P.grads(0, ds)
    eng.set_counters(0, ds)
    eng.set_weights(w0)
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.train_steps(P.d, perm=perm_t, first_step=0, n_steps=1, lr=1e-3)
    m, v = eng.unpack(eng.adam_m), eng.unpack(eng.adam_v)
    torch.cuda.synchronize(dev)
    cs.assert_slots(m, v, want, what="%s Adam" % what)
    for n in P.names:
        if n not in want:
            assert not m[n].any() and not v[n].any(), (what, n)
    assert eng.counters() == (1, ds + 1)
    # c. one accumulate step: learning phase 0 whatever the rate
    ds = 9
    eng.set_counters(3, ds)
    eng.set_weights(w0)
    acc = eng.new_vector()
    eng.bind_accumulator(acc)
    m0, v0 = eng.adam_m.clone(), eng.adam_v.clone()
    eng.train_steps(P.d, perm=perm_t, first_step=0, n_steps=1, optimizer="accumulate")
    _, want = P.grads(0, ds, train=False)
    got = eng.unpack(acc)
    rep = cs.Report({n: got[n] for n in want}, want, 0.0, 0.0)
    assert rep.ok(), ("%s accumulate" % what, rep)
    for n in P.names:
        if n not in want:
            assert not got[n].any(), (what, n)
    assert eng.counters() == (3, ds + 1)            # (the dropout counter advances although no mask is drawn)
    assert torch.equal(eng.weights, w0) and torch.equal(eng.adam_m, m0) and torch.equal(eng.adam_v, v0)
    # d. evaluation: both regularisers in the loss
    val = P.g["data"]["val"][P.d]
    loss_g, _, _, preds = eng.evaluate(P.d, "val", want_preds=True)
    loss_o, preds_o = P.model.evaluate(P.d, val, eng.eval_batch) if P.family == "mtl" else P.model.evaluate(val, eng.eval_batch)
    print("%s eval loss got %.8f want %.8f" % (what, loss_g, float(loss_o)))
    assert cs.loss_excess(loss_g, loss_o) <= 1.0, (what, loss_g, float(loss_o))
    np.testing.assert_allclose(preds, preds_o, rtol=2e-5, atol=2e-7, err_msg=what)
    DURATIONS.append((what, time.perf_counter() - t_start))
    return first


# ---------------------------------------------------------------- step engine
STEP_CASES = [
    # id, kind, trainable, uncertainty, environment, tower tile, rates
    ("mlp frozen k_wgrad_adam", "mlp", False, False, {}, None, cs.RATES),
    ("mlp frozen k_update", "mlp", False, False, {"MAMDR_FUSED": "0"}, None, cs.RATES),
    ("mlp frozen tile 4", "mlp", False, False, {}, 4, cs.RATES),
    ("mlp frozen tile 16", "mlp", False, False, {}, 16, cs.RATES),
    ("mlp trainable lazy", "mlp", True, False, {}, None, (0.75,)),
    ("mlp trainable dense sweep", "mlp", True, False, {"MAMDR_DENSE_ADAM": "1"}, None, (0.25,)),
    ("mlp trainable separate tails", "mlp", True, False, {"MAMDR_NO_TAILFUSE": "1"}, None, (0.25,)),
    ("deepfm trainable lazy", "deepfm", True, False, {}, None, (0.25,)),
    ("deepfm trainable dense sweep", "deepfm", True, False, {"MAMDR_DENSE_ADAM": "1"}, None, (0.75,)),
    ("deepfm frozen", "deepfm", False, False, {}, None, (0.75,)),
    ("wdl frozen", "wdl", False, False, {}, None, (0.25,)),
    ("pnn@step frozen", "pnn", False, False, {}, None, cs.RATES),
    ("nfm@step trainable", "nfm", True, False, {}, None, cs.RATES),
    ("mlp uncertainty_weight", "mlp", False, True, {}, None, (0.25,)),
]


@pytest.mark.parametrize("what,kind,trainable,uncertainty,env,tile,rate",
                         [c[:6] + (r,) for c in STEP_CASES for r in c[6]], ids=lambda v: str(v) if not isinstance(v, dict) else "env")
def test_step_engine(what, kind, trainable, uncertainty, env, tile, rate):
    """the step kernels: k_tower4 / k_tower apply dropout themselves, the regularisers enter through k_wgrad_adam's pending
    domain-table step and loss, k_update, the table kernels (lazy replay, dense sweep, fused and separate tails) and, for the
    towers with linear tables, two_l2_lin / reg_terms."""
    from mamdr_amd import _lib as L
    P = cs.Problem(kind, trainable, rate=rate, uncertainty=uncertainty)
    eng = make_engine(P, "step", env, tile)
    # (k_wgrad_adam serves the plain mlp tower over frozen tables; everything else steps through k_wgrad + k_update)
    fused = kind == "mlp" and not trainable and not uncertainty and env.get("MAMDR_FUSED") != "0"
    assert eng.step_kernel_names(cs.BATCH)[L.KERNEL_WGRAD] == ("k_wgrad_adam" if fused else "k_wgrad"), what
    assert eng.tower_tile(cs.BATCH) == (tile or 4), what          # (16 rows: k_tower; 4: k_tower4 and its FM instances)
    run_case(P, eng, "step %s rate %.2f" % (what, rate))
    if trainable:       # read after the Adam step of (b): the lazy path replayed lagging rows, the dense sweep never has to
        flushes = int(eng.lib.mamdr_table_flushes(eng.ctx, 0))
        assert (flushes > 0) == ("MAMDR_DENSE_ADAM" not in env), (what, flushes)
    eng.close()


# ---------------------------------------------------------------- generic-layer engine
@pytest.mark.parametrize("rate", cs.RATES)
def test_graph_mlp_width_64_under_both_tile_plans(rate):
    """mlp (128, 64) at width 64: the default plan runs 32 x 32 tiles at this batch, MAMDR_GRAPH_TILE32_BELOW=0 the 64 x 64
    ones -- each GEMM has its own dropout epilogue.  Both meet the oracle; their bits differ (another summation order),
    which is what shows that the switch changed the plan."""
    got = []
    for env in ({}, {"MAMDR_GRAPH_TILE32_BELOW": "0"}):
        P = cs.Problem("mlp", False, rate=rate, emb_dim=64, hidden=(128, 64))
        eng = make_engine(P, "graph", env)
        got.append(run_case(P, eng, "graph mlp w64 %s rate %.2f" % ("tile64" if env else "default plan", rate)))
        eng.close()
    assert not all(same_bits(got[0][n], got[1][n]) for n in ("W0", "W1"))


@pytest.mark.parametrize("env,rate", [({}, 0.25), ({"MAMDR_GRAPH_NO_DEFER": "1"}, 0.75)], ids=["tail job", "own launch"])
def test_graph_nfm_trainable_both_linear_domain_routes(env, rate):
    """NFM with trainable tables: the linear domain table's gradient (+ 2 l2_linear w) rides in the step's tail launch, or --
    MAMDR_GRAPH_NO_DEFER=1 -- takes a launch of its own behind the backward pass.  The route shows in the launches one
    step makes: the undeferred step launches every weight gradient and this one by themselves."""
    counts = {}
    for e in ({}, {"MAMDR_GRAPH_NO_DEFER": "1"}):
        P = cs.Problem("nfm", True, rate=rate)
        eng = make_engine(P, "graph", e)
        w0 = eng.get_weights().clone()
        before = int(eng.lib.mamdr_graph_launch_count())
        eng.train_steps(P.d, perm=torch.from_numpy(P.perm).to(eng.device), first_step=0, n_steps=1, lr=1.0, optimizer="sgd")
        counts[bool(e)] = int(eng.lib.mamdr_graph_launch_count()) - before
        eng.set_weights(w0)
        if e == env:
            run_case(P, eng, "graph nfm trainable %s rate %.2f" % ("own launch" if e else "tail job", rate))
        eng.close()
    assert counts[True] > counts[False], counts


GRAPH_CASES = [("deepfm", True, 32, (0.75,)), ("pnn", False, 128, (0.75,)), ("ccpm", False, 128, (0.25,)),
               ("autoint", False, 128, cs.RATES), ("shared_bottom", True, 128, (0.25,)), ("mmoe", False, 128, cs.RATES),
               ("ple", False, 128, cs.RATES)]


@pytest.mark.parametrize("kind,trainable,emb_dim,rate", [c[:3] + (r,) for c in GRAPH_CASES for r in c[3]])
def test_graph_engine(kind, trainable, emb_dim, rate):
    """deepfm with trainable tables at width 32, PNN, CCPM, AutoInt (the attention columns of the head follow no dropout:
    they must not be scaled), and the multi-task kinds (shared_bottom with trainable tables; the gated ones' gate backward
    scales by the keep scale at two sites)."""
    from mamdr_amd import graph_engine
    P = cs.Problem(kind, trainable, rate=rate, emb_dim=emb_dim)
    eng = make_engine(P, "graph")
    assert type(eng) is graph_engine.GraphEngine and eng.kind == kind
    run_case(P, eng, "graph %s%s rate %.2f" % (kind, " trainable" if trainable else "", rate))
    eng.close()


# ---------------------------------------------------------------- Star: no dropout, no regulariser, whatever the config says
def _star_run(make, dropout, l2):
    eng, d, perm_t = make(dropout, l2)
    eng.train_steps(d, perm=perm_t, first_step=0, n_steps=3, lr=1e-3)
    loss, auc = eng.evaluate(d, "val")
    out = {"w": _host(eng.weights), "m": _host(eng.adam_m), "v": _host(eng.adam_v), "loss": np.array([loss], F32),
           "aux": _host(eng.aux) if eng.aux is not None else np.zeros(0, F32)}
    eng.close()
    return out


@pytest.mark.parametrize("where,trainable", [("step", True), ("step", False), ("graph", True)])
def test_star_ignores_dropout_and_regularisers(where, trainable):
    """model_zoo/Star/star.py:70-96 builds no Dropout layer and no regulariser.  A Star context created with dropout 0.75 and
    a large unequal l2 pair takes three Adam steps and one evaluation: weights, both slots, the norm layer's moving
    statistics and the loss are bit-identical to the same context created with zeros.  (The generic-layer engine zeroes
    the three at create; the step engine's Star path passes 0 at every site a Star step reaches.)"""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine, graph_engine
    from oracle import rng as orng
    from oracle import star as ostar
    from test_star_forms_ref import perturbed
    g = cs.generate("mlp", seed=11)
    rs = np.random.RandomState(11)
    if where == "step":
        p = ostar.init_params(rs, g["n_user"], g["n_item"], g["n_domain"])
        for n in ("pn_gamma_shared", "pn_gamma_spec"):
            p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
        for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
    else:
        p = perturbed(rs, g["n_user"], g["n_item"], g["n_domain"], "pn", "star", 64, cs.HIDDEN)
    p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    perm = orng.shuffle_perm(g["data"]["train"][d]["uid"].shape[0], 10000, seed=5)

    def make(dropout, l2):
        if where == "step":
            eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], cs.BATCH, dropout=dropout, emb_trainable=trainable,
                                     tower="star", l2_emb=l2[0], l2_linear=l2[1])
        else:
            eng = graph_engine.GraphEngine("star", g["n_user"], g["n_item"], g["n_domain"], cs.BATCH, cs.HIDDEN, (), dropout=dropout,
                                           emb_trainable=trainable, l2_emb=l2[0], l2_linear=l2[1], norm="pn", dense="star",
                                           auxiliary_dim=64)
        if not trainable:
            eng.bind_table("user_emb", p["user_emb"])
            eng.bind_table("item_emb", p["item_emb"])
        for split in ("train", "val"):
            c = g["data"][split][d]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])
        eng.set_weights(eng.pack(p))
        return eng, d, torch.from_numpy(perm).to(eng.device)
    t0 = time.perf_counter()
    plain = _star_run(make, 0.0, (0.0, 0.0))
    loud = _star_run(make, 0.75, (0.3, 0.7))
    assert np.abs(plain["m"]).max() > 0 and np.isfinite(plain["loss"]).all()
    for k in plain:
        assert same_bits(plain[k], loud[k]), (where, trainable, k)
    DURATIONS.append(("star %s%s" % (where, " trainable" if trainable else ""), time.perf_counter() - t0))
