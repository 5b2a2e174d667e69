"""Every step path at the domain counts D where its kernels change path, against the CPU oracle.

D is the parameter the step engine branches on most after the batch size, and the other GPU files compare with the oracle
at 2, 3, 4 and 10 domains only.  The cases (tests/domain_counts.py, named by the boundary they sit on):

  mlp, frozen tables, k_tower4 + k_wgrad_adam    D = 1, 16 | 17, 32 | 33, 48 | 49, 64 at 256 rows: both sides of every
                                                 MT = ceil(D / 16) instantiation of fz_s_contract, its LDS size, the padded
                                                 rows of S; 17 and 64 at 8 rows (4 tiles: the writer lanes' remaining-rows loop
                                                 runs up to 16 times per tile); 64 at 1,024 rows (the full grid)
  the same with tower_tile = 16                  k_tower's copy of that loop (dm_tile_writer): 17 and 64 at 8 rows (one tile
                                                 steps every other row), 64 at 256 rows (16 tiles, three trips)
  the same context under MAMDR_FUSED=0           k_update's narrow form at 8 | 9, 16 | 17, 32 | 33, 64 (its eight-domain
                                                 prefetch, the second trip of the s_l fill, s_l exactly full); its WIDE form
                                                 -- more than 8 row groups: 2,064 rows, derived from wgrad_groups' rule -- at
                                                 32 | 33 and 64 (the loop over domains 32 .. 63)
  D = 65                                         no linear dW0[256:384], plain tiles, no fused path: mlp at 256, 2,064 and 5
                                                 rows, deepfm (its S2 region)
  layout, D = 33, 34, 35 (1, 2, 3 mod 4)         deepfm frozen / trainable (k_update_lin), wdl, pnn, mlp + uncertainty
                                                 weighting: lin_domain and log_var put what follows them off 16-byte alignment
  star                                           D = 1 (no lazy slices), 2, 33, 65 (D is gridDim.y of k_star_update / _catchup)
  generic-layer engine                           shared_bottom, mmoe, ple, star pn/star/64 at D = 1 and 33: gradients only

Every case asserts the path it ran on (mamdr_step_path, tower_tile), so none can silently run another kernel.  Per case and
per batch kind -- `mixed`: every id in every batch, so every row of S and the highest row of the last one-hot block are
non-zero; `one`: all rows carry D - 1 -- with the bars of the sibling tests unchanged:
  (a) one SGD step at lr 1: the loss (2e-6) and every segment (test_gpu_parity.py::test_mixed_domain_ids_in_one_batch,
      test_deepfm_gradients_adam_eval, test_uncertainty_weighted_step_matches_oracle, test_star_step_adam_eval;
      test_gpu_fmnets.py for pnn);
  (b) one call of three Adam steps without a loss output -- the domain-table step stays pending and the tower's writer lanes
      materialise it: the weights (assert_adam_close as tests/test_gpu_edge_batches.py calls it), both counters, and both
      Adam slots of the domain table: per tensor within 3 % of its norm (tests/test_gpu_embdim.py's bar for the slots, without
      its absolute floor of 1e-7, which is the size of v here), and the rows NO batch touched row by row at rounding level
      (`check_untouched_rows`);
  (c) the evaluation of a split of domain 0 at equal weights (test_deepfm_gradients_adam_eval, test_gpu_fmnets.py,
      test_star_step_adam_eval).
Star also takes the three steps as three one-step calls (the dense sweep) and its idle slices must come out of both with
the same bits (test_gpu_parity.py::test_star_lazy_slices_equal_the_per_step_sweep); one idle slice starts from non-zero
Adam slots so that the replay has something to replay.

The oracle alone is held to float64 autograd on every first batch used here in tests/test_oracle_crosscheck.py::
test_domain_count_inputs_are_fit (no input had to be moved) and tests/test_star_forms_ref.py.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import domain_counts as dc                          # noqa: E402
import test_gpu_mtl as t_mtl                        # noqa: E402
import test_gpu_parity as t_par                     # noqa: E402
import test_gpu_star_forms as t_sf                  # noqa: E402
from oracle import auc as oauc                      # noqa: E402
from oracle import mtl as omtl                      # noqa: E402
from oracle import star as ostar                    # noqa: E402
from oracle import tower as otower                  # noqa: E402

F32 = np.float32
STAR_SLICED = ("pn_gamma_spec", "pn_beta_spec", "Wd0", "Wd1", "Wd2", "bd0", "bd1", "bd2")


def pad16(rows):
    return -(-rows // 16) * 16


def test_the_wide_batch_follows_the_row_group_rule():
    """k_update<WIDE> serves steps of more than 8 row groups; mamdr_api.hip::wgrad_groups gives 256-row groups between 1,025
    and 4,096 padded rows, so 2,048 rows are 8 groups and the next whole tile makes 9."""
    assert dc.wgrad_groups(2048) == 8 and dc.wgrad_groups(2064) == 9 and dc.WIDE == 2064
    assert [dc.wgrad_groups(r) for r in (16, 256, 512, 528, 1024, 1040)] == [1, 1, 2, 5, 8, 5]


# ---------------------------------------------------------------------------------------------- one engine per case
class Problem(object):
    def __init__(self, case):
        from mamdr_amd import engine
        self.case = case
        self.params, self.splits, self.val = dc.make_inputs(case)
        self.star = case.tower == "star"
        switches = {"MAMDR_FUSED": "0"} if case.path == "slab" else {}
        os.environ.update(switches)         # (the library reads its switches when the context is created)
        try:
            eng = engine.TowerEngine(dc.N_USER, dc.N_ITEM, case.D, case.batch, dropout=0.0 if self.star else 0.5,
                                     emb_trainable=case.trainable, tower=case.tower, uncertainty_weight=case.uncertainty,
                                     tower_tile=16 if case.path == "fused16" else None)
        finally:
            for k in switches:
                os.environ.pop(k, None)
        self.eng = eng
        if not case.trainable:
            eng.bind_table("user_emb", self.params["user_emb"])
            eng.bind_table("item_emb", self.params["item_emb"])
        vd, vc = self.val
        eng.bind_domain_data(vd, "val", vc["uid"], vc["pid"], vc["domain"], vc["label"])
        assert eng.dropout_seed == dc.DROPOUT_SEED
        assert sorted(set(eng.segments) - {"W0x"}) == sorted(dc.names_of(case)), list(eng.segments)
        eng.set_weights(eng.pack(self.params))
        self.w0 = eng.get_weights()
        self.aux0 = eng.aux.clone() if eng.aux is not None else None
        # ---- the path: no case may silently run another kernel
        rows_pad = pad16(case.batch)
        want_path = 1 if case.path in ("fused", "fused16") else 0
        want_tile = 16 if self.star or case.path == "fused16" else (4 if rows_pad <= 1024 else 16)
        assert int(eng.lib.mamdr_step_path(eng.ctx, case.batch)) == want_path, case.name
        assert eng.tower_tile(case.batch) == want_tile, (case.name, eng.tower_tile(case.batch))
        if case.path == "slab" or case.D > 64:
            assert dc.wgrad_groups(rows_pad) == (9 if case.batch == dc.WIDE else 1)

    def close(self):
        self.eng.close()

    def fresh(self):
        """engine and oracle at the start: weights, zero slots, both counters, the norm layer's statistics"""
        eng = self.eng
        eng.set_weights(self.w0)
        eng.optimizer_reset()
        eng.set_counters(0, 0)
        if self.aux0 is not None:
            eng.aux.copy_(self.aux0)
        return dc.make_model(self.case, self.params)

    def bind(self, which):
        d, cols = self.splits[which]
        self.eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
        return d, cols


_LIVE = {}


def problem_of(case):
    """one engine per case serves both batch kinds; the previous case's engine is closed."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if case.name not in _LIVE:
        for p in _LIVE.values():
            p.close()
        _LIVE.clear()
        _LIVE[case.name] = Problem(case)
    return _LIVE[case.name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for p in _LIVE.values():
        p.close()
    _LIVE.clear()


# ---------------------------------------------------------------------------------------------- the bars, by family
def floor_of(case, name):
    table = name in ("user_emb", "item_emb")
    if case.uncertainty:
        return 1e-7                             # test_uncertainty_weighted_step_matches_oracle
    if case.tower == "pnn":
        return 4e-8 if table else 1.5e-8        # tests/test_gpu_fmnets.py::test_one_step_gradients_match_oracle
    return 6e-8 if table else 1e-8              # test_mixed_domain_ids_in_one_batch, test_deepfm_gradients_adam_eval


def check_probe(P, d, args):
    """(a) one SGD step at lr 1 = the gradient of every segment, and the loss"""
    case, eng = P.case, P.eng
    model = P.fresh()
    loss, grads, c = dc.oracle_step(case, model, args)
    w0 = eng.get_weights()
    loss_t = torch.zeros(1, device=eng.device)
    eng.train_steps(d, first_step=0, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
    got = eng.unpack(w0 - eng.get_weights())
    eng.set_weights(w0)
    got_loss = float(loss_t.cpu()[0])
    print("%s: loss hip %.7f oracle %.7f" % (case.name, got_loss, float(loss)))
    assert abs(got_loss - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
    assert sorted(grads) == sorted(got), (sorted(grads), sorted(got))
    for name in got:
        a, w = got[name], np.asarray(otower.bigtable.densify(grads[name]), F32).ravel()
        if P.star:          # test_star_step_adam_eval
            if name == "domain_emb":        # constant over a one-domain batch: PartitionedNorm removes it; rounding residue
                assert np.abs(a).max() < 1e-5 and np.abs(w).max() < 1e-5
                continue
            floor = 2e-7 if name.startswith("pn_gamma") else (6e-8 if name in ("user_emb", "item_emb") or name.startswith("Wd") else 3e-8)
            np.testing.assert_allclose(a, w, rtol=5e-4, atol=max(4e-6 * max(np.abs(w).max(), 1e-3), floor), err_msg=name)
            if name in STAR_SLICED:         # the idle domains' slices: exact zeros
                idle = np.delete(a.reshape(case.D, -1), d, axis=0)
                assert not idle.any() and np.any(a), name
        else:
            np.testing.assert_allclose(a, w, rtol=2e-4, atol=max(2e-6 * max(np.abs(w).max(), 1e-3), floor_of(case, name)),
                                       err_msg=name)
    if not P.star:
        mag = np.abs(grads["domain_emb"]).max(axis=1)
        ids = np.unique(args[2])
        # (every row the batch names carries a gradient of its own; the others see the regulariser only)
        assert mag[ids].min() > 0 and (ids.shape[0] == case.D or mag[ids].min() > 10 * np.delete(mag, ids).max())
    if case.uncertainty:
        assert got["log_var"][d] != 0 and not np.delete(got["log_var"], d).any()
    if P.star:
        ostar.update_moving(model.state, c["d"], c["mean"], c["var"])
        aux = eng.aux_state()
        np.testing.assert_allclose(aux["steps"], model.state["steps"])
        np.testing.assert_allclose(aux["mov_mean"], model.state["mov_mean"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(aux["mov_var"], model.state["mov_var"], rtol=1e-4, atol=1e-7)


def check_untouched_rows(case, got, m, v, model, touched):
    """A domain row no batch names sees the regulariser alone, g = 2 l2 p: the same fp32 products on either side, no sum whose
    order could differ, so TF1's dense Adam moves it alike to rounding.  Three steps of ~1.4e-4 each (|p| ~ 0.05: m / (sqrt v +
    eps) = 0.43) against half an ulp of p per step (|p| < 0.25: 1.5e-8): the row within 5e-8, m and v -- products and
    well-conditioned sums -- within 1e-5 of their value (a few hundred ulp).  A skipped step shows as 1.4e-4, 3,000 times the bar."""
    rows = np.setdiff1d(np.arange(case.D), touched)
    if rows.size == 0:
        return
    w = {k: x.reshape(case.D, 128)[rows] for k, x in (("p", got), ("m", m), ("v", v))}
    o = {"p": model.params["domain_emb"][rows], "m": model.opt.m["domain_emb"][rows], "v": model.opt.v["domain_emb"][rows]}
    assert np.abs(o["p"]).max() < 0.25 and np.abs(o["m"]).max() > 0
    np.testing.assert_allclose(w["p"], o["p"], rtol=0, atol=5e-8, err_msg="untouched rows %r" % (rows[:8],))
    np.testing.assert_allclose(w["m"], o["m"], rtol=1e-5, atol=0, err_msg="adam m of untouched rows")
    np.testing.assert_allclose(w["v"], o["v"], rtol=1e-5, atol=0, err_msg="adam v of untouched rows")


def check_adam(P, d, cols):
    """(b) one call of three Adam steps, no loss output"""
    case, eng = P.case, P.eng
    model = P.fresh()
    assert eng.train_steps(d, first_step=0, n_steps=dc.STEPS, lr=1e-3) == dc.STEPS
    for s in range(dc.STEPS):
        model.train_on_batch(*dc.batch_of(cols, s, case.batch))
    got = eng.unpack(eng.get_weights())
    for name in model.names:
        t_par.assert_adam_close(got[name], model.params[name], dc.STEPS, 1e-3, case.name + " " + name, max_frac=2e-3)
    assert eng.counters() == (model.opt.t, model.step) == (dc.STEPS, dc.STEPS), eng.counters()
    m, v = eng.unpack(eng.adam_m)["domain_emb"], eng.unpack(eng.adam_v)["domain_emb"]
    for what, a, o in (("adam m", m, model.opt.m["domain_emb"]), ("adam v", v, model.opt.v["domain_emb"])):
        err, nrm = float(np.linalg.norm(a - o.ravel())), float(np.linalg.norm(o))
        print("%s %s domain_emb: err %.3e of %.3e" % (case.name, what, err, nrm))
        assert nrm > 0 and err <= 3e-2 * nrm, (what, err, nrm)
    check_untouched_rows(case, got["domain_emb"], m, v, model, np.unique(cols["domain"]))
    return model


def star_slots(P, rs):
    """non-zero Adam slots for domain 0's slice of every per-domain tensor: an idle slice with something to decay"""
    eng, D = P.eng, P.case.D
    out = {}
    for name in STAR_SLICED:
        per = eng.segments[name][1] // D
        out[name] = ((rs.standard_normal(per) * 1e-2).astype(F32), rs.uniform(1e-6, 1e-4, per).astype(F32))
    return out


def put_star_slots(P, slots, model=None):
    eng = P.eng
    for name, (m, v) in slots.items():
        off = eng.segments[name][0]
        eng.adam_m[off:off + m.size] = torch.from_numpy(m).to(eng.device)
        eng.adam_v[off:off + v.size] = torch.from_numpy(v).to(eng.device)
        if model is not None:
            model.opt.m[name][0] = m.reshape(model.opt.m[name][0].shape)
            model.opt.v[name][0] = v.reshape(model.opt.v[name][0].shape)


def check_star_adam(P, d, cols):
    """(b) for Star: the three steps as one call (lazy slices, k_star_catchup) and as three calls (the dense sweep)"""
    case, eng = P.case, P.eng
    D = case.D
    slots = star_slots(P, np.random.RandomState(5)) if D > 1 else {}
    runs = {}
    for mode in ("lazy", "dense"):
        model = P.fresh()
        put_star_slots(P, slots, model)
        if mode == "lazy":
            assert eng.train_steps(d, first_step=0, n_steps=dc.STEPS, lr=1e-3) == dc.STEPS
        else:
            for s in range(dc.STEPS):
                eng.train_steps(d, first_step=s, n_steps=1, lr=1e-3)
        assert eng.counters() == (dc.STEPS, dc.STEPS), (mode, eng.counters())
        runs[mode] = tuple(eng.unpack(x) for x in (eng.get_weights(), eng.adam_m, eng.adam_v))
    for s in range(dc.STEPS):
        model.train_on_batch(*dc.batch_of(cols, s, case.batch))
    assert (model.opt.t, model.step) == (dc.STEPS, dc.STEPS)
    for mode, (w, m, v) in runs.items():
        for name in model.names:
            if name == "domain_emb":        # Adam normalises its rounding-residue gradient: not comparable (test_star_step_adam_eval)
                idle = np.delete(w[name].reshape(D, 128), d, axis=0)
                assert np.array_equal(idle, np.delete(P.params[name], d, axis=0))       # zero gradient, zero slots: in place
                continue
            t_par.assert_adam_close(w[name], model.params[name], dc.STEPS, 1e-3, "%s %s %s" % (case.name, mode, name))
        if D > 1:
            # domain 0's slice decays from its slots with a zero gradient: the oracle's dense step to rounding (values up to
            # 0.8: half an ulp, 3e-8, per step and operand; a skipped step shows as ~1e-3)
            for name in STAR_SLICED:
                o_p, o_m, o_v = (x[name][0].ravel() for x in (model.params, model.opt.m, model.opt.v))
                per = o_p.size
                np.testing.assert_allclose(w[name][:per], o_p, rtol=0, atol=3e-7, err_msg="%s %s" % (mode, name))
                np.testing.assert_allclose(m[name][:per], o_m, rtol=1e-5, atol=0, err_msg="%s %s m" % (mode, name))
                np.testing.assert_allclose(v[name][:per], o_v, rtol=1e-5, atol=0, err_msg="%s %s v" % (mode, name))
                assert np.abs(o_p - P.params[name][0].ravel()).max() > 1e-4, name
    # the idle slices: the same bits out of the replay and out of the per-step sweep
    for what, a, b in zip(("weights", "adam m", "adam v"), runs["lazy"], runs["dense"]):
        for name in STAR_SLICED + ("domain_emb",):
            ia, ib = (np.delete(x[name].reshape(D, -1), d, axis=0) for x in (a, b))
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)), (what, name)
    return model


def check_eval(P, model):
    """(c) the evaluation split of domain 0 at equal weights"""
    case, eng = P.case, P.eng
    vd, vc = P.val
    eng.set_weights(eng.pack(model.params))
    loss, auc, hist, preds = eng.evaluate(vd, "val", want_preds=True)
    loss_o, preds_o = model.evaluate(vc, eng.eval_batch)
    p_rtol, p_atol, l_rel, a_abs = ((5e-4, 5e-5, 1e-4, 1e-3) if P.star else            # test_star_step_adam_eval
                                    (2e-5, 2e-7, 2e-6, 1e-4) if case.tower == "pnn" else     # test_eval_predictions_at_equal_weights
                                    (2e-4, 2e-5, 1e-4, 1e-7))                            # test_deepfm_gradients_adam_eval
    np.testing.assert_allclose(preds, preds_o, rtol=p_rtol, atol=p_atol)
    assert abs(loss - float(loss_o)) < l_rel * max(1.0, abs(float(loss_o))), (loss, float(loss_o))
    assert int(hist.sum()) == dc.EVAL_ROWS
    # (the reference metric of the engine's own predictions, as tests/test_gpu_edge_batches.py has it)
    assert abs(auc - float(oauc.auc500(vc["label"], preds, eng.eval_batch))) <= a_abs


@pytest.mark.parametrize("case,which", [(c, w) for c in dc.CASES for w in dc.which_of(c)],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_step_engine_at_domain_count(case, which):
    P = problem_of(case)
    d, cols = P.bind(which)
    args = dc.batch_of(cols, 0, case.batch)
    if which == "mixed":
        assert np.unique(args[2]).shape[0] == min(case.D, case.batch) and args[2].max() == case.D - 1 and args[2][0] == d
    else:
        assert np.all(args[2] == case.D - 1) and d == case.D - 1
    check_probe(P, d, args)
    model = check_star_adam(P, d, cols) if P.star else check_adam(P, d, cols)
    check_eval(P, model)


# ---------------------------------------------------------------------------------------------- the generic-layer engine
@pytest.mark.parametrize("n_domain", dc.GRAPH_D)
@pytest.mark.parametrize("kind", dc.MTL_KINDS)
def test_generic_mtl_towers_at_domain_count(kind, n_domain):
    """shared_bottom / mmoe / ple with 1 and 33 tasks: one-step gradients of the largest domain's and of the last domain's
    first batch, tests/test_gpu_mtl.py::test_one_step_gradients_match_oracle's bars"""
    g, eng, model, spec = t_mtl.make_problem(kind, n_domain=n_domain)
    checked = dc.mtl_problem(kind, n_domain)[2]         # (what the CPU suite held to float64 autograd: the same problem)
    assert sorted(checked) == sorted(model.params) and all(np.array_equal(model.params[n], checked[n]) for n in checked)
    for step, (d, args) in enumerate(dc.probe_batches(g)):
        n = args[0].shape[0]
        masks = omtl.train_masks(spec, model.seed, model.step, n, 0.5)
        loss, grads, _ = omtl.loss_and_grads(model.params, spec, d, *args, masks, 0.5, False, model.frozen_sumsq())
        loss_t = torch.zeros(1, device=eng.device)
        w0 = eng.get_weights()
        eng.train_steps(d, first_step=0, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
        got = eng.unpack(w0 - eng.get_weights())
        after = eng.get_weights().cpu().numpy()
        eng.set_weights(w0)
        model.step += 1
        assert abs(float(loss_t.cpu()[0]) - float(loss)) < 2e-6 * max(1.0, abs(float(loss)))
        for name in eng.segments:
            if name in grads:
                want = grads[name].ravel()
                np.testing.assert_allclose(got[name], want, rtol=2e-4, atol=max(2e-6 * max(np.abs(want).max(), 1e-3), 1.5e-8),
                                           err_msg=name)
            else:                         # not on task d's path: untouched, bit for bit
                off, cnt = eng.segments[name]
                assert np.array_equal(after[off:off + cnt], w0.cpu().numpy()[off:off + cnt]), name
    eng.close()


@pytest.mark.parametrize("n_domain", dc.GRAPH_D)
def test_generic_star_form_at_domain_count(n_domain):
    """pn + star + a 64-wide auxiliary network with 1 and 33 domains: tests/test_gpu_star_forms.py's probe and bars"""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    g = dc.star_form_problem(n_domain)
    eng, model, _ = t_sf.build(g, "pn", "star", 64, t_sf.H3)
    for d, args in dc.probe_batches(g):
        cols = g["data"]["train"][d]
        t_sf.probe_steps(eng, model, cols, d, 256, (0,), np.arange(cols["uid"].shape[0], dtype=np.int32), True)
    eng.close()
