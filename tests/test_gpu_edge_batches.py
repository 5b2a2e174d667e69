"""Every tower on both engines at batches placed ON the kernels' tile boundaries (the reference keeps the final partial batch
of a pass, `utils/dataset.py:20-38`; a pass over 256 + r rows is one full batch and one of r rows).

The generic-layer engine pads a step to rp = ceil(rows / 64) * 64 rows and contracts every weight gradient and bias column
sum over rp rows, so every backward kernel has to leave exact zeros in the padded rows of `dact`; its split-K choice differs
between 64 rows and 128.  The step engine works in 16-row tiles, 4-row tiles and 16-row Star chunks.  Here one domain is
trimmed to n = 256 + r rows: step 0 (a full batch) leaves live values in every padded row, step 1 -- r rows -- is the one
under test, with r on each side of those boundaries (generic: 1, 17, 63, 64, 65; step: 1, 3, 4, 5, 15, 16, 17).

Per case: the SGD probe of the ragged step against the oracle (loss, every tensor on the path -- the bias gradients are the
column sums over rp rows --, everything off the path bit-unchanged), step 0 again afterwards (the pad rows of the ragged
step must not leak into it), a two-step Adam pass with both counters, the evaluation of the same r rows, and with trainable
tables the gradient of every table row outside the batch read through the accumulator.  One engine per tower kind serves
all its row counts.  The oracles are held to float64 autograd at these row counts in tests/test_oracle_crosscheck.py and
tests/test_star_forms_ref.py.

Inputs: every ragged batch used here was checked on the CPU with the harness of tests/test_oracle_crosscheck.py (the oracle
alone against float64 autograd, `_check_grads`' bars, loss 2e-6): all 85 non-Star batches are fit at the siblings' seeds, the
Star kinds apply `fit_reference` per batch (it never had to switch).  One input was moved: FIRST_ROW below.

Bars are the existing ones of each family's own file, unchanged:
  deepfm / wdl (step)          tests/test_gpu_parity.py::test_deepfm_gradients_adam_eval, tests/test_gpu_edges.py
  star (step) and the forms    tests/test_gpu_parity.py::test_star_step_adam_eval, tests/test_gpu_star_forms.py
  nfm / pnn / ccpm / autoint   tests/test_gpu_fmnets.py (both engines)
  shared_bottom / mmoe / ple   tests/test_gpu_mtl.py
  mlp at hidden (128, 64)      tests/test_gpu_hidden.py
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import star_forms_ref as sref                       # noqa: E402
import test_gpu_fmnets as t_fm                      # noqa: E402
import test_gpu_hidden as t_hid                     # noqa: E402
import test_gpu_mtl as t_mtl                        # noqa: E402
import test_gpu_parity as t_par                     # noqa: E402
import test_gpu_star_forms as t_sf                  # noqa: E402
from oracle import auc as oauc                      # noqa: E402
from oracle import fmnets as ofm                    # noqa: E402
from oracle import mtl as omtl                      # noqa: E402
from oracle import star as ostar                    # noqa: E402
from oracle import tower as otower                  # noqa: E402

F32 = np.float32
B = 256
STEP_R = (1, 3, 4, 5, 15, 16, 17)          # k_tower4's 4-row tiles, the 16-row tiles and Star chunks
GRAPH_R = (1, 17, 63, 64, 65)              # rp = 64 (no split-K) up to 64 rows, 128 (split 2) at 65
STEP_KINDS = ["deepfm@step", "wdl@step", "star@step", "pnn@step", "nfm@step"]
GRAPH_KINDS = ["shared_bottom", "mmoe", "ple", "nfm", "pnn", "ccpm", "autoint", "mlp", "star:pn/star/64", "star:bn/dense/0",
               "star:none/star/0"]
TRAINABLE = ["deepfm@step", "star@step", "mmoe", "autoint", "star:pn/star/64"]
assert ("none", "star", 0, t_sf.H3) in t_sf.FORMS
# Where in the domain's file order the 256 + r rows start.  none/star/0 starts 256 rows in: in its first 256 rows one unit of
# layer 0 has a pre-activation of 7.5e-9 (positive in the fp32 reference and in float64); the engine's contraction order rounds
# it to the other side of the relu, and bs0 / Ws0 / domain_emb of that FULL batch differ by that one row's share, 1.3e-3 of
# the tensor (the deeper layers agree to 1e-7).  The next 256 rows have no unit within 2e-7 of the kink.  Same bars.
FIRST_ROW = {"star:none/star/0": 256}


def r_of(kind):
    return STEP_R if kind.endswith("@step") else GRAPH_R


CASES = [(k, e, r) for k, e in [(k, False) for k in STEP_KINDS + GRAPH_KINDS] + [(k, True) for k in TRAINABLE] for r in r_of(k)]


def _id(v):
    return {True: "trainable", False: "frozen"}.get(v, str(v)) if isinstance(v, bool) else str(v)


# ---------------------------------------------------------------------------------------------- one engine per tower kind
class Problem(object):
    """the engine of one tower kind with its pristine oracle; `fam` names the oracle and the bars."""

    def __init__(self, kind, emb_trainable):
        from mamdr_amd import engine, synthetic
        self.kind, self.emb_trainable, self.spec = kind, emb_trainable, None
        scale = 0.1 if emb_trainable else 0.05
        base = kind.split("@")[0]
        if kind in ("deepfm@step", "wdl@step"):
            self.fam = "tower"
            g, eng, model = t_par.make_problem((engine, synthetic), scale=scale, emb_trainable=emb_trainable, tower=base)
        elif kind == "star@step":
            self.fam = "star"
            g, eng, model = t_par.make_star_problem((engine, synthetic), emb_trainable, scale=0.1)
            model.norm, model.dense, model.auxiliary_dim = "pn", "star", 0          # (what fit_reference reads)
        elif base in ("nfm", "pnn", "ccpm", "autoint"):
            self.fam = "fm"
            g, eng, model = t_fm.make_problem(kind, scale=scale, emb_trainable=emb_trainable)
        elif kind in t_mtl.SHAPES:
            self.fam = "mtl"
            g, eng, model, self.spec = t_mtl.make_problem(kind, scale=scale, emb_trainable=emb_trainable)
        elif kind == "mlp":
            self.fam = "hidden"
            g, eng, model = t_hid.make_problem("mlp", (128, 64), scale=scale, emb_trainable=emb_trainable)
        else:
            self.fam = "star"
            norm, dense, aux = kind.split(":")[1].split("/")
            g = t_sf.problem(scale=0.1)
            eng, model, _ = t_sf.build(g, norm, dense, int(aux), t_sf.H3, emb_trainable)
        self.g, self.eng, self.model0 = g, eng, model
        self.step_engine = kind.endswith("@step")
        self.normed = self.fam == "star" and model.norm != "none"
        self.d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
        lo = FIRST_ROW.get(kind, 0)
        self.src = {k: v[lo:] for k, v in g["data"]["train"][self.d].items()}
        assert self.src["uid"].shape[0] >= B + 2 * max(r_of(kind)) + 16
        self.saved = {s: g["data"][s][self.d] for s in ("train", "val")}
        self.w0 = eng.get_weights()
        self.aux0 = eng.aux.clone() if eng.aux is not None else None
        self.step0 = None           # the oracle's step 0 (the same full batch whatever r is): computed once

    def close(self):
        self.eng.close()

    def fresh(self):
        """engine and oracle back at the start: weights, zero slots, both counters, the norm layer's statistics."""
        eng = self.eng
        eng.set_weights(self.w0)
        eng.optimizer_reset()
        eng.set_counters(0, 0)
        if self.aux0 is not None:
            eng.aux.copy_(self.aux0)
        return copy.deepcopy(self.model0)

    def rewind(self):
        """both counters and the norm layer's statistics back at the start (the weights were put back by the probes)."""
        self.eng.set_counters(0, 0)
        if self.aux0 is not None:
            self.eng.aux.copy_(self.aux0)

    def columns(self, r):
        """256 + r rows of the domain in file order; with trainable tables the last r avoid the first and the last row of
        both tables (a padded row that gathered through index 0, or a clamped one, would show in those rows' gradient)."""
        src, g = self.src, self.g
        ok = np.ones(src["uid"].shape[0] - B, bool)
        if self.emb_trainable:
            ok = ~np.isin(src["uid"][B:], (0, g["n_user"] - 1)) & ~np.isin(src["pid"][B:], (0, g["n_item"] - 1))
        tail = B + np.flatnonzero(ok)[:r]
        assert tail.shape[0] == r
        idx = np.concatenate([np.arange(B), tail])
        cols = {k: np.ascontiguousarray(v[idx]) for k, v in src.items()}
        last = {k: np.ascontiguousarray(v[B:]) for k, v in cols.items()}
        if self.emb_trainable:
            assert 0 not in last["uid"] and g["n_user"] - 1 not in last["uid"]
            assert 0 not in last["pid"] and g["n_item"] - 1 not in last["pid"]
        return cols, last

    # ------------------------------------------------------------------ the oracle's side of one probed step
    def oracle_step(self, model, c):
        """loss and gradients of one batch at the model's weights; the dropout position and the moving statistics advance as
        the engine's do in an SGD probe."""
        args = (c["uid"], c["pid"], c["domain"], c["label"])
        n = c["uid"].shape[0]
        if self.fam in ("tower", "hidden"):
            masks = otower.train_masks(model.seed, model.step, n, model.hidden, model.rate)
            loss, grads, _ = otower.loss_and_grads(model.params, *args, masks, model.rate, self.emb_trainable,
                                                   model.frozen_sumsq(), model.deepfm)
        elif self.fam == "fm":
            base = self.kind.split("@")[0]
            masks = otower.train_masks(model.seed, model.step, n, t_fm.HIDDEN, 0.5)
            fn = ofm.loss_and_grads_conv if base in ("ccpm", "autoint") else ofm.loss_and_grads
            loss, grads, _ = fn(model.params, base, *args, masks, 0.5, self.emb_trainable, model.frozen_sumsq())
        elif self.fam == "mtl":
            masks = omtl.train_masks(self.spec, model.seed, model.step, n, 0.5)
            loss, grads, _ = omtl.loss_and_grads(model.params, self.spec, self.d, *args, masks, 0.5, self.emb_trainable,
                                                 model.frozen_sumsq())
        else:
            if isinstance(model, ostar.OracleStar):
                loss, grads, _, cc = ostar.loss_and_grads(model.params, model.state, *args, self.emb_trainable)
            else:
                loss, grads, _, cc = model.loss_and_grads(*args)
            # fit_reference's rule as it stands: float64 autograd judges a batch on which the fp32 reference misses its own bar
            grads = t_sf.fit_reference(model, grads, args, self.normed)
            if model.norm != "none":
                sref.update_moving(model.state, model.norm, cc["d"], cc["mean"], cc["var"])
        model.step += 1
        return float(loss), {k: np.asarray(otower.bigtable.densify(v), F32) for k, v in grads.items()}

    def probe(self, step):
        """SGD probe (lr 1) of one step: -> (loss, w0 - w as a flat vector, the weights after the step); weights put back."""
        eng = self.eng
        w0 = eng.get_weights()
        loss_t = torch.zeros(1, device=eng.device)
        eng.train_steps(self.d, first_step=step, n_steps=1, lr=1.0, optimizer="sgd", loss_out=loss_t)
        after = eng.get_weights()
        eng.set_weights(w0)
        return float(loss_t.cpu()[0]), (w0 - after).cpu().numpy(), after.cpu().numpy()

    # ------------------------------------------------------------------ the bars, by family
    def floors(self, name):
        table = name in ("user_emb", "item_emb")
        if self.fam == "tower":         # test_gpu_parity.py::test_deepfm_gradients_adam_eval
            return 6e-8 if table else 1e-8
        return 4e-8 if table else 1.5e-8        # test_gpu_fmnets.py / test_gpu_hidden.py / test_gpu_mtl.py

    def check_grads(self, got, after, grads, w_before, single_row):
        eng = self.eng
        if self.fam == "star":
            got = got.copy()
            if single_row and self.normed:
                # ONE row under a norm: x - mean = 0, the normalised input is beta whatever x is, and the reference's gradient
                # of gamma and of all 384 input columns (the tables' rows, the domain row) is exactly 0.  The engine's is
                # exactly 0 or rounding residue below the bound of the domain row's rule (1e-5); which of the two is printed.
                # Measured on an MI355X: EXACTLY 0 for every one of these tensors on both engines (star@step, pn/star/64 and
                # bn/dense/0, frozen and trainable tables) -- x - mean is an exact 0 there too.
                for name in ("pn_gamma_shared", "pn_gamma_spec", "bn_gamma", "user_emb", "item_emb", "domain_emb"):
                    if name in eng.segments and name in grads:
                        off, cnt = eng.segments[name]
                        assert not np.any(grads[name]), name
                        worst = float(np.abs(got[off:off + cnt]).max())
                        print("r = 1, %s: gradient of %s %s" % (self.kind, name, "exactly 0" if worst == 0 else "residue %.2e" % worst))
                        assert worst < 1e-5, (name, worst)
                        got[off:off + cnt] = 0
            # rtol 5e-4, atol max(4e-6 max|w|, floor); the idle domains' slices exact zeros; domain_emb under a norm: < 1e-5
            t_sf.check_grads(eng, got, grads, self.model0.params, self.normed)
            return
        named = eng.unpack(torch.from_numpy(got))
        before, now = eng.unpack(torch.from_numpy(w_before)), eng.unpack(torch.from_numpy(after))
        biases = [n for n in grads if n.split("/")[-1][0] == "b" or n.endswith("gb") or n.endswith("_b")]
        assert biases, sorted(grads)
        for name in biases + [n for n in grads if n not in biases]:      # (the bias gradients: column sums over rp rows)
            want = grads[name].ravel()
            np.testing.assert_allclose(named[name], want, rtol=2e-4,
                                       atol=max(2e-6 * max(np.abs(want).max(), 1e-3), self.floors(name)), err_msg=name)
        for name in named:
            if name not in grads:           # off the path: bit-unchanged
                assert np.array_equal(now[name].view(np.uint32), before[name].view(np.uint32)), name

    def check_state(self, model, after_adam=False):
        """moving mean / variance and pn's steps; after Adam steps the forms compare the user / item columns only (check_state's
        docstring) and the step kernels' family does not compare (test_star_step_adam_eval)."""
        if self.fam != "star":
            return
        if after_adam:
            if not isinstance(model, ostar.OracleStar):
                t_sf.check_state(self.eng, model, domain_cols=False)
        elif isinstance(model, ostar.OracleStar):       # test_gpu_parity.py::test_star_step_adam_eval
            aux = self.eng.aux_state()
            np.testing.assert_allclose(aux["steps"], model.state["steps"])
            np.testing.assert_allclose(aux["mov_mean"], model.state["mov_mean"], rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(aux["mov_var"], model.state["mov_var"], rtol=1e-4, atol=1e-7)
        else:
            t_sf.check_state(self.eng, model)

    def check_adam(self, model, n_steps, start):
        eng = self.eng
        got = eng.unpack(eng.get_weights())
        if self.fam == "star" and not isinstance(model, ostar.OracleStar):
            t_sf.displacement(eng, model, start)            # test_gpu_star_forms.py
        elif self.fam == "hidden":                          # test_gpu_hidden.py::test_adam_pass_and_evaluation_match_oracle
            for name in model.names:
                a, o, s = np.asarray(got[name]).ravel(), model.params[name].ravel(), np.asarray(start[name]).ravel()
                nrm, err = float(np.linalg.norm(o - s)), float(np.linalg.norm(a - o))
                assert err <= 3e-2 * nrm + 1e-6 * float(np.linalg.norm(s)) + 1e-7, (name, err, nrm)
        elif self.fam == "mtl":                             # test_gpu_mtl.py
            for name in eng.segments:
                t_mtl.assert_adam_close(got[name], model.params[name], n_steps, 1e-3, name)
        else:
            for name in model.names:
                if name == "domain_emb" and self.fam == "star":
                    continue        # Adam normalises its rounding-residue gradient: not comparable (test_star_step_adam_eval)
                # test_star_step_adam_eval: the default 1e-3; deepfm / wdl / the step kernels' PNN and NFM: 2e-3
                t_par.assert_adam_close(got[name], model.params[name], n_steps, 1e-3, name,
                                        **({} if self.fam == "star" else {"max_frac": 2e-3}))
        t = model.t if self.fam == "mtl" else model.opt.t
        assert eng.counters() == (t, model.step), (eng.counters(), t, model.step)

    def evaluate(self, model, cols):
        if self.fam == "mtl":
            return model.evaluate(self.d, cols, B)
        return model.evaluate(cols, B)

    def check_eval(self, model, last):
        """the r rows as the val split, at equal weights: predictions, loss, histogram total, AUC-500."""
        eng, r = self.eng, last["uid"].shape[0]
        loss, auc, hist, preds = eng.evaluate(self.d, "val", want_preds=True)
        loss_o, preds_o = self.evaluate(model, last)
        # predictions / loss / AUC at equal weights, as the family's own file has them
        p_rtol, p_atol, l_rel, a_abs = {"tower": (2e-4, 2e-5, 1e-4, 1e-7),       # test_deepfm_gradients_adam_eval; test_gpu_edges.py
                                        "fm": (2e-5, 2e-7, 2e-6, 1e-4),          # test_eval_predictions_at_equal_weights
                                        "mtl": (2e-5, 2e-7, 2e-6, 1e-4),         # test_eval_predictions_match_oracle_at_equal_weights
                                        "hidden": (2e-4, 2e-5, 1e-4, 1e-3),      # test_adam_pass_and_evaluation_match_oracle (no
                                        #                                          prediction bar of its own: deepfm's)
                                        "star": (5e-4, 5e-5, 1e-4, 1e-3)}[self.fam]   # test_gpu_star_forms.py::evaluate_both
        np.testing.assert_allclose(preds, preds_o, rtol=p_rtol, atol=p_atol)
        assert abs(loss - float(loss_o)) < l_rel * max(1.0, abs(float(loss_o))), (loss, float(loss_o))
        assert int(hist.sum()) == r
        # (the reference metric of the engine's own predictions: a prediction within rounding of one of the 500 thresholds
        # would move a whole row of so short a split to the next bin)
        assert abs(auc - float(oauc.auc500(last["label"], preds, B))) <= a_abs
        if r == 1:          # one class: the reference metric's guarded 0 (utils/auc.py:248-281), as in test_gpu_edges.py
            assert auc == 0.0 and float(oauc.auc500(last["label"], preds_o, B)) == 0.0

    def bit_exact_reruns(self):
        """the Star forms assert run-to-run bit equality (test_two_engines_take_identical_steps)."""
        return self.fam == "star" and not self.step_engine


_LIVE = {}


def problem_of(kind, emb_trainable):
    """one engine per (kind, tables): the cases of a kind follow each other, the previous kind's engine is closed."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    key = (kind, emb_trainable)
    if key not in _LIVE:
        for p in _LIVE.values():
            p.close()
        _LIVE.clear()
        _LIVE[key] = Problem(kind, emb_trainable)
    return _LIVE[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for p in _LIVE.values():
        p.close()
    _LIVE.clear()


# ---------------------------------------------------------------------------------------------- 1. a full batch, then r rows
@pytest.mark.parametrize("kind,emb_trainable,r", CASES, ids=_id)
def test_ragged_step_after_a_full_batch(kind, emb_trainable, r):
    """a pass over 256 + r rows of one domain in file order: step 0 is a full batch, step 1 the r rows (module docstring)."""
    P = problem_of(kind, emb_trainable)
    eng, d = P.eng, P.d
    cols, last = P.columns(r)
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    eng.bind_domain_data(d, "val", last["uid"], last["pid"], last["domain"], last["label"])
    first = {k: v[:B] for k, v in cols.items()}
    try:
        # ---- the SGD probes: step 0 fills every padded row, step 1 is the ragged one
        model = P.fresh()
        w_start = eng.get_weights().cpu().numpy()
        if P.step0 is None:
            m0 = copy.deepcopy(model)
            P.step0 = P.oracle_step(m0, first) + (m0,)
        loss0, grads0, after0 = P.step0
        model = copy.deepcopy(after0)
        if P.bit_exact_reruns():        # (step 0 through the accumulator, before anything ragged ran)
            acc_a = eng.new_vector()
            eng.bind_accumulator(acc_a)
            eng.train_steps(d, first_step=0, n_steps=1, optimizer="accumulate")
            P.rewind()
        got_loss, got0, after = P.probe(0)
        assert abs(got_loss - loss0) < 2e-6 * max(1.0, abs(loss0))
        P.check_grads(got0, after, grads0, w_start, False)
        loss1, grads1 = P.oracle_step(model, last)
        got_loss, got1, after = P.probe(1)
        print("%s r = %d: loss hip %.7f oracle %.7f" % (kind, r, got_loss, loss1))
        assert abs(got_loss - loss1) < 2e-6 * max(1.0, abs(loss1))
        P.check_grads(got1, after, grads1, w_start, r == 1)
        P.check_state(model)
        # ---- the same r rows as the val split, at the probes' (equal) weights and the statistics the two probes left
        P.check_eval(model, last)
        # ---- the pad rows of the ragged step do not leak into a following full step
        P.rewind()
        if P.bit_exact_reruns():        # bit equality where the family asserts it (test_two_engines_take_identical_steps)
            acc_b = eng.new_vector()
            eng.bind_accumulator(acc_b)
            eng.train_steps(d, first_step=0, n_steps=1, optimizer="accumulate")
            assert torch.equal(acc_a.view(torch.int32), acc_b.view(torch.int32))
        else:                           # the gradient bars, the first run of step 0 as the reference
            _, again, after = P.probe(0)
            P.check_grads(again, after, _named(eng, got0, grads0), w_start, False)
        # ---- trainable tables: the rows outside the ragged batch, through the accumulator
        if emb_trainable:
            _check_rows_outside_the_batch(P, last)
        # ---- two Adam steps from fresh state, both counters
        model = P.fresh()
        start = eng.unpack(eng.get_weights())
        losses = torch.zeros(2, device=eng.device)
        assert eng.train_steps(d, lr=1e-3, loss_out=losses) == 2
        model.lr = 1e-3
        perm = np.arange(B + r)
        want = model.train_pass(d, cols, perm, B) if P.fam == "mtl" else model.train_pass(cols, perm, B)
        # (per-step losses of a pass: tests/test_gpu_edges.py; the second step's weights carry one Adam step's noise)
        np.testing.assert_allclose(losses.cpu().numpy(), np.asarray(want, F32), rtol=3e-5, atol=1e-6)
        P.check_adam(model, 2, start)
        P.check_state(model, after_adam=True)
    finally:
        for split in ("train", "val"):
            c = P.saved[split]
            eng.bind_domain_data(d, split, c["uid"], c["pid"], c["domain"], c["label"])


def _named(eng, flat, like):
    """the engine's own first step-0 gradient as the reference of its repetition, on the tensors `like` names."""
    named = eng.unpack(torch.from_numpy(flat))
    return {k: np.asarray(named[k], F32).reshape(np.shape(like[k])) for k in like}


def _check_rows_outside_the_batch(P, last):
    """MAMDR_OPT_ACCUMULATE adds the step's gradient to a zeroed vector (dropout off: the meta passes' mode).  A table row no
    row of the batch names -- row 0 and the last row among them, where a padded row's gather would land -- receives nothing
    from the batch: its gradient is exactly the regulariser's 2 l2 w (the deepctr towers; test_trainable_tables_gradients_
    and_adam) and exactly 0 in the Star family, which has none (oracle/star.py)."""
    eng, d = P.eng, P.d
    P.fresh()
    P.probe(0)
    acc = eng.new_vector()
    eng.bind_accumulator(acc)
    w = eng.unpack(eng.get_weights())
    eng.train_steps(d, first_step=1, n_steps=1, optimizer="accumulate")
    got = eng.unpack(acc)
    E = 128
    for name, ids, width in (("user_emb", last["uid"], E), ("item_emb", last["pid"], E), ("lin_user", last["uid"], 1),
                             ("lin_item", last["pid"], 1)):
        if name not in got:
            continue
        rows = got[name].reshape(-1, width)
        outside = np.setdiff1d(np.arange(rows.shape[0]), ids)
        assert 0 in outside and rows.shape[0] - 1 in outside and outside.shape[0] >= rows.shape[0] - ids.shape[0]
        reg = np.zeros_like(rows) if P.fam == "star" else (F32(2) * F32(1e-5)) * w[name].reshape(-1, width)
        bad = np.flatnonzero((rows[outside].view(np.uint32) != reg[outside].astype(F32).view(np.uint32)).any(axis=1))
        assert bad.size == 0, (name, outside[bad][:8], rows[outside[bad][:2]], reg[outside[bad][:2]])
        if not (P.normed and ids.shape[0] == 1):            # (one row under a norm: its own rows' gradient is 0 too, see check_grads)
            assert np.any(rows[np.unique(ids)])             # ... and the batch's own rows did receive theirs


# ---------------------------------------------------------------------------------------------- 2. the batch size argument itself
@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("kind", ["deepfm@step", "mmoe"])
def test_batch_size_argument_of_one_and_65_rows(kind, batch):
    """train_steps(batch_size = 1 / 65) on a 130-row domain: three Adam steps against the oracle's pass at that batch size."""
    P = problem_of(kind, False)
    eng, d = P.eng, P.d
    cols = {k: np.ascontiguousarray(v[:130]) for k, v in P.src.items()}
    eng.bind_domain_data(d, "train", cols["uid"], cols["pid"], cols["domain"], cols["label"])
    try:
        model = P.fresh()
        losses = torch.zeros(3, device=eng.device)
        assert eng.train_steps(d, n_steps=3 if batch == 1 else None, lr=1e-3, loss_out=losses, batch_size=batch) == (3 if batch == 1 else 2)
        if batch == 65:
            eng.train_steps(d, first_step=0, n_steps=1, lr=1e-3, loss_out=losses[2:], batch_size=batch)
        model.lr = 1e-3
        perm = np.arange(130)
        if batch == 1:
            want = model.train_pass(d, cols, perm, 1, max_steps=3) if P.fam == "mtl" else model.train_pass(cols, perm, 1, max_steps=3)
        else:
            want = []
            for n in (2, 1):
                want += model.train_pass(d, cols, perm, 65, max_steps=n) if P.fam == "mtl" else model.train_pass(cols, perm, 65, max_steps=n)
        np.testing.assert_allclose(losses.cpu().numpy(), np.asarray(want, F32), rtol=3e-5, atol=1e-6)
        P.check_adam(model, 3, None)
    finally:
        c = P.saved["train"]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])


# ---------------------------------------------------------------------------------------------- 3. the generic-layer engine's refusals
def _state(eng):
    return (eng.weights.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.counters())


def _unchanged(eng, s):
    return torch.equal(eng.weights, s[0]) and torch.equal(eng.adam_m, s[1]) and torch.equal(eng.adam_v, s[2]) and eng.counters() == s[3]


def test_generic_engine_zero_steps_is_a_no_op():
    """mamdr_graph_*: n_steps = 0 leaves the weights, both Adam slots and both counters bit-unchanged (its twin for the step
    engine: tests/test_gpu_edges.py::test_zero_steps_is_a_no_op)."""
    P = problem_of("mmoe", False)
    eng = P.eng
    P.fresh()
    eng.train_steps(P.d, n_steps=1, lr=1e-3)            # (non-zero slots and counters to keep)
    s = _state(eng)
    assert eng.train_steps(P.d, n_steps=0) == 0
    torch.cuda.synchronize()
    assert _unchanged(eng, s) and s[3] == (1, 1)


def test_generic_engine_empty_split_and_bad_arguments_are_errors():
    """the twin of tests/test_gpu_edges.py::test_empty_split_and_bad_arguments_are_errors for mamdr_graph_*: every refusal is an
    error code with a message (mamdr_graph_last_error), never a silent no-op, and changes nothing; the context works afterwards."""
    from mamdr_amd import _lib as L
    P = problem_of("mmoe", False)
    eng, g = P.eng, P.g
    P.fresh()
    eng.train_steps(P.d, n_steps=1, lr=1e-3)
    empty = (P.d + 1) % g["n_domain"]
    saved = {s: g["data"][s][empty] for s in ("train", "val")}
    none = {k: v[:0] for k, v in saved["train"].items()}
    n_pass = -(-eng.n_rows(P.d, "train") // B)
    try:
        for split in ("train", "val"):
            eng.bind_domain_data(empty, split, none["uid"], none["pid"], none["domain"], none["label"])
        s = _state(eng)
        assert eng.n_rows(empty, "train") == 0
        assert eng.train_steps(empty) == 0                  # ceil(0 / B) = 0 steps: nothing to run, nothing changes
        assert _unchanged(eng, s)
        refusals = [
            lambda: eng.train_steps(empty, n_steps=1),                          # a step on an empty domain
            lambda: eng.evaluate(empty, "val"),                                 # `model.evaluate(steps=0)` has no defined result
            lambda: eng.train_steps(P.d, batch_size=eng.batch_size + 64),       # beyond max_batch
            lambda: eng.train_steps(P.d, batch_size=-16),
            lambda: L.check(eng.lib.mamdr_graph_train_steps(eng.ctx, g["n_domain"], None, 0, 1, B, eng.dropout_seed, L.OPT_ADAM,
                                                            1e-3, None), graph=True),      # no such domain
            lambda: eng.train_steps(P.d, first_step=n_pass, n_steps=1),         # beyond the pass
        ]
        for k, call in enumerate(refusals):
            with pytest.raises(L.MamdrError):
                call()
            assert eng.lib.mamdr_graph_last_error(), k
            torch.cuda.synchronize()
            assert _unchanged(eng, s), k
    finally:
        for split in ("train", "val"):
            c = saved[split]
            eng.bind_domain_data(empty, split, c["uid"], c["pid"], c["domain"], c["label"])
    w = eng.weights.clone()         # the context still works after the refusals
    eng.train_steps(P.d, n_steps=1, lr=1e-3)
    torch.cuda.synchronize()
    assert not torch.equal(eng.weights, w) and eng.counters() == (2, 2)
