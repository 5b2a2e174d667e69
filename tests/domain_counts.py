"""The cases and inputs of tests/test_gpu_domain_counts.py: the step engine at the domain counts where its kernels change
path.  They live here, without a GPU import, because the CPU suite checks every one of these batches first: the oracle
alone against float64 autograd at `_check_grads`' bars (tests/test_oracle_crosscheck.py::test_domain_count_inputs_are_fit),
so that a batch with a hidden unit within rounding of the relu kink never reaches the GPU file.

A problem is 64 users, 64 items and D domains; its parameters come from the oracles' own initialisers, moved off their
special initial values the way tests/test_gpu_parity.py::make_problem / make_star_problem and tests/test_gpu_fmnets.py::
make_problem do.  Per problem two train splits of three batches each and one evaluation split:
  mixed   every domain id 0 .. D - 1 occurs in every batch, shuffled (D > batch: the ids D - batch .. D - 1); the first row of
          each batch carries the id the split is bound under (uncertainty weighting reads the call's domain)
  one     all rows carry id D - 1
  val     EVAL_ROWS rows of domain id 0
The inputs depend on (tower, tables, uncertainty, D, batch) only, so the fused and the slab path of one count see the same rows.
"""
import collections

import numpy as np

from oracle import fmnets as ofm
from oracle import star as ostar
from oracle import tower as otower

F32 = np.float32
N_USER = N_ITEM = 64
HIDDEN = (256, 128, 64)
EVAL_ROWS = 100
DROPOUT_SEED = 1024         # engine.TowerEngine's default
STEPS = 3
WHICH = ("mixed", "one")

# path: "fused" k_tower4 + k_wgrad_adam; "fused16" k_tower (tower_tile = 16) + k_wgrad_adam; "slab" the mlp context
# created under MAMDR_FUSED=0 (k_wgrad -> slabs -> k_update);
# "plain" contexts that have no fused path to switch off (D > 64, the other towers); "star" the Star step
Case = collections.namedtuple("Case", "name tower D batch path trainable uncertainty")


def wgrad_groups(rows_pad):
    """mamdr_api.hip::wgrad_groups: the row groups (= gradient slabs) of a step of rows_pad rows."""
    r = 256 if rows_pad <= 512 else (128 if rows_pad <= 1024 else (256 if rows_pad <= 4096 else 512))
    groups = -(-rows_pad // r)
    if groups > 16:
        r = (-(-rows_pad // 16) + 7) // 8 * 8
        groups = -(-rows_pad // r)
    return groups


def wide_batch():
    """the smallest step (in whole 16-row tiles) with more than 8 row groups: k_update's WIDE form."""
    rows = 16
    while wgrad_groups(rows) <= 8:
        rows += 16
    return rows


WIDE = wide_batch()


def _case(boundary, tower, D, batch, path, trainable=False, uncertainty=False):
    name = "%s-%s-D%d-b%d-%s" % (tower + ("+uw" if uncertainty else "") + ("+tables" if trainable else ""), path, D, batch, boundary)
    return Case(name, tower, D, batch, path, trainable, uncertainty)


def _mt(D):
    return "MT%d" % (-(-D // 16))


FUSED = ([_case(_mt(D) + ("hi" if D % 16 == 0 or D == 1 else "lo"), "mlp", D, 256, "fused") for D in (1, 16, 17, 32, 33, 48, 49, 64)] +
         [_case("writer-rows", "mlp", D, 8, "fused") for D in (17, 64)] +
         [_case("full-grid", "mlp", 64, 1024, "fused")] +
         # the sixteen-row tower on the same path: ITS writer lanes (dm_tile_writer) step the rows no workgroup owns
         [_case("writer-rows-k_tower", "mlp", D, 8, "fused16") for D in (17, 64)] +
         [_case("writer-rows-k_tower", "mlp", 64, 256, "fused16")])
SLAB = ([_case("narrow-%d" % D, "mlp", D, 256, "slab") for D in (8, 9, 16, 17, 32, 33, 64)] +
        [_case("wide-%d" % D, "mlp", D, WIDE, "slab") for D in (32, 33, 64)])
BEYOND = [_case("no-linear-w0", "mlp", 65, 256, "plain"), _case("no-linear-w0-wide", "mlp", 65, WIDE, "plain"),
          _case("no-linear-w0-s2", "deepfm", 65, 256, "plain"), _case("no-linear-w0-tiny", "mlp", 65, 5, "plain")]
LAYOUT = [_case("mod4=%d" % (D % 4), tower, D, 256, "plain", trainable, uw)
          for tower, trainable, uw in (("deepfm", False, False), ("deepfm", True, False), ("wdl", False, False),
                                       ("pnn", False, False), ("mlp", False, True))
          for D in (33, 34, 35)]
STAR = [_case({1: "no-lazy", 2: "one-idle", 33: "grid-y", 65: "beyond-64"}[D], "star", D, 256, "star") for D in (1, 2, 33, 65)]
CASES = FUSED + SLAB + BEYOND + LAYOUT + STAR
assert len({c.name for c in CASES}) == len(CASES)

# Inputs moved after the CPU check: {(tower, trainable, uncertainty, D, batch): seed}.  None had to be.
MOVED_SEEDS = {}


def which_of(case):
    """the Star step takes one-domain batches only (the first row's domain serves the batch: oracle/star.py)"""
    return ("one",) if case.tower == "star" else WHICH


def input_key(case):
    return (case.tower, case.trainable, case.uncertainty, case.D, case.batch)


def seed_of(case):
    k = input_key(case)
    return MOVED_SEEDS.get(k, 100 + 7 * case.D + case.batch % 97 + 1000 * ("mlp", "deepfm", "wdl", "pnn", "star").index(case.tower)
                           + 500 * case.trainable + 250 * case.uncertainty)


def make_params(case, rs):
    D, tower = case.D, case.tower
    if tower == "star":         # tests/test_gpu_parity.py::make_star_problem
        p = ostar.init_params(rs, N_USER, N_ITEM, D)
        for n in ("pn_gamma_shared", "pn_gamma_spec"):
            p[n] = (p[n] + rs.standard_normal(p[n].shape) * 0.2).astype(F32)
        for n in ("pn_beta_shared", "pn_beta_spec", "bs0", "bs1", "bs2", "bd0", "bd1", "bd2", "gb"):
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        for l in range(3):
            p["Wd%d" % l] = (p["Wd%d" % l] * 8).astype(F32)
        p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
        return p
    if tower == "pnn":          # tests/test_gpu_fmnets.py::make_problem
        p = ofm.init_params(rs, "pnn", N_USER, N_ITEM, D, hidden=HIDDEN)
        for n in ("b0", "b1", "b2", "lin_domain", "lin_user", "lin_item"):
            p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        p["gb"] = np.array([0.1], F32)
        if not case.trainable:
            p["lin_user"][...] = 0
            p["lin_item"][...] = 0
    else:                       # tests/test_gpu_parity.py::make_problem
        p = otower.init_params(rs, N_USER, N_ITEM, D)
        for l in range(3):
            p["b%d" % l] = (rs.standard_normal(p["b%d" % l].shape) * 0.05).astype(F32)
        if tower in ("deepfm", "wdl"):
            p["lin_domain"] = (rs.standard_normal(D) * 0.05).astype(F32)
            if case.trainable:
                p["lin_user"] = (rs.standard_normal(N_USER) * 0.05).astype(F32)
                p["lin_item"] = (rs.standard_normal(N_ITEM) * 0.05).astype(F32)
    p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
    if case.uncertainty:        # distinct per-domain scales around the initial value 1
        p["log_var"] = (1.0 + rs.uniform(-0.3, 0.3, D)).astype(F32)
    return p


def _columns(rs, dom):
    rows = dom.shape[0]
    return {"uid": rs.randint(0, N_USER, rows).astype(np.int32), "pid": rs.randint(0, N_ITEM, rows).astype(np.int32),
            "domain": dom.astype(np.int32), "label": (rs.uniform(size=rows) < 0.4).astype(F32)}


def make_inputs(case):
    """-> params, {"mixed": (bound-under id, columns), "one": (D - 1, columns)}, (0, evaluation columns)"""
    rs = np.random.RandomState(seed_of(case))
    D, batch = case.D, case.batch
    params = make_params(case, rs)
    ids = (np.arange(batch) % D) if D <= batch else (D - batch + np.arange(batch))
    steps = [rs.permutation(ids) for _ in range(STEPS)]
    first = int(steps[0][0])
    for s in steps[1:]:         # the bound-under id leads every batch
        k = int(np.flatnonzero(s == first)[0])
        s[0], s[k] = s[k], s[0]
    for s in steps:
        assert s[0] == first and np.array_equal(np.unique(s), np.unique(ids)) and s.max() == D - 1
    splits = {"mixed": (first, _columns(rs, np.concatenate(steps))),
              "one": (D - 1, _columns(rs, np.full(STEPS * batch, D - 1)))}
    return params, splits, (0, _columns(rs, np.zeros(EVAL_ROWS, np.int64)))


def batch_of(cols, step, batch):
    return tuple(cols[k][step * batch:(step + 1) * batch] for k in ("uid", "pid", "domain", "label"))


def deepfm_flag(case):
    return {"deepfm": 1, "wdl": 2}.get(case.tower, 0)


def names_of(case):
    if case.tower == "star":
        return sum(ostar.param_names(case.trainable), ())
    if case.tower == "pnn":
        return tuple(ofm.param_names("pnn", case.trainable, case.uncertainty))
    return otower.param_names(case.trainable, deepfm_flag(case), case.uncertainty)


def make_model(case, params):
    p = {k: v.copy() for k, v in params.items()}
    if case.tower == "star":
        return ostar.OracleStar(p, emb_trainable=case.trainable, lr=1e-3)
    if case.tower == "pnn":
        return ofm.OracleNet(p, "pnn", emb_trainable=case.trainable, dropout=0.5, lr=1e-3, hidden=HIDDEN, dropout_seed=DROPOUT_SEED,
                             **({"uncertainty": True} if case.uncertainty else {}))
    return otower.OracleModel(p, emb_trainable=case.trainable, dropout=0.5, lr=1e-3, dropout_seed=DROPOUT_SEED, tower=case.tower,
                              uncertainty=case.uncertainty)


def oracle_step(case, model, args, frozen_reg=True):
    """loss and gradients of one batch at the model's weights and dropout position (the oracle's fp32 statement).
    frozen_reg False: the loss without the frozen tables' regulariser, as oracle/torch_ref.py states it."""
    if case.tower == "star":
        loss, grads, _, c = ostar.loss_and_grads(model.params, model.state, *args, case.trainable)
        return loss, grads, c
    masks = otower.train_masks(model.seed, model.step, args[0].shape[0], HIDDEN, 0.5)
    if case.tower == "pnn":
        loss, grads, _ = ofm.loss_and_grads(model.params, "pnn", *args, masks, 0.5, case.trainable,
                                            model.frozen_sumsq() if frozen_reg else None, case.uncertainty)
    else:
        loss, grads, _ = otower.loss_and_grads(model.params, *args, masks, 0.5, case.trainable,
                                               model.frozen_sumsq() if frozen_reg else None, deepfm_flag(case), case.uncertainty)
    return loss, grads, None


def float64_step(case, model, args):
    """the same batch through float64 autograd of the independently written forward (oracle/torch_ref.py)."""
    from oracle import torch_ref as tref
    names = list(names_of(case))
    if case.tower == "star":
        loss, grads, _, _ = tref.loss_and_grads(model.params, names, *args, tower="star")
        return loss, grads
    masks = otower.train_masks(model.seed, model.step, args[0].shape[0], HIDDEN, 0.5)
    if case.tower == "pnn":
        loss, grads, _ = tref.fmnet_loss_and_grads(model.params, names, "pnn", *args, masks, 0.5, uncertainty=case.uncertainty)
    else:
        loss, grads, _, _ = tref.loss_and_grads(model.params, names, *args, masks, 0.5, case.tower, case.uncertainty)
    return loss, grads


def distinct_inputs():
    """one case per distinct set of inputs (the fused and the slab path of a count share theirs)."""
    seen, out = set(), []
    for c in CASES:
        if input_key(c) not in seen:
            seen.add(input_key(c))
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- the generic-layer engine
GRAPH_D = (1, 33)
MTL_KINDS = ("shared_bottom", "mmoe", "ple")


def synthetic_problem(D, seed, scale):
    from mamdr_amd import synthetic
    return synthetic.generate(dict(synthetic.SHAPES["taobao10"], n_domain=D), batch_size=256, seed=seed, scale=scale)


def probe_domains(g):
    """the largest domain and the one with the highest id"""
    big = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    return sorted({big, g["n_domain"] - 1})


def probe_batches(g):
    """[(domain, the first min(256, n) rows of its train split in file order)], in the order they are probed"""
    out = []
    for d in probe_domains(g):
        c = g["data"]["train"][d]
        n = min(256, c["uid"].shape[0])
        out.append((d, tuple(c[k][:n] for k in ("uid", "pid", "domain", "label"))))
    return out


def mtl_problem(kind, D, seed=7, scale=0.05):
    """tests/test_gpu_mtl.py::make_problem's problem without its engine: -> g, spec, params"""
    from keras_variables import MTL_SHAPES
    from oracle import mtl as omtl
    eh, th, gh, ne, se, sp = MTL_SHAPES[kind]
    g = synthetic_problem(D, seed, scale)
    spec = omtl.Spec(kind, D, eh, th, gh, num_experts=ne, shared_expert_num=se, specific_expert_num=sp)
    rs = np.random.RandomState(seed)
    params = omtl.init_params(rs, spec, g["n_user"], g["n_item"])
    params["user_emb"], params["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
    for n in params:
        if "/b" in n or n.endswith("/gb") or n == "domain_emb":
            params[n] = (rs.standard_normal(params[n].shape) * 0.05).astype(F32)
    return g, spec, params


def star_form_problem(D, seed=11, scale=0.2):
    """tests/test_gpu_star_forms.py::problem at D domains: -> g"""
    return synthetic_problem(D, seed, scale)
