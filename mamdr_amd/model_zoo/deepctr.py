"""DeepCTR tower -- host-side mirror of model_zoo/DeepCTR/deepctr.py.

`build_model` keeps the reference's substring registry (deepctr.py:24-50): names
containing `mlp` build the 3 x 128-d embedding -> DNN(hidden_dim) -> Dense(1) -> sigmoid
tower (deepctr.py:95-136) on the HIP engine; names containing `deepfm` add the linear
tables and the FM second-order term to the logit (deepctr.py:36-38);
`wdl` is the same without the FM term (deepctr.py:29-32); `nfm` (deepctr.py:33-35: linear tables + DNN over the
bi-interaction of the three fields) and `pnn` (deepctr.py:44-46: DNN over the fields and their pairwise inner
products) and `ccpm` (deepctr.py:41-43: convolutions over the field axis) run on the generic-layer engine
(`GraphEngine`, csrc/graph_engine.hip), and so does `autoint` (deepctr.py:37-40: three multi-head self-attention
layers over the fields beside the DNN).  `route` is the one place that decides which engine a config runs on -- for this
model, Star and DeepMTLCTR -- and `build_model` is route, construct, draw the initial tensors, bind.  Initial tensors follow the reference's initialisers (glorot normal for the
kernels, zeros for biases, N(0, 1e-4^2) for the domain table and for user/item tables
without pretraining, constants from the pretrained tables otherwise) drawn from a numpy
stream seeded with dataset.seed -- TF's own streams are not reproducible.
"""
import collections
import os
import random

import numpy as np

from .base_model import BaseModel

GRAPH_TOWERS = ("nfm", "pnn", "ccpm", "autoint")
MTL_KINDS = ("shared_bottom", "mmoe", "ple")
REFERENCE_HIDDEN = (256, 128, 64)
# embedding widths (user_dim == item_dim == domain_dim) of the mlp / wdl / deepfm towers: the step kernels are built for
# 128, the generic-layer engine's gather / FM / table kernels for these (mamdr_graph_create checks the same set)
EMB_WIDTHS = (32, 64, 128, 256)


def check_emb_width(tower, emb_dim, any_width):
    """the width limit of a tower that runs on a HIP engine: NotImplementedError for a tower whose kernels know 128 only,
    ValueError for a width outside EMB_WIDTHS."""
    if emb_dim == 128:
        return
    if not any_width:
        raise NotImplementedError("user_dim %r: the '%s' tower is built for 128-wide embeddings only (mlp / wdl / deepfm "
                                  "take user_dim in %r)" % (emb_dim, tower, EMB_WIDTHS))
    if emb_dim not in EMB_WIDTHS:
        raise ValueError("user_dim %r: the '%s' tower takes an embedding width in %r" % (emb_dim, tower, EMB_WIDTHS))


# engine: "step" (engine.TowerEngine) or "graph" (graph_engine.GraphEngine); kind: the tower / kind the engine is built as;
# args, kwargs: the constructor call's leading positional argument and the keyword arguments the config decides; offer: the
# attribute of an injected factory that serves the route (None: the factory itself -- TowerEngine-style for a step route,
# GraphEngine-style for the multi-task kinds)
Route = collections.namedtuple("Route", "engine kind args kwargs offer")


def route(tower, mc, batch_size, factory, environ, star_form=None):
    """Which engine a config runs on, and how it is constructed -- every such decision, once.

    tower: the registry's name (DeepCTR / Star / DeepMTLCTR.tower_kind); mc: model_config; factory: None (the HIP
    engines) or the injected factory, whose `graph` / `star_graph` attributes say what it offers beside the step-style
    call; star_form: Star's {norm, dense, auxiliary_dim, plain}.

        shared_bottom / mmoe / ple                          graph
        ccpm / autoint                                      graph
        pnn / nfm                                           step at hidden_dim [256, 128, 64], width 128 and batches of up to
                                                            2,048 rows (every reference config); graph beyond either limit,
                                                            under MAMDR_PNN_ENGINE=graph / MAMDR_NFM_ENGINE=graph (the parity
                                                            twins, one switch per tower) and on an injected factory
        mlp / wdl / deepfm                                  step at [256, 128, 64] and width 128, else graph (1 - 4 layers of
                                                            multiples of 64, a width of EMB_WIDTHS); an injected factory is
                                                            always called step-style, with `hidden=` and `emb_dim=`
        star, plain form (norm none, dense dense, no aux)   as mlp, without dropout and regularisers
        star, pn + star, no aux, [256, 128, 64]             step; MAMDR_STAR_ENGINE=graph: graph (the parity twin)
        star, every other form                              graph -- where the factory offers it, else what Star raised
    """
    E, hidden, injected = mc["user_dim"], tuple(mc["hidden_dim"]), factory is not None
    if not (mc["user_dim"] == mc["item_dim"] == mc["domain_dim"]):
        raise ValueError("user_dim, item_dim and domain_dim must be equal")
    if tower in MTL_KINDS:                  # deep_mtl_ctr.py:25-49
        if tower == "ple" and mc.get("num_levels", 1) != 1:
            raise NotImplementedError("ple with num_levels = %r: the reference's configs all use one level" % mc.get("num_levels"))
        if not injected:
            check_emb_width(tower, E, False)
        gate = tuple(mc.get("gate_dnn_hidden_units", ())) if tower != "shared_bottom" else ()
        return Route("graph", tower, (tower,), dict(
            dropout=mc.get("dropout", 0.0), emb_dim=E, expert_hidden=hidden, tower_hidden=tuple(mc["tower_hidden_dim"]),
            gate_hidden=gate, num_experts=int(mc.get("num_experts", 0)), shared_expert_num=int(mc.get("shared_expert_num", 0)),
            specific_expert_num=int(mc.get("specific_expert_num", 0))), None)
    kw = dict(dropout=mc.get("dropout", 0.0), emb_dim=E)
    if star_form is not None:               # star.py:74-95 attaches no regulariser to any layer and builds no Dropout layer
        kw["dropout"] = 0.0
        if star_form["plain"]:
            tower = "mlp"
            kw.update(l2_emb=0.0, l2_linear=0.0)
    if "uncertainty_weight" in mc["name"]:     # run.py:49-50: the weighted loss joins the compiled model
        kw["uncertainty_weight"] = True
    if not 1 <= len(hidden) <= 4:
        raise ValueError("hidden_dim %r: the '%s' tower takes 1 to 4 hidden layers" % (mc["hidden_dim"], tower))
    reference_shape = hidden == REFERENCE_HIDDEN and E == 128
    any_width = False
    if tower == "star":
        step_form = (star_form["norm"], star_form["dense"], star_form["auxiliary_dim"], hidden) == ("pn", "star", 0, REFERENCE_HIDDEN)
        graph = (not injected or hasattr(factory, "star_graph")) and not (
            step_form and environ.get("MAMDR_STAR_ENGINE", "step") != "graph")
        if graph:
            kw.update(norm=star_form["norm"], dense=star_form["dense"], auxiliary_dim=star_form["auxiliary_dim"])
        elif len(hidden) != 3:
            raise ValueError("hidden_dim %r: the Star tower's kernels are built for three hidden layers (the reference's "
                             "configs all have [256, 128, 64])" % (mc["hidden_dim"],))
    elif tower == "pnn":
        graph = injected or batch_size > 2048 or not reference_shape or environ.get("MAMDR_PNN_ENGINE", "step") == "graph"
    elif tower == "nfm":
        graph = injected or batch_size > 2048 or not reference_shape or environ.get("MAMDR_NFM_ENGINE", "step") == "graph"
    elif tower in GRAPH_TOWERS:
        graph = True
    else:                                   # mlp / wdl / deepfm
        graph, any_width = not reference_shape and not injected, True
    if not injected:                        # (an injected factory -- the tests' CPU stand-in -- takes any width and shape)
        check_emb_width(tower, E, any_width)
        if graph and tower not in GRAPH_TOWERS and any(h <= 0 or h % 64 for h in hidden):
            raise ValueError("hidden_dim %r: layer widths must be multiples of 64" % (mc["hidden_dim"],))
    elif graph and tower in GRAPH_TOWERS and getattr(factory, "graph", None) is None:
        raise NotImplementedError("the injected engine factory has no '%s' tower" % tower)
    if graph:
        return Route("graph", tower, (tower,), dict(kw, expert_hidden=hidden, tower_hidden=()),
                     "star_graph" if tower == "star" else "graph")
    return Route("step", tower, (), dict(kw, tower=tower, hidden=hidden), None)


def truncated_normal(rs, shape):
    """standard normal draws, redrawn where they lie beyond 2 sigma (Keras' TruncatedNormal)."""
    x = rs.standard_normal(shape)
    bad = np.abs(x) > 2.0
    while bad.any():
        x[bad] = rs.standard_normal(int(bad.sum()))
        bad = np.abs(x) > 2.0
    return x


def glorot_normal(rs, fan_in, fan_out, shape):
    """Keras glorot_normal: truncated normal (2 sigma), stddev = sqrt(2 / (fan_in + fan_out))."""
    return (truncated_normal(rs, shape) * np.sqrt(2.0 / (fan_in + fan_out))).astype(np.float32)


def initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, user_emb=None, item_emb=None):
    """every initializer of the model, in layer order (what `init_layer` re-runs,
    specific_base_model.py:174-178)."""
    t = {}
    t["user_emb"] = user_emb if user_emb is not None else (rs.standard_normal((n_user, emb_dim)) * 1e-4).astype(np.float32)
    t["item_emb"] = item_emb if item_emb is not None else (rs.standard_normal((n_item, emb_dim)) * 1e-4).astype(np.float32)
    t["domain_emb"] = (rs.standard_normal((n_domain, emb_dim)) * 1e-4).astype(np.float32)
    dims = (3 * emb_dim,) + tuple(hidden)
    for l in range(len(hidden)):          # (the step kernels take exactly three layers; the generic-layer towers 1 - 4)
        t["W%d" % l] = glorot_normal(rs, dims[l], dims[l + 1], (dims[l], dims[l + 1]))
        t["b%d" % l] = np.zeros(dims[l + 1], np.float32)
    t["wo"] = glorot_normal(rs, dims[-1], 1, (dims[-1], 1))
    t["gb"] = np.zeros(1, np.float32)
    # DeepFM 1-d linear tables: Zeros initialiser (deepctr get_linear_logit); unused by the mlp tower
    t["lin_user"] = np.zeros(n_user, np.float32)
    t["lin_item"] = np.zeros(n_item, np.float32)
    t["lin_domain"] = np.zeros(n_domain, np.float32)
    # uncertainty weighting: `log_var` [D], Constant(1.) (uncertainty_weight/weighted_loss.py:23-28)
    t["log_var"] = np.ones(n_domain, np.float32)
    return t


class DeepCTR(BaseModel):
    def __init__(self, dataset, config, engine_factory=None):
        super(DeepCTR, self).__init__(dataset, config, engine_factory)

    def tower_kind(self):
        name = self.model_config["name"]
        if "mlp" in name:
            tower = "mlp"
        elif "wdl" in name:               # deepctr.py:29-32: linear tables + DNN (DeepFM without the FM term)
            tower = "wdl"
        elif "nfm" in name:               # deepctr.py:33-35
            tower = "nfm"
        elif "autoint" in name:           # deepctr.py:37-40
            tower = "autoint"
        elif "ccpm" in name:              # deepctr.py:41-43
            tower = "ccpm"
        elif "pnn" in name:               # deepctr.py:44-46
            tower = "pnn"
        elif "deepfm" in name:
            tower = "deepfm"
        else:
            raise ValueError("model: {} not found".format(name))
        return tower

    def star_form(self):
        """Star: {norm, dense, auxiliary_dim, plain} of the config; None for every other model."""
        return None

    def build_model(self):
        """route, construct, draw the initial tensors, bind."""
        self.pretrained = self.pretrained_tables()
        self.form = self.star_form()
        r = self.route = route(self.tower_kind(), self.model_config, self.batch_size, self.engine_factory, os.environ, self.form)
        self.tower = r.kind
        eng = self.construct_engine(r)
        self.init_rs = np.random.RandomState(self.dataset.seed)
        return self.bind_engine(eng, self.draw_initial_tensors(), "on the hot path")

    def draw_initial_tensors(self):
        mc = self.model_config
        t = initial_tensors(self.init_rs, self.n_uid, self.n_pid, self.n_domain, mc["user_dim"],
                            tuple(mc["hidden_dim"]), self.pretrained[0], self.pretrained[1])
        tower = self.tower
        if tower in GRAPH_TOWERS:         # first kernel: NFM on the 128 interaction columns, PNN on the fields + 3 inner products,
            E, h0 = mc["user_dim"], mc["hidden_dim"][0]       # CCPM on the [128 x 4] convolution features
            in_dim = {"nfm": E, "pnn": 3 * E + 3, "ccpm": 4 * E, "autoint": 3 * E}[tower]
            t["W0"] = glorot_normal(self.init_rs, in_dim, h0, (in_dim, h0))
            if tower == "autoint":        # InteractingLayer: W_Query | W_key | W_Value | W_Res, TruncatedNormal(stddev 0.05) each
                d_in = E
                for l in range(3):
                    t["att%d_w" % l] = (truncated_normal(self.init_rs, (d_in, 128)) * 0.05).astype(np.float32)
                    d_in = 32
                h_last = mc["hidden_dim"][-1]
                t["wo"] = glorot_normal(self.init_rs, 96 + h_last, 1, (96 + h_last, 1))
            if tower == "ccpm":           # Keras Conv2D defaults: glorot_uniform kernels [6,1,1,4] / [5,1,4,4] (centre tap kept), zero biases
                lim1, lim2 = np.sqrt(6.0 / (6 * 1 + 6 * 4)), np.sqrt(6.0 / (5 * 4 + 5 * 4))
                t["conv1_w"] = self.init_rs.uniform(-lim1, lim1, (6, 4)).astype(np.float32)
                t["conv1_b"] = np.zeros(4, np.float32)
                t["conv2_w"] = self.init_rs.uniform(-lim2, lim2, (4, 4)).astype(np.float32)
                t["conv2_b"] = np.zeros(4, np.float32)
        return t

    def train(self):
        """alternate ('joint') training, deepctr.py:63-93."""
        self.model.optimizer_reset()
        train_sequence = list(range(self.n_domain))
        rng = random.Random(self.dataset.seed)
        for epoch in range(self.train_config["epoch"]):
            print("Epoch: {}".format(epoch), "-" * 30)
            rng.shuffle(train_sequence)
            for idx in train_sequence:
                self.fit_domain(idx, phase="alt")
            print("Val Result: ")
            avg_loss, avg_auc, domain_loss, domain_auc = self.val_and_test("val")
            if self.early_stop_step(avg_auc):
                break
            print("Test Result: ")
            # as in the reference, this reloads the best checkpoint into the live model
            self.val_and_test("test")
