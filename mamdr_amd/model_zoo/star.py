"""Star tower -- host-side mirror of model_zoo/Star/star.py.

Structure (star.py:70-97): 3 x 128-d embeddings -> norm (`none`, PartitionedNorm `pn`, BatchNormalization `bn`) -> one
hidden layer per width (`dense: "star"` StarFCN, `dense: "dense"` Keras Dense) -> [+ the AuxiliaryNet's output when
`auxiliary_net` is true] -> Dense(1, sigmoid).  Which engine runs which member of the family:

    pn + star, no auxiliary net, hidden_dim [256, 128, 64]    the step kernels, `TowerEngine(tower="star")`
                                                              (MAMDR_STAR_ENGINE=graph: the generic-layer engine, its parity twin)
    none + dense, no auxiliary net                            the mlp tower without dropout / regularisers, Keras initial values
                                                              and variable names (`dense/kernel` ...), on the mlp engines
    everything else: bn, the mixed forms, auxiliary_net,      `GraphEngine("star", norm=, dense=, auxiliary_dim=)`
    1 - 4 hidden layers of multiples of 64                    (csrc/graph_engine.hip, MAMDR_GRAPH_STAR)

`Star.star_form` reads and checks these keys once per build; `deepctr.route` picks the engine from the form.
`auxiliary_net: true` needs `auxiliary_dim == hidden_dim[-1]` (Keras' Add).  `bn` keeps one pair of moving statistics whose
shape the several-process / several-lane synchronisation does not know: it raises there.  An injected engine factory (the
tests' CPU stand-ins) gets the generic-layer forms only if it offers them as `factory.star_graph`.  The
plain `star` name trains with the same alternate loop as DeepCTR (star.py:34-69 == deepctr.py:63-93).
Initial tensors follow the Keras defaults of the reference's layers: Embedding uniform(-0.05, 0.05)
unless pretrained (star.py:113-127), glorot-uniform kernels (fans of the 3-d specific kernel include
the domain axis, as Keras computes them), zero biases, gamma one / beta zero; no regularisers, no
dropout.  Numerics: `TowerEngine(tower="star")` (csrc/star_kernels.hip).
"""
import functools

import numpy as np

from ..engine import keras_name
from .deepctr import DeepCTR


def glorot_uniform(rs, shape, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rs.uniform(-lim, lim, size=shape).astype(np.float32)


def initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, user_emb=None, item_emb=None):
    """the step kernels' form: PartitionedNorm + StarFCN, no auxiliary network."""
    return forms_initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, "pn", "star", 0, user_emb, item_emb)


def dense_initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, user_emb=None, item_emb=None):
    """star.py:84-86,95 with `dense: "dense"`: Keras Dense layers (glorot-uniform kernels, zero biases) on the concatenated
    embeddings, Dense(1, sigmoid) on top -- in the mlp tower's segment names (the output unit's kernel / bias = wo / gb)."""
    return forms_initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, "none", "dense", 0, user_emb, item_emb)


def forms_initial_tensors(rs, n_user, n_item, n_domain, emb_dim, hidden, norm, dense, auxiliary_dim, user_emb=None,
                          item_emb=None):
    """Keras defaults of every member of the family, drawn in `initial_tensors`' order (the pn + star form without the
    auxiliary network at three layers draws exactly its values): glorot-uniform kernels -- the 3-d specific ones and
    `aux_W` with the fans Keras computes from the 3-d shape --, zero biases, gamma one, beta zero."""
    t = {}
    t["user_emb"] = user_emb if user_emb is not None else rs.uniform(-0.05, 0.05, (n_user, emb_dim)).astype(np.float32)
    t["item_emb"] = item_emb if item_emb is not None else rs.uniform(-0.05, 0.05, (n_item, emb_dim)).astype(np.float32)
    t["domain_emb"] = rs.uniform(-0.05, 0.05, (n_domain, emb_dim)).astype(np.float32)
    dims = (3 * emb_dim,) + tuple(hidden)
    if norm == "pn":
        t["pn_gamma_shared"] = np.ones(dims[0], np.float32)
        t["pn_beta_shared"] = np.zeros(dims[0], np.float32)
        t["pn_gamma_spec"] = np.ones((n_domain, dims[0]), np.float32)
        t["pn_beta_spec"] = np.zeros((n_domain, dims[0]), np.float32)
    elif norm == "bn":
        t["bn_gamma"] = np.ones(dims[0], np.float32)
        t["bn_beta"] = np.zeros(dims[0], np.float32)
    for l in range(len(hidden)):
        if dense == "star":
            t["Wd%d" % l] = glorot_uniform(rs, (n_domain, dims[l], dims[l + 1]), dims[l] * n_domain, dims[l + 1] * n_domain)
            t["bd%d" % l] = np.zeros((n_domain, dims[l + 1]), np.float32)
            t["Ws%d" % l] = glorot_uniform(rs, (dims[l], dims[l + 1]), dims[l], dims[l + 1])
            t["bs%d" % l] = np.zeros(dims[l + 1], np.float32)
        else:
            t["W%d" % l] = glorot_uniform(rs, (dims[l], dims[l + 1]), dims[l], dims[l + 1])
            t["b%d" % l] = np.zeros(dims[l + 1], np.float32)
    t["wo"] = glorot_uniform(rs, (dims[-1], 1), dims[-1], 1)
    t["gb"] = np.zeros(1, np.float32)
    if auxiliary_dim:
        A = int(auxiliary_dim)
        t["aux_W"] = glorot_uniform(rs, (n_domain, dims[0], A), dims[0] * n_domain, A * n_domain)
        t["aux_b"] = np.zeros((n_domain, A), np.float32)
    return t


class Star(DeepCTR):
    NORMS, DENSES = ("none", "pn", "bn"), ("dense", "star")

    def tower_kind(self):
        return "star"

    def star_form(self):
        """{norm, dense, auxiliary_dim, plain} of the config, checked against what the engines (or the injected factory's
        `star_graph`) build: the one place that reads the family's keys."""
        mc = self.model_config
        norm, dense, aux = mc.get("norm"), mc.get("dense"), bool(mc.get("auxiliary_net"))
        offered = self.engine_factory is None or hasattr(self.engine_factory, "star_graph")
        if aux:
            if not offered:
                raise NotImplementedError("auxiliary_net (model_zoo/Star/auxiliary_net.py) is not built")
            if mc.get("auxiliary_dim") != mc["hidden_dim"][-1]:
                raise ValueError("auxiliary_net: auxiliary_dim %r != hidden_dim[-1] %r (star.py:92-93 adds the two outputs)"
                                 % (mc.get("auxiliary_dim"), mc["hidden_dim"][-1]))
        plain = norm == "none" and dense == "dense" and not aux
        if not plain and (norm != "pn" or dense != "star"):
            if not offered:
                raise NotImplementedError("Star with norm=%r dense=%r: built are the PartitionedNorm + StarFCN form of the BASELINE "
                                          "configs and the plain form (norm none, dense dense)" % (norm, dense))
            if norm not in self.NORMS or dense not in self.DENSES:
                raise ValueError("Star with norm=%r dense=%r: norm is one of %r, dense one of %r"
                                 % (norm, dense, self.NORMS, self.DENSES))
            from .. import parallel
            if norm == "bn" and parallel.world()[1] > 1:
                raise NotImplementedError("Star with norm 'bn' under several processes or lanes: BatchNormalization keeps ONE pair "
                                          "of moving statistics [384], not the per-domain state the tail synchronisation "
                                          "of parallel.py combines")
        return dict(norm=norm, dense=dense, auxiliary_dim=int(mc["auxiliary_dim"]) if aux else 0, plain=plain)

    def build_model(self):
        eng = super(Star, self).build_model()
        if self.form["plain"]:
            # Keras names of star.py's layers (for the substring filters of maml.py:153-179) on whichever mlp engine runs
            # the form: Embedding layers named after their attribute, Dense layers numbered in creation order
            # (set on the instance: an injected factory's engine has a keras_name of its own)
            eng.keras_name = functools.partial(keras_name, "star", "dense", eng.segments)
        return eng

    def draw_initial_tensors(self):
        mc, f = self.model_config, self.form
        return forms_initial_tensors(self.init_rs, self.n_uid, self.n_pid, self.n_domain, mc["user_dim"], tuple(mc["hidden_dim"]),
                                     f["norm"], f["dense"], f["auxiliary_dim"], self.pretrained[0], self.pretrained[1])
