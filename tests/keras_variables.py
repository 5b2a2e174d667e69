"""The Keras variables behind every tower's flat vector, written down once, as data (test infrastructure).

The reference's PCGrad reduces every variable along its LAST axis (model_zoo/pcgrad.py:152-160): the one outer
operation that depends on the variables' shapes and not only on the flat vector.  Three places decide those shapes in
this build -- `TowerEngine.segment_shapes`, `GraphEngine.segment_shapes` (over `add_tensor` of csrc/graph_engine.hip) and
`oracle.loops.tensor_views` -- and each is held to THIS table (tests/test_pcgrad_tables_host.py,
tests/test_gpu_pcgrad_towers.py).  The table is taken from the layer definitions, not from any of the three:

* Embedding tables                   [n, emb]                         (deepctr.py:95-102; star.py:99-110)
* DNN kernels / biases               [in, out] / [out]                (deepctr layers/core.py DNN.build)
    PNN's first kernel               [3 emb + 3, h0]                  (the inner products feed its last three rows)
    NFM's first kernel               [emb, h0]                        (BiInteractionPooling leaves one field)
    CCPM's first kernel              [4 emb, h0]                      (emb x 4 filters, flattened)
* Dense(1, use_bias=False) heads     [in, 1]                          (AutoInt: in = 3 * 32 + h_last)
* PredictionLayer global bias        [1]
* deepctr's linear tables, log_var   [n, 1]                           (Embedding(n, 1); weighted_loss.py:23-28 [D, 1])
* Star (star_fcn.py:61-96)           kernel_specific [D, in, out], bias_specific [D, out], shared [in, out] / [out]
* PartitionedNorm (:56-97)           gamma / beta specific [D, 384], shared [384];  BatchNormalization gamma / beta [384]
* AuxiliaryNet (auxiliary_net.py:61-73)   kernel [D, 384, A], bias [D, A]
* CCPM Conv2D kernels                [6, 1, 1, 4], and of [5, 1, 4, 4] the centre tap [4, 4] (the only tap that meets data:
                                     the other four never leave zero gradient and are not in the flat vector), biases [4]
* AutoInt InteractingLayer           FOUR variables [d, 32] per layer (W_Query, W_key, W_Value, W_Res), d = emb then 32.
                                     This build keeps them side by side in one tensor `att<l>_w` [d][128]; the four column
                                     blocks of a row-major [d][128] are exactly the rows of a contiguous [4 d][32], which is
                                     the shape this table gives (the same slices, each of ONE variable)
* MMOE / PLE gate kernels            [in, n_mix]                      (Dense(n_mix, use_bias=False))

`Var.offset` is the offset in the ORACLE's flat vector (tensors back to back); the engines round some starts up to 16
bytes, so against an engine the table is matched by name (`by_name`) and the engine's own offsets are checked for order
and overlap.  Flat order = the oracle modules' `names` (Keras trainable_weights order where SURVEY A.1 pins it).
"""
import collections

Var = collections.namedtuple("Var", "name shape offset")

ATT_LAYERS, ATT_OUT = 3, 32

# the small multi-task towers of the GPU tests (tests/test_gpu_mtl.py's SHAPES, tests/test_gpu_pcgrad_towers.py,
# tests/test_pcgrad_tables_host.py): the one definition
MTL_SHAPES = {
    # (expert_hidden, tower_hidden, gate_hidden, num_experts, shared_expert_num, specific_expert_num)
    "shared_bottom": ((256, 128), (64,), (), 0, 0, 0),
    "mmoe": ((128, 64), (64,), (64,), 3, 0, 0),
    "ple": ((128,), (64,), (64,), 0, 2, 2),
}


def slices(shape):
    """(number of slices along the last axis, slice length) -- what numpy's axis=-1 reductions see."""
    n = 1
    for s in shape[:-1]:
        n *= int(s)
    return n, int(shape[-1])


def size(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _with_offsets(pairs):
    out, o = [], 0
    for name, shape in pairs:
        out.append(Var(name, tuple(int(s) for s in shape), o))
        o += size(shape)
    return out


def _dnn(in_dim, hidden, w="W", b="b"):
    """deepctr's DNN: ALL kernels, then ALL biases"""
    dims = (in_dim,) + tuple(hidden)
    return ([("%s%d" % (w, l), (dims[l], dims[l + 1])) for l in range(len(hidden))]
            + [("%s%d" % (b, l), (dims[l + 1],)) for l in range(len(hidden))])


def deepctr(kind, n_user, n_item, n_domain, emb_dim=128, hidden=(256, 128, 64), emb_trainable=False, uncertainty=False):
    """mlp / wdl / deepfm (oracle/tower.py), nfm / pnn / ccpm / autoint (oracle/fmnets.py)"""
    E, D = emb_dim, n_domain
    linear = kind in ("wdl", "deepfm", "nfm", "ccpm", "autoint")
    v = []
    if emb_trainable:
        v += [("user_emb", (n_user, E)), ("item_emb", (n_item, E))]
        if linear:
            v += [("lin_user", (n_user, 1)), ("lin_item", (n_item, 1))]
    v.append(("domain_emb", (D, E)))
    if kind == "ccpm":
        v += [("conv1_w", (6, 1, 1, 4)), ("conv1_b", (4,)), ("conv2_w", (4, 4)), ("conv2_b", (4,))]
    if kind == "autoint":
        d = E
        for l in range(ATT_LAYERS):
            v.append(("att%d_w" % l, (4 * d, ATT_OUT)))
            d = ATT_OUT
    in_dim = {"nfm": E, "pnn": 3 * E + 3, "ccpm": 4 * E}.get(kind, 3 * E)
    v += _dnn(in_dim, hidden)
    v += [("wo", ((3 * ATT_OUT if kind == "autoint" else 0) + hidden[-1], 1)), ("gb", (1,))]
    if linear:
        v.append(("lin_domain", (D, 1)))
    if uncertainty:
        v.append(("log_var", (D, 1)))
    return _with_offsets(v)


def star(n_user, n_item, n_domain, emb_dim=128, hidden=(256, 128, 64), emb_trainable=False, norm="pn", dense="star",
         auxiliary_dim=0):
    """every Star form (oracle/star.py = norm "pn", dense "star", no auxiliary net; tests/star_forms_ref.py)"""
    E, D, X = emb_dim, n_domain, 3 * emb_dim
    v = []
    if emb_trainable:
        v += [("user_emb", (n_user, E)), ("item_emb", (n_item, E))]
    v.append(("domain_emb", (D, E)))
    v += _dnn(X, hidden, *(("Ws", "bs") if dense == "star" else ("W", "b")))
    if norm == "pn":
        v += [("pn_gamma_shared", (X,)), ("pn_beta_shared", (X,)), ("pn_gamma_spec", (D, X)), ("pn_beta_spec", (D, X))]
    elif norm == "bn":
        v += [("bn_gamma", (X,)), ("bn_beta", (X,))]
    if dense == "star":
        dims = (X,) + tuple(hidden)
        v += [("Wd%d" % l, (D, dims[l], dims[l + 1])) for l in range(len(hidden))]
        v += [("bd%d" % l, (D, dims[l + 1])) for l in range(len(hidden))]
    v += [("wo", (hidden[-1], 1)), ("gb", (1,))]
    if auxiliary_dim:
        v += [("aux_W", (D, X, auxiliary_dim)), ("aux_b", (D, auxiliary_dim))]
    return _with_offsets(v)


def mtl(kind, n_user, n_item, n_domain, expert_hidden, tower_hidden, gate_hidden=(), num_experts=0, shared_expert_num=0,
        specific_expert_num=0, emb_dim=128, emb_trainable=False):
    """shared_bottom / mmoe / ple (oracle/mtl.py: the shared block, then one block per task; kernel and bias of a DNN
    layer next to each other)"""
    E, D, X = emb_dim, n_domain, 3 * emb_dim

    def dnn(name, in_dim, hidden):
        out, i = [], in_dim
        for l, h in enumerate(hidden):
            out += [("%s/W%d" % (name, l), (i, h)), ("%s/b%d" % (name, l), (h,))]
            i = h
        return out

    shared = {"shared_bottom": ["bottom"], "mmoe": ["expert_%d" % e for e in range(num_experts)],
              "ple": ["shared_expert_%d" % e for e in range(shared_expert_num)]}[kind]
    v = []
    if emb_trainable:
        v += [("user_emb", (n_user, E)), ("item_emb", (n_item, E))]
    v.append(("domain_emb", (D, E)))
    for e in shared:
        v += dnn(e, X, expert_hidden)
    for d in range(D):
        own = ["task_%d_expert_%d" % (d, e) for e in range(specific_expert_num)] if kind == "ple" else []
        for e in own:
            v += dnn(e, X, expert_hidden)
        if kind != "shared_bottom":
            v += dnn("gate_%d" % d, X, gate_hidden)
            v.append(("gate_%d/Wg" % d, (gate_hidden[-1] if gate_hidden else X, len(own) + len(shared))))
        v += dnn("tower_%d" % d, expert_hidden[-1], tower_hidden)
        v += [("head_%d/w" % d, (tower_hidden[-1], 1)), ("head_%d/gb" % d, (1,))]
    return _with_offsets(v)


def by_name(table):
    return collections.OrderedDict((t.name, t) for t in table)


def engine_slices(table, segments):
    """{tensor: (slices, slice length)} the table asks of an engine with these `segments` ({name: (offset, count)}).
    The step engine keeps the inner products' three rows of PNN's first kernel [387, 256] as a segment `W0x` of its
    own behind the rest: rows of one variable either way."""
    out = collections.OrderedDict()
    for t in table:
        rows, cols = slices(t.shape)
        if t.name == "W0" and "W0x" in segments:
            out["W0"], out["W0x"] = (rows - 3, cols), (3, cols)
        else:
            out[t.name] = (rows, cols)
    return out


def views(table, flat, offsets=None):
    """per-variable numpy views of a flat vector in the table's shapes; offsets: {name: offset} of an engine's vector
    (default: the table's own back-to-back offsets).  A variable an engine keeps in two segments (PNN's W0 / W0x) is given
    through `engine_views`."""
    out = []
    for t in table:
        o = t.offset if offsets is None else offsets[t.name]
        out.append(flat[o:o + size(t.shape)].reshape(t.shape))
    return out


def engine_views(table, flat, segments):
    """[(name, view)] of an engine's flat vector: one view per SEGMENT, shaped [slices, slice length] by the table."""
    out = []
    for name, (rows, cols) in engine_slices(table, segments).items():
        off, cnt = segments[name]
        assert cnt == rows * cols, (name, cnt, rows, cols)
        out.append((name, flat[off:off + cnt].reshape(rows, cols)))
    return out
