"""Device-resident multi-task tower (shared_bottom / mmoe / ple): the stand-in for the D compiled Keras models of
model_zoo/DeepMTLCTR/deep_mtl_ctr.py:51-67 over the `mamdr_graph_*` entry points of libmamdr_hip.so.

Same surface as `TowerEngine` where the reference's DeepMTLCTR uses the Keras models:

    domain_model_dict[d].fit(...)       -> train_steps(d, ...)      (deep_mtl_ctr.py:79-80,166-172)
    domain_model_dict[d].evaluate(...)  -> evaluate(d, split)       (deep_mtl_ctr.py:207)
    model.get_weights / set_weights     -> get_weights / set_weights (deep_mtl_ctr.py:146,158,192)

What the two engines do alike over their two entry-point families lives in `engine.DeviceEngine`; here are the graph's
description (`GraphConfig`, the tensor table with its shapes), the per-task ranges, the Keras Adam epsilon of the
separate runs and BatchNormalization's aux layout.  torch is the device allocator / stream provider only.  No CPU
fallback exists.
"""
import ctypes as C

from . import _lib as L
from .engine import DeviceEngine, _ptr, keras_names

KINDS = {"shared_bottom": L.GRAPH_SHARED_BOTTOM, "mmoe": L.GRAPH_MMOE, "ple": L.GRAPH_PLE, "nfm": L.GRAPH_NFM, "pnn": L.GRAPH_PNN,
         "ccpm": L.GRAPH_CCPM, "autoint": L.GRAPH_AUTOINT, "mlp": L.GRAPH_MLP, "wdl": L.GRAPH_WDL, "deepfm": L.GRAPH_DEEPFM,
         "star": L.GRAPH_STAR}


def star_keras_names(segments, dense):
    """{tensor: Keras variable name} of a Star form (engine.keras_names)."""
    return keras_names("star", dense, segments)


def _arr4(values):
    v = list(values) + [0] * (4 - len(values))
    return (C.c_int32 * 4)(*v)


class GraphEngine(DeviceEngine):
    PREFIX, GRAPH = "mamdr_graph_", True

    def __init__(self, kind, n_user, n_item, n_domain, batch_size, expert_hidden, tower_hidden, gate_hidden=(),
                 num_experts=0, shared_expert_num=0, specific_expert_num=0, dropout=0.5, emb_trainable=False, emb_dim=128,
                 l2_emb=1e-5, device=None, dropout_seed=1024, l2_linear=1e-5, uncertainty_weight=False,
                 adam_beta1=0.9, adam_beta2=0.999, norm="pn", dense="star", auxiliary_dim=0):
        """kind "star" (star.py:70-96): norm "none" / "pn" / "bn", dense "dense" / "star", auxiliary_dim 0 (no auxiliary
        network) or the last hidden width; every other kind ignores the three."""
        self._open(device, n_user, n_item, n_domain, batch_size, dropout_seed, emb_trainable)
        if len(expert_hidden) > 4 or len(tower_hidden) > 4 or len(gate_hidden) > 4:
            raise ValueError("at most 4 hidden layers per DNN")
        self.kind, self.emb_dim = kind, int(emb_dim)
        self.norm, self.dense, self.auxiliary_dim = (norm, dense, int(auxiliary_dim)) if kind == "star" else ("none", "dense", 0)
        if kind == "star" and (norm not in L.STAR_NORMS or dense not in L.STAR_DENSES):
            raise ValueError("Star: norm %r / dense %r (norm none, pn or bn; dense dense or star)" % (norm, dense))
        max_batch = (self.batch_size + 63) // 64 * 64
        self.eval_batch = self.batch_size
        cfg = L.GraphConfig(L.ABI_VERSION, KINDS[kind], self.n_user, self.n_item, self.n_domain, emb_dim, max_batch,
                            1 if emb_trainable else 0, len(expert_hidden), _arr4(expert_hidden), len(tower_hidden),
                            _arr4(tower_hidden), len(gate_hidden), _arr4(gate_hidden), int(num_experts),
                            int(shared_expert_num), int(specific_expert_num), float(dropout), float(l2_emb), float(adam_beta1),
                            float(adam_beta2), 1e-8,
                            float(l2_linear), 1 if uncertainty_weight else 0,
                            L.STAR_NORMS[self.norm], L.STAR_DENSES[self.dense], self.auxiliary_dim)
        handle = C.c_void_p()
        self._check(self.lib.mamdr_graph_create(C.byref(cfg), C.c_void_p(self.stream.cuda_stream), C.byref(handle)))
        self.ctx = handle
        self.n_params = int(self.lib.mamdr_graph_param_count(self.ctx))
        self.n_meta = self.n_params
        self.segments, self.shapes = {}, {}
        buf = C.create_string_buffer(128)
        for i in range(int(self.lib.mamdr_graph_tensor_count(self.ctx))):
            off, rows, cols = C.c_int64(), C.c_int64(), C.c_int64()
            self._check(self.lib.mamdr_graph_tensor_info(self.ctx, i, buf, 128, C.byref(off), C.byref(rows), C.byref(cols)))
            name = buf.value.decode()
            self.segments[name] = (off.value, rows.value * cols.value)
            self.shapes[name] = (rows.value, cols.value)
        # non-trainable state of the Star forms' norm layer: PartitionedNorm's moving statistics in TowerEngine's layout
        # (mean 0 / variance 1 per domain, biased accumulators, steps), BatchNormalization's one pair (zeros / ones)
        self._bind_buffers(self.n_domain * 384 if self.norm == "pn" else 384)

    def bind_aux(self, aux):
        self._check(self.lib.mamdr_graph_bind_aux(self.ctx, _ptr(aux)))

    def keras_key(self):
        return self.kind, self.dense, self.segments

    def aux_state(self):
        """Star forms: the norm layer's moving statistics as numpy -- pn: as TowerEngine.aux_state; bn: {mov_mean, mov_var} [384]."""
        if self.norm == "bn" and self.aux is not None:
            h = self.aux.cpu().numpy()
            return {"mov_mean": h[0:384].copy(), "mov_var": h[384:768].copy()}
        return DeviceEngine.aux_state(self)

    def set_weights(self, vec):
        dst = self.meta_weights if (self.meta_off and vec.numel() == self.n_meta) else self._weights[:vec.numel()]
        dst.copy_(vec)

    def get_weights(self, out=None):
        if out is None:
            return self._weights.clone()
        out.copy_(self._weights)
        return out

    def segment_shapes(self):
        """{tensor: (slices along the last axis, slice length)} of the Keras variables behind the tensors -- what numpy's
        axis=-1 reductions in the reference's PCGrad see (model_zoo/pcgrad.py:152-160): rows of a kernel / table, a bias
        as one slice, the Dense(1) head kernels and deepctr's 1-d linear tables ([n, 1]) as n slices of one element.
        AutoInt's `att<l>_w` [d][128] holds FOUR Keras variables [d, 32] side by side (W_query | W_key | W_value | W_res):
        the reference reduces over the 32 columns of one of them, and the four column blocks of a row-major [d][128] are
        the rows of a contiguous [4 d][32]."""
        out = {}
        for name, (rows, cols) in self.shapes.items():
            cnt = rows * cols
            if name.startswith("lin_") or name.endswith("/w") or name in ("wo", "gb") or name.endswith("/gb"):
                out[name] = (cnt, 1)
            elif self.kind == "autoint" and name.startswith("att") and name.endswith("_w"):
                out[name] = (rows * 4, cols // 4)
            else:
                out[name] = (rows, cols)
        return out

    def task_ranges(self, domain):
        """[(offset, count)] of the flat vector a step on `domain` trains (Model(inputs, outputs[domain]).trainable_weights)."""
        v = [C.c_int64() for _ in range(4)]
        self._check(self.lib.mamdr_graph_task_ranges(self.ctx, int(domain), *[C.byref(x) for x in v]))
        return [(v[0].value, v[1].value), (v[2].value, v[3].value)]

    # retrieval: the single-output kinds go through DeviceEngine's calls (mamdr_graph_recommend ...); the kinds with one task
    # per domain and the Star forms stay refused, by `self.kind` alone and before anything else is touched
    REFUSED_RETRIEVAL = ("shared_bottom", "mmoe", "ple", "star")
    # mlp / wdl / deepfm also exist on the step engine, and an engine object of these kinds has always refused retrieval by
    # name: it keeps doing so until `enable_retrieval()` is called on it (BaseModel.construct_engine calls it for every
    # engine it builds, so `model.recommend` ... serve these kinds; code that holds a bare engine opts in itself)
    OPT_IN_RETRIEVAL = ("mlp", "wdl", "deepfm")

    def enable_retrieval(self):
        """let an mlp / wdl / deepfm engine serve recommend / recommend_domain / rank_domain / rank_slates (the other
        single-output kinds serve them as they are; the multi-task kinds and star stay refused whatever is called)."""
        self._retrieval = True

    def _refuse_retrieval(self, name, served):
        opt_in = self.kind in self.OPT_IN_RETRIEVAL and not getattr(self, "_retrieval", False)
        if self.kind in self.REFUSED_RETRIEVAL or opt_in:
            raise NotImplementedError("%s: the generic-layer towers (kind '%s') are not built for retrieval; the step engine's "
                                      "%s towers at width 128, hidden [256, 128, 64] are (TowerEngine.%s)%s" % (
                                          name, self.kind, served, name,
                                          "; GraphEngine.enable_retrieval() lets this engine serve the call" if opt_in else ""))

    def recommend(self, *args, **kwargs):
        self._refuse_retrieval("recommend", "mlp / wdl / deepfm")
        return DeviceEngine.recommend(self, *args, **kwargs)

    def recommend_domain(self, *args, **kwargs):
        self._refuse_retrieval("recommend_domain", "mlp / wdl / deepfm / star")
        return DeviceEngine.recommend_domain(self, *args, **kwargs)

    def rank_domain(self, *args, **kwargs):
        self._refuse_retrieval("rank_domain", "mlp / wdl / deepfm / star")
        return DeviceEngine.rank_domain(self, *args, **kwargs)

    def rank_slates(self, *args, **kwargs):
        self._refuse_retrieval("rank_slates", "mlp / wdl / deepfm / star")
        return DeviceEngine.rank_slates(self, *args, **kwargs)

    def set_adam_eps(self, eps):
        self._check(self.lib.mamdr_graph_set_adam_eps(self.ctx, float(eps)))
