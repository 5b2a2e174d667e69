"""Device-resident tower: the compiled-Keras-model stand-in over libmamdr_hip.so.

`TowerEngine` owns (through torch, used purely as the device allocator / stream
provider) the flat trainable vector with its Adam slots, the frozen tables and
the per-domain split columns, and forwards every numeric operation to the C ABI
(include/mamdr_hip.h).  It exposes what the reference's wrappers use of the
Keras model:

    train_on_batch / fit        -> train_pass / train_steps   (mamdr.py:54,86,97)
    evaluate                    -> evaluate                   (base_model.py:131)
    K.batch_get_value(vars)     -> get_weights / weights      (maml.py:189-194)
    SetVarOp(vars)(values)      -> set_weights                (utils/tool.py:36-45)

plus the outer-update primitives on flat vectors (`FlatVectorOps`).  `DeviceEngine` holds what `TowerEngine` and
`graph_engine.GraphEngine` do alike over their two entry-point families; `keras_names` is the one table of Keras
variable names behind the reference's name filters.  No CPU fallback exists.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import bootstrap
from . import exact
from . import gauc
from . import reports
from .recommend import exclusion_csr, slates_csr


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def auc_thresholds(num_thresholds=500):
    """utils/auc.py:118-126 (python doubles -> fp32 constant)."""
    inner = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
    return np.array([0.0 - 1e-7] + inner + [1.0 + 1e-7], dtype=np.float32)


def auc_from_histogram(hist):
    """AUC(num_thresholds=500) from the kernel's exact integer histogram.

    hist[c, k] = rows of class c whose prediction exceeds exactly k thresholds, so
    the confusion counts of utils/metrics_utils.py:297-354 are suffix sums:
    tp[t] = #{pos: pred > thr_t} = sum_{k > t} hist[1, k].  The Riemann sum follows
    utils/auc.py:248-281 in fp32 (counts are exact in fp32 below 2^24, as in the
    reference's fp32 accumulators).
    """
    hist = np.asarray(hist, dtype=np.int64).reshape(2, 501)
    suffix = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1]      # suffix[c, k] = sum_{k' >= k}
    tp = suffix[1, 1:].astype(np.float32)                    # t = 0..499 -> k >= t+1
    fp = suffix[0, 1:].astype(np.float32)
    fn = (hist[1].sum() - suffix[1, 1:]).astype(np.float32)
    tn = (hist[0].sum() - suffix[0, 1:]).astype(np.float32)

    def div_no_nan(a, b):
        out = np.zeros_like(a)
        nz = b != 0
        out[nz] = a[nz] / b[nz]
        return out

    recall = div_no_nan(tp, tp + fn)
    fpr = div_no_nan(fp, fp + tn)
    heights = (recall[:-1] + recall[1:]) / np.float32(2.0)
    return float(np.sum((fpr[:-1] - fpr[1:]) * heights, dtype=np.float32)), (tp, fp, tn, fn)


class FlatVectorOps(object):
    """the outer (meta) updates on flat device vectors: stateless entry points of the library, shared by every engine
    (bit-exact vs the reference's numpy, see include/mamdr_hip.h).  Needs self.lib, self.stream, self.weights."""

    def _s(self):
        return C.c_void_p(self.stream.cuda_stream)

    # outer updates (bit-exact vs the reference's numpy, see include/mamdr_hip.h)
    def interp(self, dst, a, b, scale):
        L.check(self.lib.mamdr_interp(_ptr(dst), _ptr(a), _ptr(b), float(scale), dst.numel(), self._s()))

    def merge(self, dst, theta, phi, method="plus"):
        mode = {"plus": L.MERGE_PLUS, "times": L.MERGE_TIMES}[method]
        L.check(self.lib.mamdr_merge(_ptr(dst), _ptr(theta), _ptr(phi), mode, dst.numel(), self._s()))

    # ---- the COMPILED optimiser (deepctr.py:54-60: `model.compile(optimizer=opt)`): the wrappers' train_on_batch / fit calls
    # -- train_steps(optimizer="adam") here -- run whatever the model was compiled with.  train.optimizer "adam" =
    # tf.train.AdamOptimizer(learning_rate); any other value is handed to Keras as a STRING, i.e. the Keras optimiser of
    # that name with ITS default hyper-parameters: "sgd" = SGD(lr 0.01, no momentum), whatever learning_rate says.
    compiled = ("adam", None)

    def compile(self, optimizer):
        if optimizer == "adam":
            self.compiled = ("adam", None)
        elif optimizer == "sgd":
            self.compiled = ("sgd", 0.01)
        else:
            raise NotImplementedError("train.optimizer '%s': Keras optimisers other than 'sgd' are not built (the reference's "
                                      "configs all use adam: deepctr.py:54-57)" % optimizer)

    def _compiled(self, optimizer, lr):
        """(optimizer, lr) a train_steps call runs: "adam" names the compiled optimiser."""
        if optimizer == "adam" and self.compiled[0] != "adam":
            return self.compiled
        return optimizer, lr

    # ---- meta parameters (MAML._get_model_meta_parms, maml.py:153-179): theta / phi vectors cover ONE contiguous range
    # [meta_off, meta_off + n_meta) of the flat vector -- the whole vector ("all"), the Star filter's prefix, or e.g.
    # "all_hidden" (everything behind the embedding tables)
    meta_off = 0

    # tensors INSIDE the meta range that are not meta parameters (a `meta_parms` name list that selects tensors which are
    # no neighbours in the flat vector, maml.py:167-177): [(offset within the range, count)].  theta / phi / merged span
    # the whole range; the slots of these tensors carry no meaning and `assign_meta` never lets them reach the model.
    meta_holes = ()

    def set_meta_range(self, off, count, holes=()):
        if off < 0 or count <= 0 or off + count > self.n_params:
            raise ValueError("meta range [%d, %d) outside the flat vector of %d floats" % (off, off + count, self.n_params))
        for o, c in holes:
            if o < 0 or c <= 0 or o + c > count:
                raise ValueError("hole [%d, %d) outside the meta range of %d floats" % (o, o + c, count))
        self.meta_off, self.n_meta = int(off), int(count)
        self.meta_holes = tuple((int(o), int(c)) for o, c in holes)

    def assign_meta(self, vec):
        """MAML._set_model_meta_parms (maml.py:181-187; SetVarOp over `model_meta_parms`): the meta parameters of the live
        model := vec.  Every other variable keeps training where it is -- the tensors between two selected ones first
        take their live values into `vec`, then the range is assigned in one copy."""
        if vec.numel() != self.n_meta:
            raise ValueError("assign_meta: %d values for %d meta parameters" % (vec.numel(), self.n_meta))
        live = self.meta_weights
        for o, c in self.meta_holes:
            L.check(self.lib.mamdr_copy(_ptr(vec[o:o + c]), _ptr(live[o:o + c]), c, self._s()))
        L.check(self.lib.mamdr_copy(_ptr(live), _ptr(vec), self.n_meta, self._s()))

    @property
    def meta_weights(self):
        """live values of the meta parameters (a view: no copy)."""
        return self.weights[self.meta_off:self.meta_off + self.n_meta]

    def dr_advance(self, phi, merged, theta, gamma, method="plus", assign_model=True):
        """one DR support step in a single pass: phi += (live - merged) * gamma; merged = theta (+|*) phi; and, for
        the next support, model := merged (mamdr.py:103-105,74) -- bit-identical to interp + merge + set_weights."""
        mode = {"plus": L.MERGE_PLUS, "times": L.MERGE_TIMES}[method]
        holes = bool(self.meta_holes) and assign_model      # (the kernel's assignment would overwrite the tensors in between)
        # self.weights (not _weights): the live table rows must be brought up to the current Adam step before they
        # are read into phi / replaced by merged (include/mamdr_hip.h: sync before reading or replacing the state)
        L.check(self.lib.mamdr_dr_advance(_ptr(phi), _ptr(self.meta_weights), _ptr(merged), _ptr(theta), float(gamma), mode,
                                          1 if (assign_model and not holes) else 0, phi.numel(), self._s()))
        if holes:
            self.assign_meta(merged)

    def sub(self, dst, a, b):
        L.check(self.lib.mamdr_sub(_ptr(dst), _ptr(a), _ptr(b), dst.numel(), self._s()))

    def accumulate(self, acc, a, b, shared=None, divisor=1.0):
        L.check(self.lib.mamdr_accumulate(_ptr(acc), _ptr(a), _ptr(b), _ptr(shared), float(divisor),
                                          acc.numel(), self._s()))

    def apply_accumulated(self, dst, acc, divisor, scale):
        L.check(self.lib.mamdr_apply_accumulated(_ptr(dst), _ptr(acc), float(divisor), float(scale),
                                                 dst.numel(), self._s()))


    def adam_apply(self, p, m, v, g, lr, beta1_power, beta2_power, grad_scale=1.0):
        """outer TF1 Adam on flat vectors (maml.py:236-243)."""
        L.check(self.lib.mamdr_adam_apply(_ptr(p), _ptr(m), _ptr(v), _ptr(g), float(grad_scale), float(lr), 0.9, 0.999,
                                          1e-8, float(beta1_power), float(beta2_power), p.numel(), self._s()))


    def pcgrad_project(self, final, aux, tensors=None):
        """PCGrad.PCGrad with final_grads is current_grads (pcgrad.py:107-124,152-160) on flat device vectors.
        tensors: [(offset, rows, cols)], default = every segment inside the vectors.  Any number of tensors: one call
        takes at most L.PCG_MAX_SEG of them (its table travels as a kernel argument), the tensors are independent of
        each other, so the list goes out in calls of that many -- the same bytes as one call would leave."""
        if tensors is None:
            shapes = self.segment_shapes()
            tensors = [(off, shapes[n][0], shapes[n][1]) for n, (off, cnt) in self.segments.items()
                       if off + cnt <= final.numel()]
        for lo in range(0, max(len(tensors), 1), L.PCG_MAX_SEG):
            part = tensors[lo:lo + L.PCG_MAX_SEG]
            n = len(part)
            offs = (C.c_int64 * n)(*[t[0] for t in part])
            rows = (C.c_int64 * n)(*[t[1] for t in part])
            cols = (C.c_int32 * n)(*[t[2] for t in part])
            L.check(self.lib.mamdr_pcgrad_project(_ptr(final), _ptr(aux), offs, rows, cols, n, self._s()))

    # ---- fp64 Gram matrices of flat vectors (mamdr_gram; no reference counterpart)
    _gram_work = None       # the slab partials' workspace: kept by the engine, grown on demand

    def gram(self, vecs, ranges):
        """fp64 Gram matrices of the rows of `vecs` -- a 2-D fp32 device tensor [D, n], D <= 32, unit stride along a row,
        any stride between rows -- over `ranges` = [(offset, count)] inside [0, n): overlapping, empty and unaligned ranges
        are fine.  -> float64 device tensor [len(ranges), D, D], out[r, i, j] = sum_k double(v_i[k]) * double(v_j[k]) over
        range r: symmetric bit for bit, and the same bits for the same values and ranges wherever the rows sit
        (include/mamdr_hip.h: mamdr_gram).  Nothing is read back."""
        if vecs.dim() != 2 or vecs.dtype != torch.float32 or not vecs.is_cuda or (vecs.shape[1] > 1 and vecs.stride(1) != 1):
            raise ValueError("gram: vecs must be a 2-D fp32 device tensor with unit stride along its rows")
        D, n = int(vecs.shape[0]), int(vecs.shape[1])
        stride = int(vecs.stride(0)) if D > 1 else n
        if not 1 <= D <= L.GRAM_MAX_VEC or stride < n:
            raise ValueError("gram: %d vectors (1 to %d), row stride %d for %d columns" % (D, L.GRAM_MAX_VEC, stride, n))
        R = len(ranges)
        offs = (C.c_int64 * max(R, 1))(*[int(r[0]) for r in ranges])
        cnts = (C.c_int64 * max(R, 1))(*[int(r[1]) for r in ranges])
        for o, c in zip(offs[:R], cnts[:R]):
            if o < 0 or c < 0 or o + c > n:
                raise ValueError("gram: range [%d, %d) outside the %d columns" % (o, o + c, n))
        need = int(self.lib.mamdr_gram_work(D, offs, cnts, R))
        if need < 0:
            L.check(need)
        if self._gram_work is None or self._gram_work.numel() < need:
            self._gram_work = torch.empty(max(need, 1), dtype=torch.float64, device=vecs.device)
        out = torch.empty((R, D, D), dtype=torch.float64, device=vecs.device)
        L.check(self.lib.mamdr_gram(_ptr(vecs), stride, D, n, offs, cnts, R, _ptr(self._gram_work), self._gram_work.numel(),
                                    _ptr(out), self._s()))
        return out


# Keras variable names of the step engine's segments, for the reference's substring filters (maml.py:153-179)
KERAS_NAMES = {"Ws0": "kernel_shared_0", "Ws1": "kernel_shared_1", "Ws2": "kernel_shared_2",
               "bs0": "bias_shared_0", "bs1": "bias_shared_1", "bs2": "bias_shared_2",
               "Wd0": "kernel_specific_0", "Wd1": "kernel_specific_1", "Wd2": "kernel_specific_2",
               "bd0": "bias_specific_0", "bd1": "bias_specific_1", "bd2": "bias_specific_2",
               "pn_gamma_shared": "gamma_shared", "pn_beta_shared": "beta_shared",
               "pn_gamma_spec": "gamma_specific", "pn_beta_spec": "beta_specific",
               "wo": "dense/kernel", "gb": "dense/bias",
               # deepctr's embedding layers: "sparse_emb_<feature>", the 1-d linear ones "linear...sparse_emb_<feature>"
               "user_emb": "sparse_emb_uid", "item_emb": "sparse_emb_pid", "domain_emb": "sparse_emb_domain",
               "lin_user": "linear0sparse_emb_uid", "lin_item": "linear0sparse_emb_pid",
               "lin_domain": "linear0sparse_emb_domain"}


def keras_names(kind, dense=None, segments=()):
    """{segment: Keras variable name} (a segment that is not listed keeps its own name).  dense None: the step engine's
    towers, the step Star form among them.  kind "star" with dense "star" / "dense": model_zoo/Star's layers on the
    generic-layer engine and in the plain-DNN form -- the shared / specific names for any layer count, auxiliary_net/*,
    batch_normalization/*; with dense "dense" the numbered Keras Dense layers behind `segments` (output unit last).  Every
    other kind of the generic-layer engine: its tensor names."""
    if dense is None:
        return KERAS_NAMES
    if kind != "star":
        return {}
    names = dict(KERAS_NAMES)
    names.update({"user_emb": "user_emb/embeddings", "item_emb": "item_emb/embeddings", "domain_emb": "domain_emb/embeddings",
                  "aux_W": "auxiliary_net/kernel_specific", "aux_b": "auxiliary_net/bias_specific",
                  "bn_gamma": "batch_normalization/gamma", "bn_beta": "batch_normalization/beta"})
    for l in range(4):
        names["Ws%d" % l], names["bs%d" % l] = "kernel_shared_%d" % l, "bias_shared_%d" % l
        names["Wd%d" % l], names["bd%d" % l] = "kernel_specific_%d" % l, "bias_specific_%d" % l
    if dense == "dense":
        n = len([s for s in segments if s in ("W0", "W1", "W2", "W3")])
        for l in range(n):
            stem = "dense" if l == 0 else "dense_%d" % l
            names["W%d" % l], names["b%d" % l] = stem + "/kernel", stem + "/bias"
        names["wo"], names["gb"] = "dense_%d/kernel" % n, "dense_%d/bias" % n
    return names


def keras_name(kind, dense, segments, segment):
    """Keras variable name of one segment, for the reference's substring filters (maml.py:153-179)."""
    return keras_names(kind, dense, segments).get(segment, segment)


class DeviceEngine(FlatVectorOps):
    """what the two engines do alike over their entry-point families (`mamdr_*`, `mamdr_graph_*`: the same signatures,
    _lib.SIGNATURES): device and stream, the bound state vectors and aux buffer, tables and split columns, train_steps with
    the moving-average accumulate pass, evaluate, the accumulator and the counters.  A subclass names its family (PREFIX,
    GRAPH), creates its context between `_open` and `_bind_buffers`, and says how `keras_names` is keyed."""
    PREFIX, GRAPH = None, False
    SHARED_CALLS = ("destroy", "bind_state", "aux_count", "bind_aux", "bind_table", "bind_domain_data", "train_steps_n",
                    "eval_domain", "bind_accumulator", "set_counters", "optimizer_reset")

    def _open(self, device, n_user, n_item, n_domain, batch_size, dropout_seed, emb_trainable):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("%s needs a HIP device (no CPU fallback for the MAMDR hot path)" % type(self).__name__)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.current_stream(self.device)
        self.n_user, self.n_item, self.n_domain = int(n_user), int(n_item), int(n_domain)
        self.batch_size = int(batch_size)
        self.dropout_seed = int(dropout_seed) & 0xFFFFFFFF
        self.emb_trainable = bool(emb_trainable)
        # the family's entry points, resolved once (train_steps runs inside the benchmark's timed region)
        for name in self.SHARED_CALLS:
            setattr(self, "_c_" + name, getattr(self.lib, self.PREFIX + name))
        self._c_id_counts, self._c_list_similarity = self.lib.mamdr_id_counts, self.lib.mamdr_list_similarity
        self._c_list_diversify = self.lib.mamdr_list_diversify
        self._c_row_neighbours = self.lib.mamdr_row_neighbours
        self._c_row_neighbours_bounded = self.lib.mamdr_row_neighbours_bounded

    def _check(self, code):
        return L.check(code, graph=self.GRAPH)

    def _bind_buffers(self, aux_ones):
        """live state: weights + Adam slots (one set for the whole run); the non-trainable state of a norm layer
        (zeros, `aux_ones` ones from offset `aux_ones`: the moving variances); the evaluation's read-back buffers."""
        self._weights = self.new_vector()
        self._adam_m = self.new_vector()
        self._adam_v = self.new_vector()
        self._check(self._c_bind_state(self.ctx, _ptr(self._weights), _ptr(self._adam_m), _ptr(self._adam_v)))
        self.aux = None
        n_aux = int(self._c_aux_count(self.ctx))
        if n_aux:
            self.aux = torch.zeros(n_aux, dtype=torch.float32, device=self.device)
            self.aux[aux_ones:2 * aux_ones] = 1.0
            self._check(self._c_bind_aux(self.ctx, _ptr(self.aux)))
        self.tables = {}
        self.data = {}          # (domain, split) -> dict of device columns
        self._acc = None
        self._ema = None            # set_moving_average
        self._hist = torch.zeros(2 * 501, dtype=torch.int32, device=self.device)
        self._loss1 = torch.zeros(1, dtype=torch.float32, device=self.device)

    @property
    def weights(self):
        return self._weights

    @property
    def adam_m(self):
        return self._adam_m

    @property
    def adam_v(self):
        return self._adam_v

    def close(self):
        if getattr(self, "ctx", None):
            torch.cuda.synchronize(self.device)
            self._c_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ flat vectors
    def new_vector(self, like=None, meta=False):
        if like is not None:
            return like.clone()
        return torch.zeros(self.n_meta if meta else self.n_params, dtype=torch.float32, device=self.device)

    def keras_name(self, segment):
        return keras_name(*self.keras_key(), segment)

    def pack(self, named):
        """numpy dict {segment name: array} -> flat device vector (padding zero)."""
        host = np.zeros(self.n_params, np.float32)
        for name, (off, cnt) in self.segments.items():
            a = np.asarray(named[name], np.float32).ravel()
            if a.size != cnt:
                raise ValueError("segment %s has %d elements, expected %d" % (name, a.size, cnt))
            host[off:off + cnt] = a
        return torch.from_numpy(host).to(self.device)

    def unpack(self, vec):
        host = vec.detach().cpu().numpy()
        return {name: host[off:off + cnt].copy() for name, (off, cnt) in self.segments.items()}

    def aux_state(self):
        """PartitionedNorm (the step Star tower, the pn forms): {mov_mean, mov_var [D,384], steps [D]} as numpy (partitioned_norm.py:71-87)."""
        if self.aux is None:
            return {}
        h = self.aux.cpu().numpy()
        dx = self.n_domain * 384
        return {"mov_mean": h[0:dx].reshape(self.n_domain, 384).copy(),
                "mov_var": h[dx:2 * dx].reshape(self.n_domain, 384).copy(),
                "biased_mean": h[2 * dx:3 * dx].reshape(self.n_domain, 384).copy(),
                "biased_var": h[3 * dx:4 * dx].reshape(self.n_domain, 384).copy(),
                "steps": h[4 * dx:4 * dx + self.n_domain].copy()}

    # ------------------------------------------------------------ binding
    def bind_table(self, name, rows):
        """frozen pretrained table (deepctr.py:104-116), numpy [n, emb_dim] fp32."""
        seg = {"user_emb": L.SEG_USER_EMB, "item_emb": L.SEG_ITEM_EMB}[name]
        t = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(self.device)
        self.tables[name] = t
        self._check(self._c_bind_table(self.ctx, seg, _ptr(t), t.shape[0]))

    def bind_domain_data(self, domain, split, uid, pid, dom, label):
        split_id = {"train": L.SPLIT_TRAIN, "val": L.SPLIT_VAL, "test": L.SPLIT_TEST}[split]
        uid = np.ascontiguousarray(uid, np.int32)
        pid = np.ascontiguousarray(pid, np.int32)
        dom = np.ascontiguousarray(dom, np.int32)
        if uid.size:
            if uid.min() < 0 or uid.max() >= self.n_user or pid.min() < 0 or pid.max() >= self.n_item \
                    or dom.min() < 0 or dom.max() >= self.n_domain:
                raise ValueError("domain %d %s: id out of range" % (domain, split))
        cols = {
            "uid": torch.from_numpy(uid).to(self.device),
            "pid": torch.from_numpy(pid).to(self.device),
            "domain": torch.from_numpy(dom).to(self.device),
            "label": torch.from_numpy(np.ascontiguousarray(label, np.float32)).to(self.device),
        }
        self.data[(domain, split)] = cols
        self._check(self._c_bind_domain_data(self.ctx, domain, split_id, _ptr(cols["uid"]), _ptr(cols["pid"]),
                                             _ptr(cols["domain"]), _ptr(cols["label"]), uid.shape[0]))

    def n_rows(self, domain, split):
        return int(self.data[(domain, split)]["uid"].shape[0])

    # ------------------------------------------------------------ the hot path
    def train_steps(self, domain, perm=None, first_step=0, n_steps=None, lr=1e-3, optimizer="adam",
                    loss_out=None, batch_size=None, pass_rows=None):
        """n_steps x train_on_batch on one domain, device-side. perm: int32 device tensor or None.
        pass_rows: the pass covers only that many positions (perm then lists that many rows of the split) --
        the take / skip sub-datasets of the meta-train / meta-val split."""
        bs = batch_size or self.batch_size
        n = self.n_rows(domain, "train") if pass_rows is None else int(pass_rows)
        if n_steps is None:
            n_steps = -(-n // bs) - first_step
        optimizer, lr = self._compiled(optimizer, lr)
        opt = {"adam": L.OPT_ADAM, "sgd": L.OPT_SGD, "accumulate": L.OPT_ACCUMULATE}[optimizer]
        rows = -1 if pass_rows is None else n
        if optimizer == "accumulate" and self._ema is not None:
            # average_meta_grad == "moving_mean": every meta batch updates the accumulator's moving average
            # (maml.py:219-220) -- one step at a time into a scratch gradient, then mamdr_moving_average
            ema = self._ema
            if loss_out is not None:
                raise ValueError("accumulate passes under average_meta_grad = moving_mean report no per-step loss")
            for s in range(first_step, first_step + n_steps):
                ema["scratch"].zero_()
                self._check(self._c_train_steps_n(self.ctx, domain, _ptr(perm), rows, s, 1, bs, self.dropout_seed, opt,
                                                  float(lr), _ptr(None)))
                ema["step"] += 1
                decay = np.float32(1.0 - ema["momentum"])
                denom = np.float32(1.0) - np.power(np.float32(1.0) - decay, np.float32(ema["step"]), dtype=np.float32)
                L.check(self.lib.mamdr_moving_average(_ptr(self._acc), _ptr(ema["biased"]), _ptr(ema["scratch"]),
                                                      float(decay), float(denom), self._acc.numel(), self._s()))
            return n_steps
        self._check(self._c_train_steps_n(self.ctx, domain, _ptr(perm), rows, first_step, n_steps, bs, self.dropout_seed,
                                          opt, float(lr), _ptr(loss_out)))
        return n_steps

    def evaluate(self, domain, split, want_preds=False, want_gauc=False, want_exact=0, want_ci=None):
        """model.evaluate(data, steps=n_step) -> (loss, auc[, hist, preds][, gauc report][, exact report][, ci report]); syncs
        to read back.  The reports (reports.EVAL_REPORTS; none has a reference counterpart): the predictions stay on the device,
        the report's chain runs behind the evaluation on the engine's stream, and its finished dict ends the tuple, in table
        order.  want_gauc: mamdr_group_auc over the split's uid groups (gauc.finish).  want_exact = B > 0: mamdr_exact_metrics
        with B calibration bins (exact.finish).  want_ci = (n_rep, seed, "row" | "user"): mamdr_auc_bootstrap, "user"
        resampling the bound split's uid column, "row" its rows (bootstrap.finish)."""
        n = self.n_rows(domain, split)
        want = {"want_gauc": want_gauc, "want_exact": int(want_exact or 0), "want_ci": want_ci}
        wanted = [(e, want[e.keyword]) for e in reports.EVAL_REPORTS if want[e.keyword] not in (None, False, 0)]   # (the defaults)
        if want_ci is not None:             # (before anything is launched)
            _, _, ci_unit = want_ci
            if ci_unit not in ("row", "user"):
                raise ValueError("want_ci: the unit is 'row' or 'user', got %r" % (ci_unit,))
        preds = torch.empty(n, dtype=torch.float32, device=self.device) if (want_preds or wanted) else None
        split_id = {"train": L.SPLIT_TRAIN, "val": L.SPLIT_VAL, "test": L.SPLIT_TEST}[split]
        self._check(self._c_eval_domain(self.ctx, domain, split_id, self.eval_batch, _ptr(self._loss1),
                                        _ptr(self._hist), _ptr(preds)))
        launched = [(e, e.launch(self, preds, self.data[(domain, split)], req)) for e, req in wanted]
        hist = self._hist.cpu().numpy().astype(np.int64)
        loss = float(self._loss1.cpu().numpy()[0])
        auc, _ = auc_from_histogram(hist)
        out = (loss, auc)
        if want_preds:
            out += (hist.reshape(2, 501), preds.cpu().numpy())
        return out + tuple(e.finish(tensors) for e, tensors in launched)

    def _check_pair(self, what, preds, labels):
        if preds.numel() != labels.numel() or preds.dtype != torch.float32 or labels.dtype != torch.float32 \
                or preds.device != self.device or labels.device != self.device:
            raise ValueError("%s: preds and labels must be fp32 tensors of one length on the engine's device" % what)

    # ------------------------------------------------------------ bootstrap replicates of the exact AUC (no reference counterpart)
    def _bootstrap_launch(self, preds, labels, n_rep, seed, unit=None, part_words=None):
        """mamdr_auc_bootstrap on the engine's stream -> the device tensors (T, P, N), int64 [n_rep + 1] each (T holds
        uint64 words); nothing is read back.  part_words (tests): mamdr_auc_bootstrap_bounded with that workspace bound."""
        n, n_rep = int(preds.numel()), int(n_rep)
        bootstrap.check_sizes(n, n_rep)
        T, P, N = [torch.empty(n_rep + 1, dtype=torch.int64, device=self.device) for _ in range(3)]
        args = (_ptr(preds if n else None), _ptr(labels if n else None), _ptr(unit if n else None), n, n_rep,
                int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(T), _ptr(P), _ptr(N))
        if part_words is None:
            L.check(self.lib.mamdr_auc_bootstrap(*args, self._s()))
        else:
            L.check(self.lib.mamdr_auc_bootstrap_bounded(*args, int(part_words), self._s()))
        return T, P, N

    def auc_bootstrap(self, preds, labels, n_rep, seed=0, unit=None, level=0.95):
        """bootstrap replicates of the exact AUC (bootstrap.py's definition) of device tensors preds / labels [n] fp32 and,
        optionally, unit [n] int32 (the resampling unit of every row; None resamples rows) -> bootstrap.finish's report."""
        self._check_pair("auc_bootstrap", preds, labels)
        if unit is not None and (unit.numel() != preds.numel() or unit.dtype != torch.int32 or unit.device != self.device):
            raise ValueError("auc_bootstrap: unit must be an int32 tensor of the predictions' length on the engine's device")
        T, P, N = self._bootstrap_launch(preds.contiguous(), labels.contiguous(), n_rep, seed,
                                         unit.contiguous() if unit is not None else None)
        return bootstrap.finish(T.cpu().numpy().view(np.uint64), P.cpu().numpy(), N.cpu().numpy(), level)

    # ------------------------------------------------------------ exact AUC / AP / calibration (no reference counterpart)
    def _exact_launch(self, preds, labels, n_bins, want_sorted=False):
        """mamdr_exact_metrics on the engine's stream -> the device tensors (counts [5] int64, ap_sum [1] fp64, bins [3,
        n_bins] int64, sorted composites [n] int64 or None); nothing is read back."""
        n, n_bins = int(preds.numel()), int(n_bins)
        if not 1 <= n_bins <= exact.MAX_BINS:
            raise ValueError("exact metrics: n_bins %d outside 1..%d" % (n_bins, exact.MAX_BINS))
        counts = torch.empty(5, dtype=torch.int64, device=self.device)
        ap = torch.empty(1, dtype=torch.float64, device=self.device)
        bins = torch.empty((3, n_bins), dtype=torch.int64, device=self.device)
        out = torch.empty(n, dtype=torch.int64, device=self.device) if want_sorted else None
        L.check(self.lib.mamdr_exact_metrics(_ptr(preds if n else None), _ptr(labels if n else None), n, n_bins, _ptr(counts),
                                             _ptr(ap), _ptr(bins), _ptr(out if n else None), self._s()))
        return counts, ap, bins, out

    def exact_metrics(self, preds, labels, n_bins, want_sorted=False):
        """exact AUC, average precision and calibration (exact.py's definition) of device tensors preds / labels [n] fp32
        -> exact.finish's report; want_sorted adds "sorted", the sorted composites (int64 numpy)."""
        self._check_pair("exact_metrics", preds, labels)
        counts, ap, bins, out = self._exact_launch(preds.contiguous(), labels.contiguous(), n_bins, want_sorted)
        rep = exact.finish(counts.cpu().numpy(), ap.cpu().numpy()[0], bins.cpu().numpy())
        if want_sorted:
            rep["sorted"] = out.cpu().numpy()
        return rep

    # ------------------------------------------------------------ isotonic fit / apply / score sums (no reference counterpart)
    def predict_device(self, domain, split):
        """the fp32 predictions of a bound split as a DEVICE tensor [n]: the launch of evaluate(..., want_preds=True) on the
        engine's stream, without the copy -- nothing is read back."""
        preds = torch.empty(self.n_rows(domain, split), dtype=torch.float32, device=self.device)
        split_id = {"train": L.SPLIT_TRAIN, "val": L.SPLIT_VAL, "test": L.SPLIT_TEST}[split]
        self._check(self._c_eval_domain(self.ctx, domain, split_id, self.eval_batch, _ptr(self._loss1), _ptr(self._hist),
                                        _ptr(preds)))
        return preds

    def _isotonic_fit_launch(self, preds, labels, tile_points=None):
        """mamdr_isotonic_fit on the engine's stream -> the device tensors (counts [4] int64, first_key [n] int32 holding
        uint32 words, rows [n] int64, positives [n] int64); nothing is read back.  tile_points (tests):
        mamdr_isotonic_fit_bounded with that tile of the hull's levels."""
        from . import isotonic          # (here, not at the top: a run without --isotonic never imports the module)
        n = int(preds.numel())
        if tile_points is not None and int(tile_points) < isotonic.MIN_TILE:
            raise ValueError("isotonic fit: tile_points %d below %d" % (int(tile_points), isotonic.MIN_TILE))
        counts = torch.empty(4, dtype=torch.int64, device=self.device)
        first_key = torch.empty(n, dtype=torch.int32, device=self.device)
        rows, positives = [torch.empty(n, dtype=torch.int64, device=self.device) for _ in range(2)]
        args = (_ptr(preds if n else None), _ptr(labels if n else None), n, _ptr(counts), _ptr(first_key if n else None),
                _ptr(rows if n else None), _ptr(positives if n else None))
        if tile_points is None:
            L.check(self.lib.mamdr_isotonic_fit(*args, self._s()))
        else:
            L.check(self.lib.mamdr_isotonic_fit_bounded(*args, int(tile_points), self._s()))
        return counts, first_key, rows, positives

    def isotonic_fit(self, preds, labels, tile_points=None):
        """the isotonic (PAV) fit (isotonic.py's definition) of device tensors preds / labels [n] fp32 -> isotonic.table's
        dict: the counts and the block table as numpy arrays."""
        from . import isotonic
        self._check_pair("isotonic_fit", preds, labels)
        counts, first_key, rows, positives = self._isotonic_fit_launch(preds.contiguous(), labels.contiguous(), tile_points)
        nb = int(counts.cpu().numpy()[0])
        return isotonic.table(counts.cpu().numpy(), first_key[:nb].cpu().numpy(), rows[:nb].cpu().numpy(),
                              positives[:nb].cpu().numpy())

    def _isotonic_apply_launch(self, first_key, rows, positives, n_blocks, preds):
        """mamdr_isotonic_apply on the engine's stream over device tensors -> the device tensor of fitted values [n] fp32."""
        n = int(preds.numel())
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        L.check(self.lib.mamdr_isotonic_apply(_ptr(first_key), _ptr(rows), _ptr(positives), int(n_blocks),
                                              _ptr(preds if n else None), n, _ptr(out if n else None), self._s()))
        return out

    def isotonic_apply(self, fit, preds):
        """the step function of `fit` (isotonic_fit's / isotonic.table's dict) at the device tensor preds [n] fp32 -> the
        DEVICE tensor of fitted values [n] fp32 (isotonic.apply_host's)."""
        if preds.dtype != torch.float32 or preds.device != self.device:
            raise ValueError("isotonic_apply: preds must be an fp32 tensor on the engine's device")
        nb = int(fit["n_blocks"])
        if preds.numel() and nb < 1:
            raise ValueError("isotonic_apply: a fit without blocks cannot be applied")
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a[:nb]).view(t)).to(self.device)      # noqa: E731
        return self._isotonic_apply_launch(up(fit["first_key"], np.int32), up(fit["rows"], np.int64),
                                           up(fit["positives"], np.int64), nb, preds.contiguous())

    def _score_sums_launch(self, preds, labels):
        """mamdr_score_sums on the engine's stream -> the device tensor [2] fp64 (Brier sum, log-loss sum)."""
        n = int(preds.numel())
        out = torch.empty(2, dtype=torch.float64, device=self.device)
        L.check(self.lib.mamdr_score_sums(_ptr(preds if n else None), _ptr(labels if n else None), n, _ptr(out), self._s()))
        return out

    def score_sums(self, preds, labels):
        """(Brier sum, log-loss sum) (isotonic.py's definition) of device tensors preds / labels [n] fp32, as floats."""
        self._check_pair("score_sums", preds, labels)
        out = self._score_sums_launch(preds.contiguous(), labels.contiguous()).cpu().numpy()
        return float(out[0]), float(out[1])

    # ------------------------------------------------------------ per-user grouped AUC (no reference counterpart)
    def group_auc_plan(self, domain, split):
        """the device copy of gauc.group_plan over the bound split's uid column: built at first use, uploaded once, kept with
        the split's columns (bind_domain_data replaces both)."""
        return self._group_plan_of(self.data[(domain, split)])

    def _group_plan_of(self, cols):
        if "gauc_plan" not in cols:
            cols["gauc_plan"] = self.upload_group_plan(gauc.group_plan(cols["uid"].cpu().numpy()))
        return cols["gauc_plan"]

    def upload_group_plan(self, plan):
        """gauc.GroupPlan of numpy arrays -> the same of device tensors."""
        return gauc.GroupPlan(*[torch.from_numpy(np.ascontiguousarray(a, t)).to(self.device) for a, t in
                                zip(plan, (np.int32, np.int64, np.int32, np.int64))])

    def _group_auc_launch(self, preds, labels, plan, T=None, P=None):
        """mamdr_group_auc on the engine's stream -> the device tensor of its four results (nothing is read back)."""
        res4 = torch.empty(4, dtype=torch.float64, device=self.device)
        n_tiles = int(plan.tile_group.shape[0])
        L.check(self.lib.mamdr_group_auc(_ptr(preds), _ptr(labels), _ptr(plan.order), int(plan.order.shape[0]),
                                         _ptr(plan.group_off), int(plan.group_off.shape[0]) - 1,
                                         _ptr(plan.tile_group if n_tiles else None), _ptr(plan.tile_first if n_tiles else None),
                                         n_tiles, _ptr(T), _ptr(P), _ptr(res4), self._s()))
        return res4

    def group_auc(self, preds, labels, plan, want_groups=False):
        """GAUC (gauc.py's definition) of device tensors preds / labels [n] fp32 under `plan` (gauc.GroupPlan of device
        tensors: upload_group_plan, group_auc_plan) -> gauc.finish's report; want_groups adds "T" (uint64) and "P" (uint32)
        per group as numpy."""
        n = int(plan.order.shape[0])
        if preds.numel() != n or labels.numel() != n or preds.dtype != torch.float32 or labels.dtype != torch.float32:
            raise ValueError("group_auc: preds and labels must be fp32 device tensors of the plan's %d rows" % n)
        G = int(plan.group_off.shape[0]) - 1
        T = P = None
        if want_groups:
            # (torch has no uint64 / uint32 arithmetic: int64 / int32 storage, reinterpreted on the host)
            T = torch.empty(max(G, 1), dtype=torch.int64, device=self.device)
            P = torch.empty(max(G, 1), dtype=torch.int32, device=self.device)
        rep = gauc.finish(*self._group_auc_launch(preds, labels, plan, T, P).cpu().numpy().tolist())
        if want_groups:
            rep.update(T=T.cpu().numpy()[:G].view(np.uint64), P=P.cpu().numpy()[:G].view(np.uint32))
        return rep

    # ------------------------------------------------------------ what top-K lists are made of (no reference counterpart)
    def id_counts(self, ids, n_bins, label=None):
        """mamdr_id_counts on the engine's stream: ids -- an int32 device tensor of any shape, taken flat -- counted into
        n_bins bins, with `label` (fp32, as many elements) only the positions whose label is not 0.  An id outside
        [0, n_bins) counts nowhere.  -> the device tensor [n_bins] int32, holding the uint32 counts; nothing is read back."""
        n, n_bins = int(ids.numel()), int(n_bins)
        if ids.dtype != torch.int32 or ids.device != self.device:
            raise ValueError("id_counts: ids must be an int32 tensor on the engine's device")
        if label is not None and (label.dtype != torch.float32 or label.device != self.device or label.numel() != n):
            raise ValueError("id_counts: label must be an fp32 tensor of the ids' length on the engine's device")
        if n_bins <= 0 or n >= 2 ** 32:
            raise ValueError("id_counts: %d bins for %d ids (n_bins > 0, n < 2^32)" % (n_bins, n))
        ids = ids.contiguous()
        label = label.contiguous() if label is not None else None
        counts = torch.empty(n_bins, dtype=torch.int32, device=self.device)
        L.check(self._c_id_counts(_ptr(ids if n else None), _ptr(label if n else None), n, n_bins, _ptr(counts), self._s()))
        return counts

    def list_similarity(self, ids, rows):
        """mamdr_list_similarity on the engine's stream: ids [Q, K] int32 (K <= 128; an id outside [0, n_rows) is padding),
        rows [n_rows, E] fp32 (E 32, 64, 128 or 256; contiguous, 16-byte aligned), both device tensors -> the device tensors
        (sim_sum [Q] float64: per list the sum of its valid entries' pairwise cosines, pairs [Q] int32: how many that is);
        nothing is read back."""
        if ids.dim() != 2 or ids.dtype != torch.int32 or ids.device != self.device:
            raise ValueError("list_similarity: ids must be a [Q, K] int32 tensor on the engine's device")
        if rows.dim() != 2 or rows.dtype != torch.float32 or rows.device != self.device or not rows.is_contiguous():
            raise ValueError("list_similarity: rows must be a contiguous [n_rows, E] fp32 tensor on the engine's device")
        Q, K = int(ids.shape[0]), int(ids.shape[1])
        if not 1 <= K <= L.LIST_MAX_K or int(rows.shape[1]) not in L.LIST_EMB_DIMS or rows.shape[0] < 1:
            raise ValueError("list_similarity: K %d (1 to %d), rows %d x %d (width one of %s)" % (
                K, L.LIST_MAX_K, rows.shape[0], rows.shape[1], (L.LIST_EMB_DIMS,)))
        sim_sum = torch.empty(Q, dtype=torch.float64, device=self.device)
        pairs = torch.empty(Q, dtype=torch.int32, device=self.device)
        if Q:
            L.check(self._c_list_similarity(_ptr(ids.contiguous()), Q, K, _ptr(rows), int(rows.shape[0]), int(rows.shape[1]),
                                            _ptr(sim_sum), _ptr(pairs), self._s()))
        return sim_sum, pairs

    def list_diversify(self, ids, rel, rows, k, lam, want_values=False):
        """mamdr_list_diversify on the engine's stream -- greedy MMR: ids [Q, N] int32 (N <= 128; an id outside [0, n_rows) is
        padding; valid ids distinct within a list), rel [Q, N] fp32 (each entry's relevance, used as given), rows [n_rows, E]
        fp32 as list_similarity takes them, all device tensors; 1 <= k <= N, 0 <= lam <= 1 -> (pos [Q, k] int32: the
        position in its list of pick t, -1 behind a short list; values [Q, k] fp32: what the pick won with, or None
        without want_values); nothing is read back."""
        if ids.dim() != 2 or ids.dtype != torch.int32 or ids.device != self.device:
            raise ValueError("list_diversify: ids must be a [Q, N] int32 tensor on the engine's device")
        if rel.shape != ids.shape or rel.dtype != torch.float32 or rel.device != self.device:
            raise ValueError("list_diversify: rel must be an fp32 tensor of the ids' shape on the engine's device")
        if rows.dim() != 2 or rows.dtype != torch.float32 or rows.device != self.device or not rows.is_contiguous():
            raise ValueError("list_diversify: rows must be a contiguous [n_rows, E] fp32 tensor on the engine's device")
        Q, N, k, lam = int(ids.shape[0]), int(ids.shape[1]), int(k), float(lam)
        if not 1 <= N <= L.LIST_MAX_K or int(rows.shape[1]) not in L.LIST_EMB_DIMS or rows.shape[0] < 1:
            raise ValueError("list_diversify: N %d (1 to %d), rows %d x %d (width one of %s)" % (
                N, L.LIST_MAX_K, rows.shape[0], rows.shape[1], (L.LIST_EMB_DIMS,)))
        if not 1 <= k <= N or not 0.0 <= lam <= 1.0:
            raise ValueError("list_diversify: k %d (1 to N = %d), lambda %r (0 to 1)" % (k, N, lam))
        pos = torch.empty((Q, k), dtype=torch.int32, device=self.device)
        values = torch.empty((Q, k), dtype=torch.float32, device=self.device) if want_values else None
        if Q:
            L.check(self._c_list_diversify(_ptr(ids.contiguous()), _ptr(rel.contiguous()), Q, N, k, lam, _ptr(rows),
                                           int(rows.shape[0]), int(rows.shape[1]), _ptr(pos), _ptr(values), self._s()))
        return pos, values

    def row_neighbours(self, rows, queries, k, candidates=None, exclude_self=True, chunk=None):
        """mamdr_row_neighbours on the engine's stream -- exact cosine nearest neighbours: rows [n_rows, E] fp32 as
        list_similarity takes them, queries [Q] int32 row ids (an id outside [0, n_rows) gets an all-padding list),
        candidates [C] int32 distinct row ids or None (every row), all device tensors; 1 <= k <= 128; exclude_self: a query
        is not its own neighbour; chunk: candidates per pass (mamdr_row_neighbours_bounded; None: the library's default)
        -> (ids [Q, k] int32, -1 behind a short list; sims [Q, k] float32, 0 there) as device tensors; nothing is read
        back."""
        if rows.dim() != 2 or rows.dtype != torch.float32 or rows.device != self.device or not rows.is_contiguous():
            raise ValueError("row_neighbours: rows must be a contiguous [n_rows, E] fp32 tensor on the engine's device")
        if queries.dim() != 1 or queries.dtype != torch.int32 or queries.device != self.device:
            raise ValueError("row_neighbours: queries must be a [Q] int32 tensor on the engine's device")
        if candidates is not None and (candidates.dim() != 1 or candidates.dtype != torch.int32 or candidates.device != self.device):
            raise ValueError("row_neighbours: candidates must be a [C] int32 tensor on the engine's device, or None")
        Q, k, n_rows = int(queries.shape[0]), int(k), int(rows.shape[0])
        if not 1 <= k <= L.KNN_MAX_K or int(rows.shape[1]) not in L.LIST_EMB_DIMS or not 1 <= n_rows < 2 ** 31:
            raise ValueError("row_neighbours: k %d (1 to %d), rows %d x %d (width one of %s)" % (
                k, L.KNN_MAX_K, n_rows, rows.shape[1], (L.LIST_EMB_DIMS,)))
        if chunk is not None and int(chunk) <= 0:
            raise ValueError("row_neighbours: chunk %r is not positive" % (chunk,))
        ids = torch.full((Q, k), -1, dtype=torch.int32, device=self.device)
        sims = torch.zeros((Q, k), dtype=torch.float32, device=self.device)
        n_cand = n_rows if candidates is None else int(candidates.shape[0])
        if Q and n_cand:
            head = (_ptr(rows), n_rows, int(rows.shape[1]), _ptr(queries.contiguous()), Q,
                    _ptr(candidates.contiguous()) if candidates is not None else None, n_cand, int(bool(exclude_self)), k,
                    _ptr(ids), _ptr(sims))
            if chunk is None:
                L.check(self._c_row_neighbours(*head, self._s()))
            else:
                L.check(self._c_row_neighbours_bounded(*head, int(chunk), self._s()))
        return ids, sims

    # ------------------------------------------------------------ baselines: co-occurrence, ItemKNN scores, ranks and lists
    # from a score matrix (no reference counterpart; the host definitions: baselines.py)
    def _check_dev(self, fn, what, t, dtype, dim):
        if t.dtype != dtype or t.device != self.device or t.dim() != dim or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %d-d %s tensor on the engine's device" % (fn, what, dim, dtype))

    def _check_hist(self, fn, off, pos):
        self._check_dev(fn, "off", off, torch.int64, 1)
        self._check_dev(fn, "pos", pos, torch.int32, 1)
        if off.shape[0] < 2:
            raise ValueError("%s: off must hold n_user + 1 >= 2 offsets" % fn)
        return int(off.shape[0]) - 1, int(pos.shape[0])

    def item_cooc(self, off, pos, m):
        """mamdr_item_cooc on the engine's stream: the histories' CSR (off [n_user + 1] int64, pos [nnz] int32 positions in
        [0, m); baselines.histories builds and checks it), device tensors -> the device tensor [m, m] int32 holding the uint32
        co-occurrence counts; nothing is read back."""
        n_user, nnz = self._check_hist("item_cooc", off, pos)
        m = int(m)
        if not 1 <= m <= L.COOC_MAX_ITEMS:
            raise ValueError("item_cooc: m %d outside 1..%d" % (m, L.COOC_MAX_ITEMS))
        cooc = torch.empty((m, m), dtype=torch.int32, device=self.device)
        L.check(self.lib.mamdr_item_cooc(_ptr(off), _ptr(pos if nnz else None), nnz, n_user, m, _ptr(cooc), self._s()))
        return cooc

    def history_scores(self, cooc, off, pos, queries, shrink):
        """mamdr_history_scores on the engine's stream: cooc [m, m] int32 (item_cooc's), the histories' CSR, queries [Q] int32
        user indices into it (one outside [0, n_user) scores all zero), 0 <= shrink <= 2^20 -> the device tensor [Q, m] fp32
        of ItemKNN scores; nothing is read back."""
        n_user, nnz = self._check_hist("history_scores", off, pos)
        self._check_dev("history_scores", "cooc", cooc, torch.int32, 2)
        self._check_dev("history_scores", "queries", queries, torch.int32, 1)
        m, Q, shrink = int(cooc.shape[0]), int(queries.shape[0]), float(shrink)
        if cooc.shape[1] != m or not 1 <= m <= L.COOC_MAX_ITEMS or not 0.0 <= shrink <= 2.0 ** 20 or n_user >= 2 ** 24:
            raise ValueError("history_scores: cooc %r (square, 1..%d), shrink %r (0 to 2^20), %d users (below 2^24)" % (
                tuple(cooc.shape), L.COOC_MAX_ITEMS, shrink, n_user))
        scores = torch.empty((Q, m), dtype=torch.float32, device=self.device)
        if Q:
            L.check(self.lib.mamdr_history_scores(_ptr(cooc), m, _ptr(off), _ptr(pos if nnz else None), nnz, n_user,
                                                  _ptr(queries), Q, shrink, _ptr(scores), self._s()))
        return scores

    def _check_scores(self, fn, scores, n_query, candidates, excl_off, excl_ids):
        """the arguments rank_scores and topk_scores share -> (row_stride, n_cand)."""
        if scores.dtype != torch.float32 or scores.device != self.device or scores.dim() not in (1, 2) or not scores.is_contiguous():
            raise ValueError("%s: scores must be a contiguous fp32 tensor [Q, n_cand] (or [n_cand]: one row for every query) on "
                             "the engine's device" % fn)
        n_cand = int(scores.shape[-1])
        if scores.dim() == 2 and int(scores.shape[0]) != n_query:
            raise ValueError("%s: %d score rows for %d queries" % (fn, scores.shape[0], n_query))
        if candidates is not None:
            self._check_dev(fn, "candidates", candidates, torch.int32, 1)
            if int(candidates.shape[0]) != n_cand:
                raise ValueError("%s: %d candidate ids for %d score columns" % (fn, candidates.shape[0], n_cand))
        if (excl_off is None) != (excl_ids is None):
            raise ValueError("%s: the exclusion lists need both their offsets and their ids" % fn)
        if excl_off is not None:
            self._check_dev(fn, "excl_off", excl_off, torch.int64, 1)
            self._check_dev(fn, "excl_ids", excl_ids, torch.int32, 1)
            if int(excl_off.shape[0]) != n_query + 1:
                raise ValueError("%s: %d exclusion offsets for %d queries" % (fn, excl_off.shape[0], n_query))
        return (n_cand if scores.dim() == 2 else 0), n_cand

    def rank_scores(self, scores, n_query, tgt_off, tgt_ids, candidates=None, excl_off=None, excl_ids=None, want_scores=False):
        """mamdr_rank_scores on the engine's stream: scores [Q, n_cand] fp32 -- or [n_cand], one row for every query --,
        candidates [n_cand] int32 ascending distinct ids or None (the id of position p is p), the exclusion lists' and the
        targets' CSR (offsets [Q + 1] int64, ids int32 ascending per query; recommend.exclusion_csr), all device tensors ->
        (ranks [T] int32: the live positions that order strictly before the target, -1 for a target that is no candidate;
        live [Q] int32 [; scores [T] fp32: the targets' raw scores]) as device tensors; nothing is read back."""
        fn = "rank_scores"
        n_query = int(n_query)
        stride, n_cand = self._check_scores(fn, scores, n_query, candidates, excl_off, excl_ids)
        self._check_dev(fn, "tgt_off", tgt_off, torch.int64, 1)
        self._check_dev(fn, "tgt_ids", tgt_ids, torch.int32, 1)
        if int(tgt_off.shape[0]) != n_query + 1:
            raise ValueError("%s: %d target offsets for %d queries" % (fn, tgt_off.shape[0], n_query))
        n_tgt = int(tgt_ids.shape[0])
        ranks = torch.empty(n_tgt, dtype=torch.int32, device=self.device)
        live = torch.zeros(n_query, dtype=torch.int32, device=self.device)
        out = torch.empty(n_tgt, dtype=torch.float32, device=self.device) if want_scores else None
        if n_query and n_cand:
            L.check(self.lib.mamdr_rank_scores(_ptr(scores), stride, n_query, _ptr(candidates), n_cand, _ptr(excl_off),
                                               _ptr(excl_ids), _ptr(tgt_off), _ptr(tgt_ids if n_tgt else None), n_tgt,
                                               _ptr(ranks if n_tgt else None), _ptr(out if n_tgt else None), _ptr(live), self._s()))
        else:
            ranks.fill_(-1)
            if out is not None:
                out.zero_()
        return (ranks, live, out) if want_scores else (ranks, live)

    def topk_scores(self, scores, n_query, k, candidates=None, excl_off=None, excl_ids=None):
        """mamdr_topk_scores on the engine's stream: rank_scores' scores / candidates / exclusion lists, 1 <= k <= 128 ->
        (ids [Q, k] int32, -1 behind a short list; scores [Q, k] fp32, 0 there) as device tensors: the first k live
        positions of rank_scores' ordering; nothing is read back."""
        fn = "topk_scores"
        n_query, k = int(n_query), int(k)
        stride, n_cand = self._check_scores(fn, scores, n_query, candidates, excl_off, excl_ids)
        if not 1 <= k <= L.SCORES_MAX_K:
            raise ValueError("%s: k %d outside 1..%d" % (fn, k, L.SCORES_MAX_K))
        ids = torch.full((n_query, k), -1, dtype=torch.int32, device=self.device)
        out = torch.zeros((n_query, k), dtype=torch.float32, device=self.device)
        if n_query and n_cand:
            L.check(self.lib.mamdr_topk_scores(_ptr(scores), stride, n_query, _ptr(candidates), n_cand, _ptr(excl_off),
                                               _ptr(excl_ids), k, _ptr(ids), _ptr(out), self._s()))
        return ids, out

    def bind_accumulator(self, acc):
        """meta-gradient accumulator of the MAML / MLDG / PCGrad meta passes (maml.py:202); optimizer="accumulate" adds
        to it (or, after set_moving_average, moves it towards every batch's gradient)."""
        self._acc = acc
        self._check(self._c_bind_accumulator(self.ctx, _ptr(acc if self._ema is None else self._ema["scratch"])))

    def set_moving_average(self, momentum):
        """average_meta_grad == "moving_mean" (maml.py:219-220): accumulate passes keep TF 1.12's zero-debiased
        moving average of the batch gradients in the bound accumulator.  Its hidden state (`biased`, `local_step`)
        lives as long as the engine, like the hidden variables of the reference's accumulator."""
        self._ema = {"momentum": float(momentum), "step": 0, "biased": self.new_vector(), "scratch": self.new_vector()}
        if self._acc is not None:
            self.bind_accumulator(self._acc)

    def set_counters(self, optimizer_steps, dropout_steps):
        """restore the Adam step count (with TF's running beta powers) and the dropout stream's position
        (mamdr_set_counters): a run resumed from saved weights / slots written into the bound vectors."""
        self._check(self._c_set_counters(self.ctx, int(optimizer_steps), int(dropout_steps)))

    def optimizer_reset(self):
        self._check(self._c_optimizer_reset(self.ctx))

    # ------------------------------------------------------------ per-domain gradients (no reference counterpart)
    def counters(self):
        """(Adam steps taken, position of the dropout stream): what set_counters restores."""
        return (int(getattr(self.lib, self.PREFIX + "optimizer_steps")(self.ctx)),
                int(getattr(self.lib, self.PREFIX + "dropout_steps")(self.ctx)))

    def domain_gradients(self, domains, n_batches=None, out=None):
        """the gradient of the total loss (L2 terms included, dropout off) at the live weights, one row per domain: row j of
        the result [len(domains), n_params] is the SUM over the first `n_batches` batches (None: the whole pass) of
        domains[j]'s train split, in file order -- exactly what that many MAMDR_OPT_ACCUMULATE steps add to a zeroed
        accumulator, plain sums even after set_moving_average.  -> (rows: fp32 device tensor, a view of `out` when given;
        steps: the batches behind each row).  `out`: a 2-D fp32 device tensor of that shape whose rows start 16-byte
        aligned (the result of an earlier call serves); it is zeroed here.
        Everything else stays as it was: weights, Adam slots, the Adam step count with its beta powers, the dropout stream's
        position (accumulate steps advance it: put back with set_counters), the aux buffer (a norm layer's moving
        statistics), the bound accumulator and the moving average's hidden state.  On the step engine a window of passes
        gathered ahead (`pregather`) is gathered again afterwards: the accumulate calls are not part of it."""
        domains = [int(d) for d in domains]
        stride = (self.n_params + 3) // 4 * 4           # every row is an accumulator: 16-byte aligned
        if out is None:
            out = torch.empty((max(len(domains), 1), stride), dtype=torch.float32, device=self.device)[:len(domains), :self.n_params]
        elif (out.dim() != 2 or tuple(out.shape) != (len(domains), self.n_params) or out.dtype != torch.float32 or
              (self.n_params > 1 and out.stride(1) != 1) or out.data_ptr() % 16 or (len(domains) > 1 and out.stride(0) % 4)):
            raise ValueError("domain_gradients: out must be an fp32 device tensor [%d, %d] with 16-byte aligned rows"
                             % (len(domains), self.n_params))
        steps = []
        for d in domains:
            total = -(-self.n_rows(d, "train") // self.batch_size)
            steps.append(total if n_batches is None else min(int(n_batches), total))
        opt_steps, drop_steps = self.counters()
        aux = self.aux.clone() if self.aux is not None else None
        acc, ema = self._acc, self._ema
        self._ema = None                                # plain sums: the moving average and its hidden state stay out of it
        try:
            for j, d in enumerate(domains):
                row = out[j]
                row.zero_()
                self._acc = row
                self._check(self._c_bind_accumulator(self.ctx, _ptr(row)))
                if steps[j]:
                    self.train_steps(d, n_steps=steps[j], optimizer="accumulate")
        finally:
            self._ema, self._acc = ema, acc
            if acc is not None:
                self.bind_accumulator(acc)
            elif self.GRAPH:
                self._check(self._c_bind_accumulator(self.ctx, _ptr(None)))        # none was bound: none is now
            else:
                self._grad_rows = out       # (the step engine cannot unbind: the last row stays bound, and alive)
            if aux is not None:
                self.aux.copy_(aux)
            self.set_counters(opt_steps, drop_steps)
            self._after_domain_gradients()
        return out, np.asarray(steps, np.int64)

    def _after_domain_gradients(self):
        pass

    # ------------------------------------------------------------ retrieval (the family's recommend / recommend_domain /
    # rank_domain / rank_slates entry points: the same argument lists on both engines, the same range checks before any launch)
    def item_rows(self):
        """the item table the live weights score with, as a DEVICE view [n_item, emb_dim] fp32: the bound frozen table, or --
        trainable tables -- the item segment of the live flat vector (the step engine's `weights` first makes the rows it
        advances lazily current: mamdr_sync_tables; the generic-layer engine steps every row with the batch).  A view, not a copy: it is read on the engine's stream before the weights change."""
        if not self.emb_trainable:
            return self.tables["item_emb"]
        off, cnt = self.segments["item_emb"]
        if cnt != self.n_item * self.emb_dim or off % 4:
            raise RuntimeError("item_rows: the item segment (%d floats at %d) is not [%d, %d] at a 16-byte offset" % (
                cnt, off, self.n_item, self.emb_dim))
        return self.weights[off:off + cnt].view(self.n_item, self.emb_dim)

    def recommend(self, uids, domains, k, candidates=None, exclude=None, want_scores=False):
        """top-K items for the queries (uids[q], domains[q]) from the live weights (mamdr_recommend: the step engine's mlp /
        wdl / deepfm; mamdr_graph_recommend: the generic-layer engine's single-output towers; no reference counterpart).
        candidates: distinct item ids (None: the whole item table); exclude: one array of item ids per query that must not be returned (any order, duplicates allowed).  -> (ids [Q, k] int32, scores [Q, k] float32
        [, all_scores [Q, n_cand]]) as numpy: by logit descending, equal logits by ascending id, scores = sigmoid(logit);
        a query with fewer than k candidates left ends in id -1 / score 0; all_scores holds 0 for an excluded pair."""
        uid = np.ascontiguousarray(np.asarray(uids).ravel(), np.int32)
        dom = np.array(np.broadcast_to(np.asarray(domains), uid.shape), np.int32)          # (a writable copy)
        if uid.size and (dom.min() < 0 or dom.max() >= self.n_domain):
            raise ValueError("recommend: user or domain id out of range")
        return self._recommend(uid, dom, None, k, candidates, exclude, want_scores)

    def recommend_domain(self, uids, domain, k, candidates=None, exclude=None, want_scores=False):
        """`recommend` with every query in the one domain `domain` (mamdr_recommend_domain: mlp / wdl / deepfm, whose
        results are `recommend`'s with a constant domain vector, byte for byte, and star, which retrieves through this call
        only: its item term depends on the domain).  Same arguments otherwise, same return contract."""
        uid = np.ascontiguousarray(np.asarray(uids).ravel(), np.int32)
        if isinstance(domain, bool) or not isinstance(domain, (int, np.integer)) or not 0 <= int(domain) < self.n_domain:
            raise ValueError("recommend_domain: domain %r is not an integer inside [0, %d)" % (domain, self.n_domain))
        return self._recommend(uid, None, int(domain), k, candidates, exclude, want_scores)

    def _retrieval_inputs(self, uid, candidates, exclude):
        """the host arrays and range checks every retrieval call shares -> (n_query, candidates int32 or None, n_cand,
        exclusion offsets, exclusion ids), the CSR None when nothing is excluded."""
        nq = int(uid.shape[0])
        if nq and (uid.min() < 0 or uid.max() >= self.n_user):
            raise ValueError("recommend: user or domain id out of range")
        cand = None
        n_cand = self.n_item
        if candidates is not None:
            cand = np.ascontiguousarray(np.asarray(candidates).ravel(), np.int32)
            n_cand = int(cand.shape[0])
            if n_cand and (cand.min() < 0 or cand.max() >= self.n_item):
                raise ValueError("recommend: candidate id out of range")
            if np.unique(cand).shape[0] != n_cand:
                raise ValueError("recommend: candidate ids must be distinct")
        off = ids = None
        if exclude is not None:
            off, ids = exclusion_csr(exclude, nq)
            if ids.size and ids.max() >= self.n_item:
                raise ValueError("recommend: excluded item id out of range")
            ids = ids if ids.size else np.zeros(1, np.int32)       # (a non-null pointer for an all-empty list)
        return nq, cand, n_cand, off, ids

    def rank_domain(self, uids, domain, targets, candidates=None, exclude=None, want_scores=False):
        """exact ranks (mamdr_rank_domain) of `targets` -- one array of item ids per query, any order, duplicates allowed: made
        ascending and distinct as `exclude` is -- among the candidates, every query in the one domain `domain`, from the
        live weights.  candidates / exclude: as recommend_domain.  -> {"offsets" [Q + 1] int64, "ids" [T] int32 (the targets'
        CSR), "ranks" [T] int32: the live candidates that order strictly before the pair (higher logit, or equal logit and
        smaller id), "listed" [T] bool: the target is a candidate and not excluded for its query (only then is its rank its
        0-based position in the query's ordering), "live" [Q] int32: live candidates per query [, "scores" [T]: sigmoid(logit)
        of the pair]} as numpy.  Every range check runs before the launch."""
        uid = np.ascontiguousarray(np.asarray(uids).ravel(), np.int32)
        if isinstance(domain, bool) or not isinstance(domain, (int, np.integer)) or not 0 <= int(domain) < self.n_domain:
            raise ValueError("rank_domain: domain %r is not an integer inside [0, %d)" % (domain, self.n_domain))
        nq, cand, n_cand, off, ids = self._retrieval_inputs(uid, candidates, exclude)
        t_off, t_ids = exclusion_csr(targets, nq, "targets")
        if t_ids.size and t_ids.max() >= self.n_item:
            raise ValueError("rank_domain: target item id out of range")
        n_tgt = int(t_ids.shape[0])
        in_cand = np.ones(n_tgt, bool) if cand is None else np.isin(t_ids, cand)
        listed = in_cand.copy()
        if off is not None:
            for q in range(nq):
                sl = slice(t_off[q], t_off[q + 1])
                listed[sl] &= ~np.isin(t_ids[sl], ids[off[q]:off[q + 1]])
        dev = lambda a: torch.from_numpy(a).to(self.device) if a is not None else None      # noqa: E731
        d_uid, d_cand, d_off, d_ids, d_toff = dev(uid), dev(cand), dev(off), dev(ids), dev(t_off)
        d_tids = dev(t_ids if n_tgt else np.zeros(1, np.int32))
        ranks = torch.empty(max(n_tgt, 1), dtype=torch.int32, device=self.device)
        live = torch.empty(max(nq, 1), dtype=torch.int32, device=self.device)
        scores = torch.empty(max(n_tgt, 1), dtype=torch.float32, device=self.device) if want_scores else None
        self._check(getattr(self.lib, self.PREFIX + "rank_domain")(
            self.ctx, int(domain), nq, _ptr(d_uid), _ptr(d_cand), n_cand, _ptr(d_off), _ptr(d_ids), _ptr(d_toff), _ptr(d_tids),
            _ptr(ranks), _ptr(scores), _ptr(live)))
        res = {"offsets": t_off, "ids": t_ids, "ranks": ranks.cpu().numpy()[:n_tgt], "listed": listed,
               "live": live.cpu().numpy()[:nq]}
        if want_scores:
            res["scores"] = scores.cpu().numpy()[:n_tgt]
        return res

    def rank_slates(self, uids, domain, slates, want_order=False):
        """every query's own candidate slate scored and ordered (mamdr_rank_slates): `slates` is one array of DISTINCT item
        ids per query, kept in the caller's order (a slate may be empty), every query in the one domain `domain`, from the
        live weights.  -> {"offsets" [Q + 1] int64, "ids" [E] int32 (the slates' CSR), "scores" [E] float32: sigmoid(logit)
        of the pair -- the bits rank_domain and recommend_domain give it --, "pos" [E] int32: the entries of the same slate
        that order strictly before the entry (higher logit, or equal logit and smaller id), a permutation of 0 .. L - 1 per
        slate [, "order" [E] int32: order[offsets[q] + pos[j]] = j - offsets[q], the slate-local index of the entry at each
        position]} as numpy.  Every check runs before the launch: the work is sum of the slates' lengths pairs, and
        O(L^2) integer compares per slate -- a whole catalogue is rank_domain's job."""
        uid = np.ascontiguousarray(np.asarray(uids).ravel(), np.int32)
        if isinstance(domain, bool) or not isinstance(domain, (int, np.integer)) or not 0 <= int(domain) < self.n_domain:
            raise ValueError("rank_slates: domain %r is not an integer inside [0, %d)" % (domain, self.n_domain))
        nq = int(uid.shape[0])
        off, ids = slates_csr(slates, nq)
        if nq and (uid.min() < 0 or uid.max() >= self.n_user):
            raise ValueError("rank_slates: user id out of range")
        if ids.size and ids.max() >= self.n_item:
            raise ValueError("rank_slates: item id out of range")
        n_ent = int(ids.shape[0])
        res = {"offsets": off, "ids": ids}
        if nq == 0 or n_ent == 0:
            res.update(scores=np.zeros(0, np.float32), pos=np.zeros(0, np.int32))
            if want_order:
                res["order"] = np.zeros(0, np.int32)
            return res
        d_uid, d_off, d_ids = (torch.from_numpy(a).to(self.device) for a in (uid, off, ids))
        scores = torch.empty(n_ent, dtype=torch.float32, device=self.device)
        pos = torch.empty(n_ent, dtype=torch.int32, device=self.device)
        order = torch.empty(n_ent, dtype=torch.int32, device=self.device) if want_order else None
        self._check(getattr(self.lib, self.PREFIX + "rank_slates")(
            self.ctx, int(domain), nq, _ptr(d_uid), _ptr(d_off), _ptr(d_ids), _ptr(scores), _ptr(pos), _ptr(order)))
        res.update(scores=scores.cpu().numpy(), pos=pos.cpu().numpy())
        if want_order:
            res["order"] = order.cpu().numpy()
        return res

    def _recommend(self, uid, dom, domain, k, candidates, exclude, want_scores):
        """the marshalling of both retrieval calls: dom [Q] int32 per query (mamdr_recommend) or None and the host integer
        `domain` (mamdr_recommend_domain).  Every range check runs before the launch."""
        nq, cand, n_cand, off, ids = self._retrieval_inputs(uid, candidates, exclude)
        dev = lambda a: torch.from_numpy(a).to(self.device) if a is not None else None      # noqa: E731
        d_uid, d_dom, d_cand, d_off, d_ids = dev(uid), dev(dom), dev(cand), dev(off), dev(ids)
        kk = max(int(k), 1)
        out_ids = torch.empty((max(nq, 1), kk), dtype=torch.int32, device=self.device)
        out_scores = torch.empty((max(nq, 1), kk), dtype=torch.float32, device=self.device)
        all_scores = torch.empty((max(nq, 1), max(n_cand, 1)), dtype=torch.float32, device=self.device) if want_scores else None
        tail = (_ptr(d_cand), n_cand, _ptr(d_off), _ptr(d_ids), int(k), _ptr(out_ids), _ptr(out_scores), _ptr(all_scores))
        if domain is None:
            self._check(getattr(self.lib, self.PREFIX + "recommend")(self.ctx, nq, _ptr(d_uid), _ptr(d_dom), *tail))
        else:
            self._check(getattr(self.lib, self.PREFIX + "recommend_domain")(self.ctx, domain, nq, _ptr(d_uid), *tail))
        res = (out_ids.cpu().numpy()[:nq, :int(k)], out_scores.cpu().numpy()[:nq, :int(k)])
        return res + (all_scores.cpu().numpy()[:nq, :n_cand],) if want_scores else res


class TowerEngine(DeviceEngine):
    PREFIX, KERAS_NAMES = "mamdr_", KERAS_NAMES

    def __init__(self, n_user, n_item, n_domain, batch_size, dropout=0.5, emb_trainable=False,
                 tower="mlp", emb_dim=128, hidden=(256, 128, 64), l2_emb=1e-5, device=None,
                 dropout_seed=1024, l2_linear=1e-5, uncertainty_weight=False, tower_tile=None, adam_beta1=0.9, adam_beta2=0.999):
        """tower_tile: rows per tower workgroup (mamdr_set_tower_tile: 0 automatic, 4, 16); None = automatic, except for an
        engine built on a lane of a parallel.LaneGroup of four or more lanes, which takes 16 (it shares the CUs with the
        other lanes' launches).  adam_beta1 / adam_beta2: the compiled Adam's betas (tf.train.AdamOptimizer's defaults)."""
        self._open(device, n_user, n_item, n_domain, batch_size, dropout_seed, emb_trainable)
        tower_id = {"mlp": L.TOWER_MLP, "deepfm": L.TOWER_DEEPFM, "star": L.TOWER_STAR, "wdl": L.TOWER_WDL,
                    "pnn": L.TOWER_PNN, "nfm": L.TOWER_NFM}[tower]
        max_batch = (self.batch_size + 15) // 16 * 16
        cfg = L.Config(L.ABI_VERSION, tower_id, self.n_user, self.n_item, self.n_domain, emb_dim,
                       (C.c_int32 * 3)(*hidden), max_batch, 1 if emb_trainable else 0, float(dropout),
                       float(l2_emb), float(l2_linear), float(adam_beta1), float(adam_beta2), 1e-8,
                       1 if uncertainty_weight else 0)
        self.eval_batch = max_batch
        handle = C.c_void_p()
        L.check(self.lib.mamdr_create(C.byref(cfg), C.c_void_p(self.stream.cuda_stream), C.byref(handle)))
        self.ctx = handle
        if tower_tile is None:
            from . import parallel
            group = parallel.lanes()
            # (the PNN / NFM modes exist in the four-row tower only)
            tower_tile = 16 if (group is not None and group.n >= 4 and tower in ("mlp", "deepfm", "wdl")) else 0
        if tower_tile:
            self.set_tower_tile(tower_tile)
        self.tower, self.emb_dim = tower, int(emb_dim)
        self.n_params = int(self.lib.mamdr_param_count(self.ctx))
        # theta / phi vectors cover the META prefix only (all of it except for the Star tower)
        self.n_meta = int(self.lib.mamdr_meta_count(self.ctx))
        self.segments = {}
        for seg, name in enumerate(L.SEG_NAMES):
            off, cnt = C.c_int64(), C.c_int64()
            L.check(self.lib.mamdr_param_segment(self.ctx, seg, C.byref(off), C.byref(cnt)))
            if cnt.value:
                self.segments[name] = (off.value, cnt.value)
        # (Star: PartitionedNorm's moving statistics, initial mean 0 / variance 1 per domain)
        self._bind_buffers(self.n_domain * 3 * emb_dim)

    # The live state is only handed out synchronised: with trainable tables the library advances rows that
    # no batch touched lazily (mamdr_sync_tables in include/mamdr_hip.h); every read or replacement of the
    # bound vectors from the host side goes through these properties.
    def sync(self):
        L.check(self.lib.mamdr_sync_tables(self.ctx))

    @property
    def weights(self):
        self.sync()
        return self._weights

    @property
    def adam_m(self):
        self.sync()
        return self._adam_m

    @property
    def adam_v(self):
        self.sync()
        return self._adam_v

    def keras_key(self):
        return self.tower, None, ()

    def pack(self, named):
        """PNN: deepctr's first kernel [387, 256] is given as ONE tensor "W0"; its last three rows (the inner products')
        live in segment "W0x"."""
        if "W0x" in self.segments and "W0x" not in named:
            w0 = np.asarray(named["W0"], np.float32).reshape(-1, 256)
            named = dict(named, W0=w0[:384], W0x=w0[384:])
        return DeviceEngine.pack(self, named)

    def unpack(self, vec):
        out = DeviceEngine.unpack(self, vec)
        if "W0x" in out:           # PNN: the caller's view is deepctr's one kernel [387, 256]
            out["W0"] = np.concatenate([out["W0"], out.pop("W0x")])
        return out

    def set_weights(self, vec):
        """SetVarOp.__call__ (utils/tool.py:36-45): device copy into the live weights.  A vector of
        meta length assigns the meta prefix only (MAML._set_model_meta_parms, maml.py:181-187)."""
        dst = self.meta_weights if (self.meta_off and vec.numel() == self.n_meta) else self.weights
        L.check(self.lib.mamdr_copy(_ptr(dst), _ptr(vec), vec.numel(), self._s()))

    def get_weights(self, out=None):
        """K.batch_get_value (maml.py:189-194): snapshot of the live weights."""
        if out is None:
            out = torch.empty_like(self.weights)
        L.check(self.lib.mamdr_copy(_ptr(out), _ptr(self.weights), self.n_params, self._s()))
        return out

    def segment_shapes(self):
        """{segment: (slices along the last axis, slice length)} of the Keras variables behind the segments --
        what numpy's axis=-1 reductions in the reference's PCGrad see (model_zoo/pcgrad.py:152-160)."""
        D = self.n_domain
        out = {}
        for name, (off, cnt) in self.segments.items():
            if name in ("user_emb", "item_emb", "domain_emb"):
                out[name] = (cnt // 128, 128)
            elif name in ("W0", "Ws0"):
                out[name] = (cnt // 256, 256)          # (NFM's first kernel has 128 rows)
            elif name == "W0x":
                out[name] = (3, 256)
            elif name in ("W1", "Ws1"):
                out[name] = (256, 128)
            elif name in ("W2", "Ws2"):
                out[name] = (128, 64)
            elif name in ("Wd0", "Wd1", "Wd2"):
                cols = {"Wd0": 256, "Wd1": 128, "Wd2": 64}[name]
                out[name] = (cnt // cols, cols)
            elif name in ("bd0", "bd1", "bd2", "pn_gamma_spec", "pn_beta_spec"):
                out[name] = (D, cnt // D)
            elif name in ("wo", "lin_user", "lin_item", "lin_domain", "log_var", "gb"):
                out[name] = (cnt, 1)
            else:                                  # 1-d biases and PartitionedNorm shared vectors
                out[name] = (1, cnt)
        return out

    def set_tower_tile(self, rows):
        L.check(self.lib.mamdr_set_tower_tile(self.ctx, int(rows)))

    def tower_tile(self, batch=None):
        """rows per tower workgroup of a training step of `batch` rows (4: k_tower4, 16: k_tower)."""
        rows = int(self.lib.mamdr_tower_tile(self.ctx, int(batch or self.batch_size)))
        if rows < 0:                    # (an error code is not a tile size: ADVICE r05)
            L.check(rows)
        return rows

    def dr_advance(self, phi, merged, theta, gamma, method="plus", assign_model=True):
        """FlatVectorOps.dr_advance on the context's live weights (mamdr_dr_advance_live): the library synchronises them
        itself, and a domain-table step the fused step path left pending is materialised inside the same launch."""
        mode = {"plus": L.MERGE_PLUS, "times": L.MERGE_TIMES}[method]
        holes = bool(self.meta_holes) and assign_model
        L.check(self.lib.mamdr_dr_advance_live(self.ctx, _ptr(phi), _ptr(merged), _ptr(theta), float(gamma), mode,
                                               1 if (assign_model and not holes) else 0, self.meta_off, phi.numel()))
        if holes:
            self.assign_meta(merged)

    def pregather(self, passes, batch_size=None):
        """hint (mamdr_pregather_passes): the next train_steps calls run these passes -- [(domain, perm device tensor or
        None[, pass_rows])] -- in this order; where a call would gather its pass's rows itself (frozen tables, fused
        step path) the library gathers them all in one launch now.  Same rows, same bits; a no-op elsewhere."""
        n = len(passes)
        self._window = (list(passes), batch_size) if n else None       # (keeps the permutations alive: _after_domain_gradients)
        if n == 0:                 # forget an earlier hint
            L.check(self.lib.mamdr_pregather_passes(self.ctx, 0, None, None, None, int(batch_size or self.batch_size)))
            return
        doms = (C.c_int32 * n)(*[int(p[0]) for p in passes])
        perms = (C.c_void_p * n)(*[(p[1].data_ptr() if p[1] is not None else None) for p in passes])
        rows = (C.c_int64 * n)(*[(-1 if len(p) < 3 or p[2] is None else int(p[2])) for p in passes])
        L.check(self.lib.mamdr_pregather_passes(self.ctx, n, doms, perms, rows, int(batch_size or self.batch_size)))

    _window = None

    def _after_domain_gradients(self):
        """the accumulate calls of domain_gradients are no part of an announced window and made the library drop it: the
        window is announced -- and gathered -- again, so the passes that follow find their rows as before."""
        if self._window is not None:
            self.pregather(*self._window)

    def pregather_ahead(self, passes, batch_size=None, spread_steps=0):
        """hint (mamdr_pregather_ahead): `passes` is the window AFTER the current one -- the list the next `pregather`
        will get, once `spread_steps` more steps of the fused path have run.  Rider workgroups of those steps gather it
        meanwhile; `pregather` with the same list only gathers what they did not reach.  Same rows, same bits; a no-op
        wherever `pregather` is one, and on a device without idle CUs."""
        n = len(passes)
        doms = (C.c_int32 * n)(*[int(p[0]) for p in passes])
        perms = (C.c_void_p * n)(*[(p[1].data_ptr() if p[1] is not None else None) for p in passes])
        rows = (C.c_int64 * n)(*[(-1 if len(p) < 3 or p[2] is None else int(p[2])) for p in passes])
        L.check(self.lib.mamdr_pregather_ahead(self.ctx, n, doms, perms, rows, int(batch_size or self.batch_size),
                                               int(spread_steps)))

    def gather(self, domain, split, perm=None, first_row=0, n_rows=None, out=None):
        n = self.n_rows(domain, split) if n_rows is None else n_rows
        if out is None:
            out = torch.empty((n, 384), dtype=torch.float32, device=self.device)
        split_id = {"train": L.SPLIT_TRAIN, "val": L.SPLIT_VAL, "test": L.SPLIT_TEST}[split]
        L.check(self.lib.mamdr_gather_rows(self.ctx, domain, split_id, _ptr(perm), first_row, n, _ptr(out)))
        return out

    def step_kernel_names(self, batch=None):
        """names of the kernels behind profile_read's FWD_BWD / WGRAD / UPDATE slots for a step of `batch` rows."""
        fused = int(self.lib.mamdr_step_path(self.ctx, int(batch or self.batch_size))) == 1
        return {L.KERNEL_FWD_BWD: "k_tower<train>", L.KERNEL_WGRAD: "k_wgrad_adam" if fused else "k_wgrad",
                L.KERNEL_UPDATE: "k_dm_finish (when the live table is read)" if fused else "k_update"}

    # ------------------------------------------------------------ profiling
    def profile(self, enable):
        L.check(self.lib.mamdr_profile_enable(self.ctx, 1 if enable else 0))

    def profile_reset(self):
        L.check(self.lib.mamdr_profile_reset(self.ctx))

    def profile_read(self, kernel):
        ms, cnt = C.c_double(), C.c_int64()
        L.check(self.lib.mamdr_profile_read(self.ctx, kernel, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


def shuffle_perm(n, buffer_size, seed):
    """host: tf.data shuffle-buffer order (utils/dataset.py:27-37) via the C ABI."""
    out = np.empty(n, np.int32)
    L.check(L.load().mamdr_shuffle_perm(n, buffer_size, seed & 0xFFFFFFFFFFFFFFFF, out.ctypes.data))
    return out
