"""What tests/test_config_scalars_host.py (CPU) and tests/test_gpu_config_scalars.py (GPU) share: the values off the
defaults, the problems, the oracle calls and the ONE comparison helper both files judge with (tests only).

Three config scalars cross the C ABI into every training step (`mamdr_config`, `mamdr_graph_config`): `dropout`, `l2_emb`,
`l2_linear`.  At the configs' values distinct quantities coincide: at rate 1/2 the drop rate IS the keep probability
(1 / (1 - rate) == 1 / rate == 2, rate 2^32 == (1 - rate) 2^32, and multiplying by 2 is exact), and l2_emb == l2_linear ==
1e-5.  The values here break both ties.

Values.  L2 = (1e-5, 3e-5): l2_emb stays at the reference's 1e-5 (deepctr.py:118), l2_linear is three times it, so a
swapped pair changes a table's gradient by 4e-5 p and a linear table's by -4e-5 p against bars of 2e-6 max|g| (below).
RATES = (0.25, 0.75): float32 holds both exactly, so threshold and keep scale are exact (2^30, 3 2^30; 4/3, 4) and
1 / rate, (1 - rate) 2^32 of one rate are the other's values -- the mutants are as far from the truth as a kernel that
confuses the two would be.

Bars (= tests/test_gpu_parity.py::test_deepfm_gradients_adam_eval and the files beside it):
  gradient   |got - want| <= rtol |want| + atol, rtol 2e-4, atol max(2e-6 max(max|want|, 1e-3), floor of the tensor)
  floor      a gradient read back as w0 - (w0 - g) at lr 1 is quantised to the weights' grid: w0 - g rounds with an error
             of at most half an ulp of the tensor's largest |w0|, and the subtraction that recovers g adds as much at
             most -> one ulp of max|w0| (`ulp_floor`; 6e-8 for table values up to 0.5, 7.5e-9 for kernels ~0.1: the
             literals of the existing files).  0 where nothing is read back through a weight.
  loss       |got - want| <= 2e-6 max(1, |want|)
  Adam slots from zero, step count 0: m against (1 - beta1) g, v against (1 - beta2) g^2, computed in fp32: rtol 2e-4
             (4e-4 for v: g enters squared), atol 2e-6 max|want|, no floor (nothing is quantised to a weight's ulp)
"""
import contextlib

import numpy as np

from oracle import fmnets as ofm
from oracle import mtl as omtl
from oracle import rng as orng
from oracle import tower as otower

F32 = np.float32
L2 = (1e-5, 3e-5)
DEFAULT_L2 = (1e-5, 1e-5)
RATES = (0.25, 0.75)
BATCH = 256
HIDDEN = (256, 128, 64)
RTOL = 2e-4
TOWER_KINDS = ("mlp", "deepfm", "wdl")
FM_KINDS = ("nfm", "pnn", "ccpm", "autoint")
MTL_KINDS = ("shared_bottom", "mmoe", "ple")
# (expert_hidden, tower_hidden, gate_hidden, num_experts, shared_expert_num, specific_expert_num): tests/test_gpu_mtl.py's
MTL_SHAPES = {"shared_bottom": ((256, 128), (64,), (), 0, 0, 0),
              "mmoe": ((128, 64), (64,), (64,), 3, 0, 0),
              "ple": ((128,), (64,), (64,), 0, 2, 2)}
LINEAR_KINDS = ("deepfm", "wdl", "nfm", "ccpm", "autoint")          # towers with the three 1-d linear tables
TABLES = ("user_emb", "item_emb", "domain_emb")
LIN_TABLES = ("lin_user", "lin_item", "lin_domain")
_GEN = {}


def family(kind):
    return "tower" if kind in TOWER_KINDS else ("fm" if kind in FM_KINDS else "mtl")


def generate(kind, emb_dim=128, scale=0.05, seed=7):
    """Taobao-10 synthetic at 256 rows per batch (4 domains for the multi-task kinds), generated once per shape."""
    from mamdr_amd import synthetic
    D = 4 if family(kind) == "mtl" else 10
    key = (D, emb_dim, scale, seed)
    if key not in _GEN:
        _GEN[key] = synthetic.generate(dict(synthetic.SHAPES["taobao10"], n_domain=D), batch_size=BATCH, seed=seed, scale=scale,
                                       emb_dim=emb_dim)
    return _GEN[key]


class Problem(object):
    """one tower's initial tensors off their special values (non-zero biases, domain table and linear tables, as the existing
    GPU files set them up) and its oracle model built with the l2 pair and the rate."""

    def __init__(self, kind, emb_trainable=False, rate=0.25, l2=L2, emb_dim=128, hidden=HIDDEN, uncertainty=False, seed=7):
        self.kind, self.emb_trainable, self.rate, self.l2 = kind, bool(emb_trainable), float(rate), l2
        self.emb_dim, self.hidden, self.uncertainty = emb_dim, tuple(hidden), bool(uncertainty)
        self.family = family(kind)
        g = self.g = generate(kind, emb_dim, seed=seed)
        D = self.D = g["n_domain"]
        rs = np.random.RandomState(seed)
        self.spec = None
        if self.family == "mtl":
            eh, th, gh, ne, se, sp = MTL_SHAPES[kind]
            self.spec = omtl.Spec(kind, D, eh, th, gh, num_experts=ne, shared_expert_num=se, specific_expert_num=sp)
            p = omtl.init_params(rs, self.spec, g["n_user"], g["n_item"])
            for n in p:
                if "/b" in n or n.endswith("/gb") or n == "domain_emb":
                    p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
        else:
            if kind in ("ccpm", "autoint"):
                p = ofm.init_params_conv(rs, kind, g["n_user"], g["n_item"], D, hidden=self.hidden)
                if kind == "ccpm":
                    p["conv1_b"] = (rs.standard_normal(4) * 0.1).astype(F32)
                    p["conv2_b"] = (rs.standard_normal(4) * 0.1).astype(F32)
                else:
                    for l in range(3):
                        p["att%d_w" % l] = (p["att%d_w" % l] * 4).astype(F32)
            elif self.family == "fm":
                p = ofm.init_params(rs, kind, g["n_user"], g["n_item"], D, hidden=self.hidden)
            else:
                p = otower.init_params(rs, g["n_user"], g["n_item"], D, emb_dim=emb_dim, hidden=self.hidden)
            p["domain_emb"] = (rs.standard_normal(p["domain_emb"].shape) * 0.05).astype(F32)
            for n in ["b%d" % l for l in range(len(self.hidden))] + list(LIN_TABLES):
                p[n] = (rs.standard_normal(p[n].shape) * 0.05).astype(F32)
            p["gb"] = np.array([0.1], F32)
            if not emb_trainable:       # frozen linear tables stay at their zero initialisation (deepctr: same feature column)
                p["lin_user"][...] = 0
                p["lin_item"][...] = 0
            if uncertainty:
                p["log_var"] = (1.0 + rs.uniform(-0.3, 0.3, D)).astype(F32)
        p["user_emb"], p["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        self.params = p
        self.model = self.make_model(l2)
        self.names = list(self.model.names)
        # the largest domain: its pass has a full first batch and a partial last one
        self.d = max(range(D), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
        self.cols = g["data"]["train"][self.d]
        self.n = self.cols["uid"].shape[0]
        self.perm = orng.shuffle_perm(self.n, 10000, seed=11)
        self.n_step = -(-self.n // BATCH)
        assert self.n_step >= 2 and self.n % BATCH, "the pass needs a full and a partial batch"

    def make_model(self, l2, dropout_seed=1024):
        """the oracle model over a COPY of the initial tensors; l2 None: the oracle's own constants."""
        p = {k: v.copy() for k, v in self.params.items()}
        if self.family == "mtl":
            return omtl.OracleMTL(p, self.spec, emb_trainable=self.emb_trainable, dropout=self.rate, lr=1e-3,
                                  dropout_seed=dropout_seed, l2=l2)
        if self.family == "fm":
            return ofm.OracleNet(p, self.kind, emb_trainable=self.emb_trainable, dropout=self.rate, lr=1e-3, hidden=self.hidden,
                                 dropout_seed=dropout_seed, uncertainty=self.uncertainty, l2=l2)
        kw = {} if l2 is None else dict(l2_emb=l2[0], l2_linear=l2[1])
        return otower.OracleModel(p, emb_trainable=self.emb_trainable, dropout=self.rate, lr=1e-3, hidden=self.hidden,
                                  dropout_seed=dropout_seed, tower=self.kind, uncertainty=self.uncertainty, **kw)

    def batch(self, step):
        idx = self.perm[step * BATCH:(step + 1) * BATCH]
        return {k: self.cols[k][idx] for k in ("uid", "pid", "domain", "label")}

    def grads(self, step, drop_step, train=True, model=None, l2="model"):
        """(loss, {tensor: gradient of its shape}) of batch `step` of the pass with the masks of dropout position
        `drop_step`; train False: learning phase 0 (the accumulate pass).  l2 "model": the model's own pair."""
        m = model or self.model
        b = self.batch(step)
        rate = self.rate if train else 0.0
        l2 = m.l2 if l2 == "model" else l2
        args = (b["uid"], b["pid"], b["domain"], b["label"])
        rows = b["uid"].shape[0]
        if self.family == "mtl":
            masks = omtl.train_masks(self.spec, m.seed, drop_step, rows, rate) if rate > 0 else None
            loss, g, _ = omtl.loss_and_grads(m.params, self.spec, self.d, *args, masks, rate, self.emb_trainable, m.frozen_sumsq(), l2)
        elif self.family == "fm":
            masks = otower.train_masks(m.seed, drop_step, rows, self.hidden, rate) if rate > 0 else None
            fn = ofm.loss_and_grads_conv if self.kind in ("ccpm", "autoint") else ofm.loss_and_grads
            loss, g, _ = fn(m.params, self.kind, *args, masks, rate, self.emb_trainable, m.frozen_sumsq(), self.uncertainty, l2)
        else:
            masks = otower.train_masks(m.seed, drop_step, rows, self.hidden, rate) if rate > 0 else None
            loss, g, _ = otower.loss_and_grads(m.params, *args, masks, rate, self.emb_trainable, m.frozen_sumsq(), m.deepfm,
                                               self.uncertainty, l2)
        return float(loss), {k: np.asarray(otower.bigtable.densify(v) if hasattr(v, "dense") else v, F32) for k, v in g.items()}

    def touched(self, step):
        """{table-like tensor: boolean mask over its ELEMENTS of the rows batch `step` gathers}"""
        b = self.batch(step)
        out = {}
        for emb, lin, ids in (("user_emb", "lin_user", b["uid"]), ("item_emb", "lin_item", b["pid"]),
                              ("domain_emb", "lin_domain", b["domain"])):
            rows = np.zeros(self.params[emb].shape[0], bool)
            rows[ids] = True
            out[emb] = np.repeat(rows, self.params[emb].shape[1])
            if lin in self.params:
                out[lin] = rows
        return out


# ---------------------------------------------------------------- the comparison helper
def ulp_floor(w):
    """one ulp of the tensor's largest weight (module docstring: `floor`)."""
    w = np.asarray(w, F32)
    return float(np.spacing(F32(np.abs(w).max()))) if w.size else 0.0


def beyond(got, want, floor=0.0, rtol=RTOL):
    """boolean per element: outside the gradient bar."""
    got, want = np.asarray(got, F32).ravel(), np.asarray(want, F32).ravel()
    atol = max(2e-6 * max(float(np.abs(want).max()) if want.size else 0.0, 1e-3), floor)
    return ~(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= atol + rtol * np.abs(want.astype(np.float64)))


def loss_excess(got, want):
    """|got - want| in units of the loss bar 2e-6 max(1, |want|)."""
    return abs(float(got) - float(want)) / (2e-6 * max(1.0, abs(float(want))))


class Report(object):
    """per tensor: the fraction of its elements (of `select[name]` where given) beyond the bar; the loss in units of its bar."""

    def __init__(self, got, want, loss_got, loss_want, floors=None, select=None):
        self.frac, self.worst = {}, {}
        for name, w in want.items():
            bad = beyond(got[name], w, (floors or {}).get(name, 0.0))
            if select is not None and name in select:
                bad = bad[select[name]]
            self.frac[name] = float(bad.mean()) if bad.size else 0.0
        self.loss = loss_excess(loss_got, loss_want)

    def ok(self):
        return self.loss <= 1.0 and not any(self.frac.values())

    def rejected(self, name):
        """when a mutant counts as rejected on a tensor: at least half of the tensor beyond its bar, or the loss beyond 10 x its bar."""
        return self.frac[name] >= 0.5 or self.loss > 10.0

    def __repr__(self):
        return "loss %.3g x bar; beyond the bar: %s" % (self.loss, " ".join("%s %.3g" % kv for kv in sorted(self.frac.items()) if kv[1]))


def assert_matches(got, want, loss_got, loss_want, floors=None, what=""):
    rep = Report(got, want, loss_got, loss_want, floors)
    print("%s loss got %.8f want %.8f (%.3f x bar)" % (what, loss_got, loss_want, rep.loss))
    assert rep.ok(), (what, rep)
    return rep


def slot_beyond(got, want, rtol):
    got, want = np.asarray(got, F32).ravel(), np.asarray(want, F32).ravel()
    atol = 2e-6 * (float(np.abs(want).max()) if want.size else 0.0)
    return ~(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= atol + rtol * np.abs(want.astype(np.float64)))


def assert_slots(m, v, grads, beta1=0.9, beta2=0.999, what=""):
    """one Adam step from zero slots: m = (1 - beta1) g, v = (1 - beta2) g^2 in fp32, every element of every tensor."""
    omb1, omb2 = F32(F32(1) - F32(beta1)), F32(F32(1) - F32(beta2))
    for name, g in grads.items():
        g = np.asarray(g, F32).ravel()
        bm = slot_beyond(m[name], (g * omb1).astype(F32), RTOL)
        bv = slot_beyond(v[name], ((g * g).astype(F32) * omb2).astype(F32), 2 * RTOL)
        assert not bm.any() and not bv.any(), (what, name, float(bm.mean()), float(bv.mean()), int(np.flatnonzero(bm | bv)[0]))


# ---------------------------------------------------------------- the mutants (oracles, on the CPU)
@contextlib.contextmanager
def mutated(which):
    """"keep_scale": the keep scale from 1 / rate; "mask": the mask from u >= (1 - rate) 2^32.  Both are looked up in
    oracle/rng.py at call time by every oracle, so replacing them there mutates tower, fmnets and mtl alike."""
    name = {"keep_scale": "keep_scale", "mask": "dropout_threshold"}[which]
    real = getattr(orng, name)
    if which == "keep_scale":
        fake = lambda rate: F32(1.0 / orng.abi_rate(rate))                          # noqa: E731
    else:
        fake = lambda rate: real(1.0 - orng.abi_rate(rate))                         # noqa: E731
    setattr(orng, name, fake)
    try:
        yield
    finally:
        setattr(orng, name, real)


def l2_mutants(l2):
    return {"l2 swapped": (l2[1], l2[0]), "l2_emb dropped": (0.0, l2[1]), "l2_linear dropped": (l2[0], 0.0)}


def carriers(problem, mutant, grads):
    """the tensors that carry the mutated term, among those the step has a gradient for."""
    emb = [n for n in TABLES if n in grads]
    lin = [n for n in LIN_TABLES if n in grads] if problem.kind in LINEAR_KINDS else []
    if mutant == "l2_emb dropped":
        return emb
    if mutant == "l2_linear dropped":
        return lin
    if mutant == "l2 swapped":
        return emb + lin
    return sorted(grads)            # dropout: every tensor's gradient passes through the masked, scaled activations
