"""PCGrad's projection (model_zoo/pcgrad.py:152-160) held to the reference's numpy on EVERY tower, on the device.

The projection reduces every Keras variable along its last axis: the one outer operation that depends on the
variables' shapes.  Three things decide those shapes on the device -- `TowerEngine.segment_shapes`,
`GraphEngine.segment_shapes` and `k_pcgrad` behind `mamdr_pcgrad_project` -- and before this file only the mlp tower
with frozen tables on the step engine ran them on a GPU.  Here:

1. the kernel against vectors from the reference's own method at every shape family (tests/golden/
   pcgrad_shape_goldens.npz: every regime of numpy's pairwise summation, 1-d / 3-d / [n, 1] variables, all-zero and equal
   rows, rows with denormal products / dot product / squared norm whose projection still shows), bit for bit, at
   16-byte aligned and at back-to-back (odd) tensor starts, in one call / calls of 1 / calls of 24 tensors; what the entry point refuses stays refused and writes nothing;
2. `segment_shapes()` of every engine against the table of Keras variables (tests/keras_variables.py);
3. one `meta.pcgrad_epoch` per engine on real gradients (untouched table rows are exact zeros, dead units zero columns):
   every device projection against `oracle.outer.pcgrad_project` over views shaped by that table, bit for bit;
4. one AutoInt PCGrad epoch against the oracle (its attention kernels are four variables [d, 32] per tensor);
5. `shared_bottom_pcgrad` (47 tensors on 10 domains), `autoint_pcgrad` and a 4-layer Star form (25 tensors) through
   `cli.build_model`: more tensors than one `mamdr_pcgrad_project` call takes.

Sizes: synthetic Taobao-10 at scale 0.05 with 3 domains, batches of 64 rows -- nothing at workload size.
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import keras_variables as KV                    # noqa: E402
import star_forms_ref as sref                   # noqa: E402
from oracle import fmnets as ofm                # noqa: E402
from oracle import loops as oloops              # noqa: E402
from oracle import mtl as omtl                  # noqa: E402
from oracle import outer as oouter              # noqa: E402
from oracle import rng as orng                  # noqa: E402
from oracle import star as ostar                # noqa: E402
from oracle import tower as otower              # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H3 = (256, 128, 64)
BATCH, SEQ, AUX_PLAN = 64, [1, 0, 2], {1: [0, 2], 0: [2, 1], 2: [1]}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from mamdr_amd import engine, synthetic
    return engine, synthetic


def counting_perm_fn(sizes):
    """the shuffles of one epoch: the k-th pass over any domain draws with seed 2000 + k (as test_pcgrad_epoch_matches_oracle)"""
    counter = [0]

    def perm_fn(d):
        counter[0] += 1
        return orng.shuffle_perm(sizes[d], 10000, seed=2000 + counter[0])
    return perm_fn


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


# ====================================================================================================
# 1. the kernel against the reference's own method at every shape family
@pytest.fixture(scope="module")
def flat_ops(env):
    """an engine for its stateless flat-vector entry points (the tower behind it is never stepped)"""
    eng = env[0].TowerEngine(64, 32, 3, BATCH)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "pcgrad_shape_goldens.npz"))


def layout(G, aligned):
    """[(offset, slices, slice length)] of the goldens in one flat vector: 16-byte aligned tensor starts, or tensors back
    to back behind one leading float (odd offsets, as the engines' own vectors have behind `gb`) -- and its length"""
    tensors, off = [], 0 if aligned else 1
    for i in range(int(G["n_tensors"])):
        a = G["current_%d" % i]
        cols = a.shape[-1]
        tensors.append((off, a.size // cols, cols))
        off += (a.size + 3) // 4 * 4 if aligned else a.size
    return tensors, off + 5


def flat_of(G, prefix, tensors, n, device):
    v = np.full(n, 7.0, F32)                   # (what lies between and behind the tensors must stay as it is)
    for i, (o, r, c) in enumerate(tensors):
        v[o:o + r * c] = G["%s_%d" % (prefix, i)].ravel()
    return torch.from_numpy(v).to(device)


def chunks(tensors, k):
    return [tensors] if k is None else [tensors[i:i + k] for i in range(0, len(tensors), k)]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "packed_odd"])
def test_kernel_matches_reference_goldens_at_every_shape(flat_ops, G, aligned):
    """two successive projections, the bits of `final` and `aux` after each; the whole list through pcgrad_project (more than
    24 tensors: several calls), in calls of 1 tensor and in calls of 24 -- identical bytes."""
    eng = flat_ops
    tensors, n = layout(G, aligned)
    assert len(tensors) > 24
    if not aligned:
        assert any(o % 4 for o, _, _ in tensors) and any(o % 2 for o, _, _ in tensors)
    runs = {}
    for k in (None, 1, 24):
        fin = flat_of(G, "current", tensors, n, eng.device)
        out = []
        for tag in ("aux1", "aux2"):
            aux = flat_of(G, tag, tensors, n, eng.device)
            for part in chunks(tensors, k):
                eng.pcgrad_project(fin, aux, part)
            torch.cuda.synchronize()
            out.append((fin.cpu().numpy().copy(), aux.cpu().numpy().copy()))
        runs[k] = out
    covered = np.zeros(n, bool)
    for o, r, c in tensors:
        covered[o:o + r * c] = True
    bad = []
    for step, (fh, ah) in zip(("after1", "after2"), runs[None]):
        for i, (o, r, c) in enumerate(tensors):
            for name, h in (("final", fh), ("aux", ah)):
                want = G["%s_%s_%d" % (step, name, i)].ravel()
                if not same_bits(h[o:o + r * c], want):
                    rows = np.nonzero((h[o:o + r * c].view(np.uint32) != want.view(np.uint32)).reshape(r, c).any(axis=1))[0]
                    bad.append((step, name, i, G["current_%d" % i].shape, int(G["kinds"][i]), rows[:8].tolist()))
        assert (fh[~covered] == 7.0).all() and (ah[~covered] == 7.0).all()
    assert not bad, bad
    for k in (1, 24):
        for (f0, a0), (f1, a1) in zip(runs[None], runs[k]):
            assert same_bits(f0, f1) and same_bits(a0, a1), k


def test_one_call_equals_chunked_calls_at_24_tensors(flat_ops, G):
    """a list the entry point takes in ONE call (the first 24 tensors) against calls of 1 and of 7 tensors"""
    eng = flat_ops
    tensors, n = layout(G, False)
    tensors = tensors[:24]
    got = {}
    for k in (None, 1, 7):
        fin, aux = flat_of(G, "current", tensors, n, eng.device), flat_of(G, "aux1", tensors, n, eng.device)
        for part in chunks(tensors, k):
            offs, rows, cols = (C.c_int64 * len(part))(*[t[0] for t in part]), (C.c_int64 * len(part))(*[t[1] for t in part]), \
                (C.c_int32 * len(part))(*[t[2] for t in part])
            assert eng.lib.mamdr_pcgrad_project(C.c_void_p(fin.data_ptr()), C.c_void_p(aux.data_ptr()), offs, rows, cols,
                                                len(part), eng._s()) == 0
        torch.cuda.synchronize()
        got[k] = (fin.cpu().numpy().copy(), aux.cpu().numpy().copy())
    for k in (1, 7):
        assert same_bits(got[None][0], got[k][0]) and same_bits(got[None][1], got[k][1]), k
    for i, (o, r, c) in enumerate(tensors):
        assert same_bits(got[None][0][o:o + r * c], G["after1_final_%d" % i].ravel()), i


def test_refusals_stay_refusals_and_write_nothing(flat_ops):
    """cols of 0 and of 4097, negative rows, a negative offset, more than 24 tensors, null pointers: MAMDR_EINVAL before
    anything is launched (the table is checked as a whole: a good tensor in front of a bad one is not projected either)."""
    from mamdr_amd import _lib as L
    eng = flat_ops
    rs = np.random.RandomState(3)
    c0 = np.abs(rs.standard_normal(3 * 4097 + 64)).astype(F32)          # (every dot product positive: a launch would project)
    a0 = np.abs(rs.standard_normal(c0.size)).astype(F32)
    fin, aux = torch.from_numpy(c0).to(eng.device), torch.from_numpy(a0).to(eng.device)
    pf, pa = C.c_void_p(fin.data_ptr()), C.c_void_p(aux.data_ptr())

    def call(tensors, fin_p=pf, aux_p=pa, null=None, n=None):
        k = len(tensors)
        arrs = [(C.c_int64 * k)(*[t[0] for t in tensors]), (C.c_int64 * k)(*[t[1] for t in tensors]),
                (C.c_int32 * k)(*[t[2] for t in tensors])]
        if null is not None:
            arrs[null] = None
        return eng.lib.mamdr_pcgrad_project(fin_p, aux_p, arrs[0], arrs[1], arrs[2], k if n is None else n, eng._s())

    good = (0, 2, 16)
    cases = {"cols 0": [good, (32, 2, 0)], "cols 4097": [good, (32, 2, 4097)], "cols -1": [good, (32, 2, -1)],
             "rows -1": [good, (32, -1, 16)], "offset -4": [good, (-4, 2, 16)], "25 tensors": [(16 * i, 1, 16) for i in range(25)]}
    for what, tensors in cases.items():
        assert call(tensors) == L.EINVAL, what
    assert call([good], n=-1) == L.EINVAL
    assert call([good], fin_p=C.c_void_p(0)) == L.EINVAL and call([good], aux_p=C.c_void_p(0)) == L.EINVAL
    for null in range(3):
        assert call([good], null=null) == L.EINVAL, null
    torch.cuda.synchronize()
    assert same_bits(fin.cpu().numpy(), c0) and same_bits(aux.cpu().numpy(), a0)
    # ... and the engine's method raises where the entry point refuses
    with pytest.raises(L.MamdrError) as ei:
        eng.pcgrad_project(fin, aux, [good, (32, 2, 4097)])
    assert ei.value.code == L.EINVAL
    # the limits themselves are served: 4096 columns, 0 rows, 0 tensors, 24 tensors
    assert call([(0, 1, 4096), (4096, 0, 16)]) == 0 and call([]) == 0 and call([(16 * i, 1, 16) for i in range(24)]) == 0
    torch.cuda.synchronize()
    assert not same_bits(fin.cpu().numpy()[:4096], c0[:4096])


# ====================================================================================================
# 2. / 3. every engine: its shape table, and the projection on real gradients
def _step(tower, trainable, uncertainty=False):
    return ("step", tower, dict(emb_trainable=trainable, uncertainty=uncertainty))


ENGINES = ([_step(t, tr) for t in ("mlp", "deepfm", "wdl", "pnn", "nfm", "star") for tr in (False, True)]
           + [_step("mlp", False, True)]
           + [("graph", "mlp", dict(hidden=h, emb_dim=e)) for h, e in (((128, 64), 128), ((256, 128, 64, 64), 128),
                                                                       ((128, 64), 32), ((128, 64), 64), ((128, 64), 256))]
           + [("graph", k, dict(hidden=H3, emb_dim=128)) for k in ("nfm", "pnn", "ccpm", "autoint")]
           + [("graph_star", f, {}) for f in (("pn", "star", 64, H3), ("bn", "dense", 0, H3), ("pn", "star", 64, (256, 128, 64, 64)))]
           + [("graph_mtl", k, {}) for k in ("shared_bottom", "mmoe", "ple")])


def _id(case):
    fam, kind, opt = case
    kind = kind if isinstance(kind, str) else "-".join("x".join(map(str, k)) if isinstance(k, tuple) else str(k) for k in kind)
    return "-".join([fam, kind] + ["%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v)
                                   for k, v in sorted(opt.items()) if v not in (False, 128, H3)])


_DATA = {}


def problem(synthetic, emb_dim=128):
    if emb_dim not in _DATA:
        shape = dict(synthetic.SHAPES["taobao10"], n_domain=3)
        _DATA[emb_dim] = synthetic.generate(shape, batch_size=BATCH, seed=7, scale=0.05, emb_dim=emb_dim, splits=("train",))
    return _DATA[emb_dim]


def create(env, case, nu, ni, D):
    """-> (engine, the table of its Keras variables, initial tensors by name)"""
    from mamdr_amd import graph_engine
    fam, kind, opt = case
    rs = np.random.RandomState(11)
    if fam == "step":
        tr, uw = opt["emb_trainable"], opt["uncertainty"]
        eng = env[0].TowerEngine(nu, ni, D, BATCH, dropout=0.0 if kind == "star" else 0.5, emb_trainable=tr, tower=kind,
                                 uncertainty_weight=uw)
        if kind == "star":
            return eng, KV.star(nu, ni, D, emb_trainable=tr), ostar.init_params(rs, nu, ni, D)
        init = ofm.init_params(rs, kind, nu, ni, D) if kind in ("pnn", "nfm") else otower.init_params(rs, nu, ni, D)
        return eng, KV.deepctr(kind, nu, ni, D, emb_trainable=tr, uncertainty=uw), init
    if fam == "graph":
        hidden, E = opt["hidden"], opt["emb_dim"]
        eng = graph_engine.GraphEngine(kind, nu, ni, D, BATCH, hidden, (), dropout=0.5, emb_dim=E)
        if kind in ("ccpm", "autoint"):
            init = ofm.init_params_conv(rs, kind, nu, ni, D, hidden=hidden)
        elif kind in ("nfm", "pnn"):
            init = ofm.init_params(rs, kind, nu, ni, D, hidden=hidden)
        else:
            init = otower.init_params(rs, nu, ni, D, emb_dim=E, hidden=hidden)
        return eng, KV.deepctr(kind, nu, ni, D, E, hidden), init
    if fam == "graph_star":
        norm, dense, aux, hidden = kind
        eng = graph_engine.GraphEngine("star", nu, ni, D, BATCH, hidden, (), dropout=0.0, norm=norm, dense=dense, auxiliary_dim=aux)
        return eng, KV.star(nu, ni, D, 128, hidden, False, norm, dense, aux), sref.init_params(rs, nu, ni, D, hidden, norm, dense, aux)
    eh, th, gh, ne, se, sp = KV.MTL_SHAPES[kind]
    eng = graph_engine.GraphEngine(kind, nu, ni, D, BATCH, eh, th, gh, num_experts=ne, shared_expert_num=se,
                                   specific_expert_num=sp, dropout=0.5)
    spec = omtl.Spec(kind, D, eh, th, gh, num_experts=ne, shared_expert_num=se, specific_expert_num=sp)
    return eng, KV.mtl(kind, nu, ni, D, eh, th, gh, ne, se, sp), omtl.init_params(rs, spec, nu, ni)


def check_shape_table(eng, table):
    """segment_shapes() == the table's (slices, slice length) per tensor; the tensors lie in the flat vector in ascending,
    non-overlapping ranges with less than 16 bytes between two of them"""
    want = KV.engine_slices(table, eng.segments)
    got = eng.segment_shapes()
    assert set(got) == set(want) == set(eng.segments), (sorted(got), sorted(want), sorted(eng.segments))
    wrong = {n: (got[n], want[n]) for n in want if tuple(got[n]) != tuple(want[n])}
    assert not wrong, wrong
    for n, (off, cnt) in eng.segments.items():
        assert cnt == want[n][0] * want[n][1], (n, cnt, want[n])
    spans = sorted((off, cnt, n) for n, (off, cnt) in eng.segments.items())
    for (o0, c0, n0), (o1, c1, n1) in zip(spans, spans[1:]):
        assert o0 + c0 <= o1, (n0, n1)
    assert spans[-1][0] + spans[-1][1] <= eng.n_params


@pytest.mark.parametrize("case", ENGINES, ids=_id)
def test_segment_shapes_equal_the_keras_table(env, case):
    """create only"""
    eng, table, _ = create(env, case, 203, 101, 3)
    try:
        check_shape_table(eng, table)
    finally:
        eng.close()


class _Lib(object):
    """the library with mamdr_pcgrad_project's host tables recorded on their way through"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mamdr_pcgrad_project(self, fin, aux, offs, rows, cols, n, stream):
        self.calls.append([(int(offs[i]), int(rows[i]), int(cols[i])) for i in range(n)])
        return self._lib.mamdr_pcgrad_project(fin, aux, offs, rows, cols, n, stream)


def run_epoch_and_check(env, case, meta_from=None):
    """one meta.pcgrad_epoch; every device projection against oracle.outer.pcgrad_project over the table's views.
    meta_from: a tensor name -- the meta range starts there (a `meta_parms` selection that leaves the tables out)."""
    from mamdr_amd import meta
    fam, kind, opt = case
    g = problem(env[1], opt.get("emb_dim", 128))
    nu, ni, D = g["n_user"], g["n_item"], g["n_domain"]
    eng, table, init = create(env, case, nu, ni, D)
    try:
        check_shape_table(eng, table)
        init["user_emb"], init["item_emb"] = g["tables"]["user_emb"].copy(), g["tables"]["item_emb"].copy()
        if "user_emb" not in eng.segments:
            eng.bind_table("user_emb", init["user_emb"])
            eng.bind_table("item_emb", init["item_emb"])
        for d in range(D):
            c = g["data"]["train"][d]
            eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
        eng.set_weights(eng.pack(init))
        if meta_from is not None:
            lo = eng.segments[meta_from][0]
            eng.set_meta_range(lo, eng.n_params - lo)
        lo, hi = eng.meta_off, eng.meta_off + eng.n_meta
        slices_of = KV.engine_slices(table, eng.segments)
        inside = [n for n, (off, cnt) in eng.segments.items() if off >= lo and off + cnt <= hi]
        assert inside and (meta_from is None or (len(inside) < len(eng.segments)) == (lo > 0))
        eng.lib = lib = _Lib(eng.lib)
        real, seen = eng.pcgrad_project, []

        def recorded(final, aux, tensors=None):
            torch.cuda.synchronize()
            before = (final.cpu().numpy().copy(), aux.cpu().numpy().copy())
            n_calls = len(lib.calls)
            real(final, aux, tensors)
            torch.cuda.synchronize()
            seen.append((before, (final.cpu().numpy().copy(), aux.cpu().numpy().copy()), lib.calls[n_calls:]))

        eng.pcgrad_project = recorded
        sizes = [g["data"]["train"][d]["uid"].shape[0] for d in range(D)]
        cur, aux = eng.new_vector(), eng.new_vector()
        trace = meta.pcgrad_epoch(eng, meta.OuterAdamState(eng), cur, aux, SEQ, AUX_PLAN, counting_perm_fn(sizes), BATCH, lr=1e-3,
                                  meta_lr=0.003)
        torch.cuda.synchronize()
        assert [t[0] for t in trace].count("pcgrad_aux") == len(seen) == sum(len(v) for v in AUX_PLAN.values())
        pos = neg = 0
        for (c0, a0), (c1, a1), calls in seen:
            # every tensor of the meta range exactly once, nothing else, no call above the cap
            sent = [t for call in calls for t in call]
            assert all(len(call) <= 24 for call in calls) and len(calls) == -(-len(inside) // 24), [len(c) for c in calls]
            assert sorted(sent) == sorted((eng.segments[n][0],) + tuple(slices_of[n]) for n in inside)
            want_c, want_a = c0.copy(), a0.copy()
            vc, va = [], []
            for n in inside:
                off, cnt = eng.segments[n]
                vc.append(want_c[off:off + cnt].reshape(slices_of[n]))
                va.append(want_a[off:off + cnt].reshape(slices_of[n]))
                dots = np.sum(vc[-1] * va[-1], axis=-1)
                pos, neg = pos + int((dots > 0).sum()), neg + int((dots <= 0).sum())
            with np.errstate(all="ignore"):
                oouter.pcgrad_project(vc, va)
            # the whole vectors: the tensors as numpy leaves them, everything outside the meta range (and the padding) untouched
            bad = [n for n in eng.segments if not same_bits(c1[slice(*_span(eng, n))], want_c[slice(*_span(eng, n))])
                   or not same_bits(a1[slice(*_span(eng, n))], want_a[slice(*_span(eng, n))])]
            assert not bad, bad
            assert same_bits(c1, want_c) and same_bits(a1, want_a)
            assert np.any(c0[lo:hi]) and np.any(a0[lo:hi])
        assert pos > 0 and neg > 0, (pos, neg)
        print("PCGRAD_TOWERS %s tensors=%d in_meta=%d calls_per_projection=%d projections=%d slices_dot_pos=%d slices_dot_le0=%d"
              % (_id(case) + ("" if meta_from is None else "-meta_from=" + meta_from), len(eng.segments), len(inside),
                 len(seen[0][2]), len(seen), pos, neg))
    finally:
        eng.close()


def _span(eng, name):
    off, cnt = eng.segments[name]
    return off, off + cnt


@pytest.mark.parametrize("case", ENGINES, ids=_id)
def test_projection_on_real_gradients_matches_numpy(env, case):
    run_epoch_and_check(env, case)


def test_projection_under_a_meta_range_without_the_tables(env):
    """trainable tables outside `meta_parms` (n_meta != n_params, meta.py: the projection walks the meta parameters only):
    the tables' gradients in both vectors stay as the passes left them"""
    run_epoch_and_check(env, _step("deepfm", True), meta_from="domain_emb")


def test_projection_over_every_tensor_of_the_step_star_tower(env):
    """the step engine's Star tower projects its meta prefix by default (tables, shared kernels and biases: the reference's
    Star filter); under `meta_parms` ["all"] the 3-d specific kernels [D, in, out], the specific biases and PartitionedNorm's
    vectors project too -- the rows of the hand-written shape table no default run reaches"""
    run_epoch_and_check(env, _step("star", True), meta_from="user_emb")


# ====================================================================================================
# 4. one AutoInt PCGrad epoch against the oracle
def test_autoint_pcgrad_epoch_matches_oracle():
    """as tests/test_gpu_parity.py::test_pcgrad_epoch_matches_oracle, on the tower whose attention kernels are four Keras
    variables per tensor: equal trace, weights within that test's bars (assert_adam_close: 3 outer Adam steps at 0.003)."""
    from mamdr_amd import meta
    from test_gpu_fmnets import make_problem
    from test_gpu_parity import assert_adam_close
    g, eng, model = make_problem("autoint", batch=256, dropout=0.5, scale=0.3)
    sizes = [g["data"]["train"][d]["uid"].shape[0] for d in range(g["n_domain"])]
    tr_o = oloops.pcgrad_epoch(model, otower.OuterAdam(model.get_flat().size), g["data"]["train"], SEQ, AUX_PLAN,
                               counting_perm_fn(sizes), 256, 0.003)
    cur, aux = eng.new_vector(), eng.new_vector()
    tr_g = meta.pcgrad_epoch(eng, meta.OuterAdamState(eng), cur, aux, SEQ, AUX_PLAN, counting_perm_fn(sizes), 256, lr=1e-3, meta_lr=0.003)
    assert tr_g == tr_o
    got = eng.unpack(eng.get_weights())
    for name in model.names:
        assert_adam_close(got[name], model.params[name], 3, 0.003, name, max_frac=2e-3)
    eng.close()


# ====================================================================================================
# 5. registry names with more tensors than one call takes, through build_model
def _config(tmp_path, cfg_file, name, **model):
    """the reference's PCGrad config (its train section carries the wrapper's keys) around `cfg_file`'s model section"""
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_pcgrad_taobao_10.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    with open(os.path.join(ROOT, "config", "Taobao-10", cfg_file)) as f:
        cfg["model"] = copy.deepcopy(json.load(f)["model"])
    cfg["model"].update(name=name, **model)
    cfg["train"].update(epoch=1, patience=1, sample_num=2, meta_learning_rate=0.003, meta_parms=["all"],
                        result_save_path=str(tmp_path / "result"), checkpoint_path=str(tmp_path / "ckpt"))
    cfg["dataset"].update(batch_size=256, synthetic="taobao10", synthetic_scale=0.05)
    return cfg


@pytest.mark.parametrize("which", ["shared_bottom_pcgrad", "autoint_pcgrad", "star_pcgrad_4_layers"])
def test_pcgrad_names_run_an_epoch_through_build_model(env, tmp_path, which):
    """no registry name reaches MAMDR_EINVAL from inside an epoch: shared_bottom on 10 domains has 47 tensors, the 4-layer
    Star form 25"""
    from mamdr_amd import cli
    from mamdr_amd.utils import dataset as mds
    if which == "shared_bottom_pcgrad":
        cfg, n_min = _config(tmp_path, "shared_bottom.json", which), 47
    elif which == "autoint_pcgrad":
        cfg, n_min = _config(tmp_path, "deepctr_DN+DR.json", which), 9
    else:
        cfg, n_min = _config(tmp_path, "star_taobao.json", "star_pcgrad", hidden_dim=[256, 128, 64, 64], auxiliary_net=True), 25
    model = cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]))
    eng = model.model
    assert len(eng.segments) >= n_min, len(eng.segments)
    eng.lib = lib = _Lib(eng.lib)
    before = eng.get_weights().cpu().numpy().copy()
    model.train()
    after = eng.get_weights().cpu().numpy()
    assert [t[0] for t in model.trace].count("pcgrad_aux") == 20 and lib.calls
    assert all(len(call) <= 24 for call in lib.calls)
    assert len(lib.calls) == 20 * -(-len(eng.segments) // 24)
    assert np.isfinite(after).all() and not np.array_equal(before, after)
    eng.close()
