"""The oracle's PCGrad views held to the table of Keras variable shapes (tests/keras_variables.py), and the host side
of `FlatVectorOps.pcgrad_project` (no GPU).

The reference's projection reduces every variable along its last axis (model_zoo/pcgrad.py:152-160), so
`oracle.loops.tensor_views` must cut the flat vector into exactly the table's slices, for every oracle model: the
step towers, the four generic single towers, both Star oracles and the multi-task towers.  AutoInt is the case that
used to differ: `att<l>_w` [d, 128] is four variables [d, 32].
"""
import ctypes as C

import numpy as np
import pytest

import keras_variables as KV
import star_forms_ref as sref
from oracle import fmnets as ofm
from oracle import loops as oloops
from oracle import mtl as omtl
from oracle import outer as oouter
from oracle import star as ostar
from oracle import tower as otower

F32 = np.float32
NU, NI, D = 11, 7, 3


def oracle_and_table(case):
    """-> (oracle model, table) of one case: (family, kind, options)"""
    family, kind, opt = case
    rs = np.random.RandomState(1)
    tr, uw = opt.get("emb_trainable", False), opt.get("uncertainty", False)
    if family == "tower":
        E, hidden = opt.get("emb_dim", 128), opt.get("hidden", (256, 128, 64))
        model = otower.OracleModel(otower.init_params(rs, NU, NI, D, E, hidden), emb_trainable=tr, hidden=hidden, tower=kind,
                                   uncertainty=uw)
        return model, KV.deepctr(kind, NU, NI, D, E, hidden, tr, uw)
    if family == "fmnets":
        init = ofm.init_params_conv if kind in ("ccpm", "autoint") else ofm.init_params
        model = ofm.OracleNet(init(rs, kind, NU, NI, D), kind, emb_trainable=tr, **({"uncertainty": True} if uw else {}))
        return model, KV.deepctr(kind, NU, NI, D, emb_trainable=tr, uncertainty=uw)
    if family == "star":
        return ostar.OracleStar(ostar.init_params(rs, NU, NI, D), emb_trainable=tr), KV.star(NU, NI, D, emb_trainable=tr)
    if family == "star_forms":
        norm, dense, aux, hidden = kind
        p = sref.init_params(rs, NU, NI, D, hidden, norm, dense, aux)
        return (sref.StarForms(p, norm, dense, aux, emb_trainable=tr),
                KV.star(NU, NI, D, 128, hidden, tr, norm, dense, aux))
    eh, th, gh, ne, se, sp = KV.MTL_SHAPES[kind]
    spec = omtl.Spec(kind, D, eh, th, gh, num_experts=ne, shared_expert_num=se, specific_expert_num=sp)
    return (omtl.OracleMTL(omtl.init_params(rs, spec, NU, NI), spec, emb_trainable=tr),
            KV.mtl(kind, NU, NI, D, eh, th, gh, ne, se, sp, emb_trainable=tr))


CASES = ([("tower", k, {"emb_trainable": t}) for k in ("mlp", "wdl", "deepfm") for t in (False, True)]
         + [("tower", "mlp", {"uncertainty": True}), ("tower", "deepfm", {"emb_trainable": True, "uncertainty": True}),
            ("tower", "mlp", {"emb_dim": 32, "hidden": (128, 64)}), ("tower", "wdl", {"emb_dim": 256, "hidden": (256, 128, 64, 64)})]
         + [("fmnets", k, {"emb_trainable": t}) for k in ("nfm", "pnn", "ccpm", "autoint") for t in (False, True)]
         + [("fmnets", "autoint", {"uncertainty": True}), ("fmnets", "pnn", {"uncertainty": True})]
         + [("star", "star", {"emb_trainable": t}) for t in (False, True)]
         + [("star_forms", f, {}) for f in (("pn", "star", 64, (256, 128, 64)), ("bn", "dense", 0, (256, 128, 64)),
                                            ("none", "star", 0, (128, 64)), ("pn", "star", 64, (256, 128, 64, 64)))]
         + [("star_forms", ("pn", "dense", 64, (256, 128, 64)), {"emb_trainable": True})]
         + [("mtl", k, {"emb_trainable": t}) for k in ("shared_bottom", "mmoe", "ple") for t in (False, True)])


def _id(case):
    family, kind, opt = case
    kind = kind if isinstance(kind, str) else "x".join(str(k) if not isinstance(k, tuple) else "-".join(map(str, k)) for k in kind)
    return "-".join([family, kind] + ["%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v)
                                      for k, v in sorted(opt.items())])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_oracle_tensor_views_equal_the_keras_table(case):
    """names, order, offsets, sizes and the (slices, slice length) of every view: the table's."""
    model, table = oracle_and_table(case)
    assert list(model.names) == [t.name for t in table]
    n = model.get_flat().size
    assert n == table[-1].offset + KV.size(table[-1].shape) < 2 ** 24          # (the marker below is exact in fp32)
    flat = np.arange(n, dtype=F32)
    views = oloops.tensor_views(model, flat)
    assert len(views) == len(table)
    for v, t in zip(views, table):
        assert v.base is not None and np.shares_memory(v, flat), t.name          # a view: the projection writes through it
        assert v.size == KV.size(t.shape) and int(v.ravel()[0]) == t.offset, (t.name, v.shape, t)
        rows, cols = KV.slices(t.shape)
        assert (v.size // v.shape[-1], v.shape[-1]) == (rows, cols), (t.name, v.shape, t.shape)
        assert np.array_equal(v.reshape(rows, cols), flat[t.offset:t.offset + v.size].reshape(rows, cols)), t.name


def test_autoint_slices_are_rows_of_one_variable():
    """what the table's [4 d, 32] claims: slice 4 i + j of the row-major [d][128] tensor is row i of variable j (W_query,
    W_key, W_value, W_res) -- and the projection over the table's views is the reference's rule applied to the four
    variables separately, which slices of 128 are not."""
    rs = np.random.RandomState(5)
    d = 6
    cur, aux = (rs.standard_normal((2, d, 128)) * 0.01).astype(F32)
    four = [[x[:, 32 * j:32 * (j + 1)].copy() for j in range(4)] for x in (cur, aux)]
    oouter.pcgrad_project(four[0], four[1])
    got_c, got_a = cur.copy(), aux.copy()
    oouter.pcgrad_project([got_c.reshape(4 * d, 32)], [got_a.reshape(4 * d, 32)])      # (views: written through)
    assert np.array_equal(got_c, np.concatenate(four[0], axis=1)) and np.array_equal(got_a, np.concatenate(four[1], axis=1))
    wide_c, wide_a = cur.copy(), aux.copy()
    oouter.pcgrad_project([wide_c], [wide_a])
    assert not np.array_equal(wide_c, got_c)


def test_denormal_golden_rows_tell_a_flushing_kernel_apart(golden_dir):
    """the committed goldens' `denormal_dot` / `denormal_norm` rows (tests/golden/make_pcgrad_shape_goldens.py): products
    and dot product below fp32's smallest normal (the squared norm too in the second), AND a projection that moves the
    auxiliary gradient -- so that a projection with any of them flushed to zero (dot 0: nothing projected; norm 0: a
    division by zero) leaves other bytes than the goldens hold.  The row at scale 1e-20 cannot tell: nothing moves there."""
    import os
    G = np.load(os.path.join(golden_dir, "pcgrad_shape_goldens.npz"))
    tiny, kinds = np.finfo(F32).tiny, list(G["kinds"])
    names = ("cur_zero", "aux_zero", "dot_neg", "dot_pos", "equal", "scale_1e-20", "denormal_dot", "denormal_norm")
    seen = []
    for i in [i for i, k in enumerate(kinds) if k != -1]:
        n = G["current_%d" % i].shape[-1]
        for r, kind in enumerate(names) if kinds[i] == -2 else [(0, names[kinds[i]])]:
            cur, a1, after = (G["%s_%d" % (k, i)].reshape(-1, n)[r] for k in ("current", "aux1", "after1_aux"))
            moved = (after.view(np.uint32) != a1.view(np.uint32)).mean()
            if kind == "scale_1e-20":
                assert moved == 0
            if not kind.startswith("denormal"):
                continue
            prod, dot, nrm2 = cur * a1, np.sum(cur * a1), np.sum(cur * cur)
            assert 0 < np.abs(prod).max() < tiny and 0 < dot < tiny, (i, r, kind)
            assert (0 < nrm2 < tiny) if kind == "denormal_norm" else nrm2 > tiny, (i, r, kind, nrm2)
            assert moved > 0.9, (i, r, kind, moved)
            flushed = np.where(np.abs(prod) < tiny, F32(0), prod)          # what a kernel that flushes denormals would sum
            assert not np.sum(flushed) > 0
            seen.append((n, kind))
    assert sorted(set(seen)) == [(64, "denormal_dot"), (64, "denormal_norm"), (128, "denormal_dot"), (128, "denormal_norm"),
                                 (384, "denormal_dot"), (384, "denormal_norm")]


class _Lib(object):
    """records mamdr_pcgrad_project's host tables; refuses what the library refuses"""

    def __init__(self):
        self.calls = []

    def mamdr_pcgrad_project(self, fin, aux, offs, rows, cols, n, stream):
        from mamdr_amd import _lib as L
        if n > L.PCG_MAX_SEG:
            return L.EINVAL
        self.calls.append([(offs[i], rows[i], cols[i]) for i in range(n)])
        return 0


@pytest.mark.parametrize("n", [0, 1, 23, 24, 25, 47, 48, 49, 117])
def test_pcgrad_project_sends_any_table_in_calls_of_at_most_24(n):
    """the whole list, in order, every tensor exactly once, no call above the library's cap (shared_bottom on 10 domains
    has 47 tensors, a 4-layer Star form 25)."""
    torch = pytest.importorskip("torch")
    from mamdr_amd import _lib as L
    from mamdr_amd.engine import FlatVectorOps
    ops = FlatVectorOps.__new__(FlatVectorOps)
    ops.lib, ops._s = _Lib(), lambda: C.c_void_p(0)
    tensors = [(7 * i, i + 1, 1 + i % 5) for i in range(n)]
    v = torch.zeros(8)
    ops.pcgrad_project(v, v.clone(), tensors)
    assert [t for call in ops.lib.calls for t in call] == tensors
    assert all(len(call) <= L.PCG_MAX_SEG for call in ops.lib.calls)
    assert len(ops.lib.calls) == max(1, -(-n // L.PCG_MAX_SEG))


def test_slices_beyond_the_kernels_reach_are_refused_at_build_model(tmp_path, monkeypatch):
    """the one combination PCGrad rules out -- a variable with more than 4096 elements along its last axis (a hidden
    layer that wide) -- raises NotImplementedError when the model is built, naming the tensor; 4096 itself builds."""
    from fake_engine import FakeEngine
    from mamdr_amd import cli
    from mamdr_amd.model_zoo import PCGrad
    from mamdr_amd.utils import dataset as mds
    from test_host_logic import patch_emb_dim, tiny_config
    patch_emb_dim(monkeypatch)
    cfg = tiny_config(tmp_path, "mlp_pcgrad")
    ds = mds.MultiDomainDataset(cfg["dataset"])

    def factory(width):
        class Shaped(FakeEngine):
            def segment_shapes(self):
                return {n: ((1, width) if n == "b0" else (c, 1)) for n, (o, c) in self.segments.items()}
        return Shaped

    assert type(cli.build_model(cfg, ds, factory(4096))) is PCGrad
    with pytest.raises(NotImplementedError, match="b0"):
        cli.build_model(cfg, ds, factory(4097))
    assert type(cli.build_model(tiny_config(tmp_path, "mlp_meta_maml"), ds, factory(4097))) is not PCGrad      # (PCGrad's limit only)
