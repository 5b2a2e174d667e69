"""Host side of the Star family (CPU): routing of every norm / dense / auxiliary_net combination, the library's argument
checks with no device present, Keras names and the reference's name filters, the several-process limit of `bn`, and the
wrappers' loops on a CPU stand-in of GraphEngine("star", ...) (tests/star_forms_ref.fake_star_graph)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import star_forms_ref as sref
from fake_engine import FakeEngine, FakeStarEngine, fake_factory
from mamdr_amd import cli, parallel
from mamdr_amd.utils import dataset as mds
from test_host_logic import tiny_config


def star_factory(*args, **kw):
    """an injected factory that offers the generic-layer Star forms (and the step form, and the mlp tower)."""
    star_factory.calls.append((args, kw))
    return fake_factory(*args, **kw)


def _star_graph(*args, **kw):
    star_factory.graph_calls.append((args, kw))
    return sref.fake_star_graph(*args, **kw)


star_factory.star_graph = _star_graph
star_factory.graph = fake_factory.graph
star_factory.calls, star_factory.graph_calls = [], []


def star_config(tmp_path, name="star", norm="pn", dense="star", aux=False, hidden=(64, 64), epochs=2):
    cfg = tiny_config(tmp_path, name, epochs)
    for k in ("user_dim", "item_dim", "domain_dim"):
        cfg["model"][k] = 128
    cfg["model"].update(norm=norm, dense=dense, auxiliary_net=aux, auxiliary_dim=hidden[-1], hidden_dim=list(hidden))
    cfg["train"].update(meta_parms=["emb", "kernel_shared", "bias_shared"])
    return cfg


@pytest.mark.parametrize("norm,dense,aux", list(itertools.product(("none", "pn", "bn"), ("dense", "star"), (False, True))))
def test_routing_of_every_combination(tmp_path, monkeypatch, norm, dense, aux):
    monkeypatch.delenv("MAMDR_STAR_ENGINE", raising=False)
    hidden = (256, 128, 64)
    cfg = star_config(tmp_path, "star", norm, dense, aux, hidden)
    ds = mds.MultiDomainDataset(cfg["dataset"])
    star_factory.calls, star_factory.graph_calls = [], []
    m = cli.build_model(cfg, ds, star_factory)
    eng = m.model
    if (norm, dense, aux) == ("pn", "star", False):         # the step kernels' form
        assert isinstance(eng, FakeStarEngine) and not star_factory.graph_calls
        assert star_factory.calls[0][1]["tower"] == "star"
    elif (norm, dense, aux) == ("none", "dense", False):    # the mlp tower
        assert type(eng) is FakeEngine and eng.tower == "mlp" and not star_factory.graph_calls
    else:
        (args, kw), = star_factory.graph_calls
        assert args[0] == "star" and not star_factory.calls
        assert kw["norm"] == norm and kw["dense"] == dense and kw["auxiliary_dim"] == (64 if aux else 0)
        assert kw["expert_hidden"] == hidden and kw["dropout"] == 0.0 and kw["emb_dim"] == 128
        assert eng.created_with["norm"] == norm and list(eng.segments) == list(eng.oracle.names)
        assert (eng.aux is None) == (norm == "none")
        if norm == "bn":
            assert eng.aux.numel() == 2 * 384 and float(eng.aux[384:].sum()) == 384.0
        if norm == "pn":
            assert eng.aux.numel() == (4 * 3 * 384 + 3 + 3) // 4 * 4


def test_hidden_dims_and_the_parity_twin_switch(tmp_path, monkeypatch):
    monkeypatch.delenv("MAMDR_STAR_ENGINE", raising=False)
    for hidden in ((128, 64), (256, 128, 64, 64), (64,)):          # pn + star at another depth: the generic-layer engine
        cfg = star_config(tmp_path, "star", hidden=hidden)
        star_factory.graph_calls = []
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
        assert star_factory.graph_calls[0][1]["expert_hidden"] == hidden
    cfg = star_config(tmp_path, "star", hidden=(256, 128, 64))
    monkeypatch.setenv("MAMDR_STAR_ENGINE", "graph")                # the twin of the step kernels
    star_factory.graph_calls = []
    m = cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
    assert len(star_factory.graph_calls) == 1 and m.model.kind == "star"
    from oracle import star as ostar
    assert tuple(m.model.segments) == sum(ostar.param_names(False), ())


def test_exceptions_are_unchanged_without_star_graph(tmp_path):
    for norm, dense in (("bn", "dense"), ("pn", "dense"), ("none", "star")):
        cfg = star_config(tmp_path, "star", norm, dense, hidden=(256, 128, 64))
        with pytest.raises(NotImplementedError, match="plain form"):
            cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), fake_factory)
    cfg = star_config(tmp_path, "star", aux=True, hidden=(256, 128, 64))
    with pytest.raises(NotImplementedError, match="auxiliary_net"):
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), fake_factory)
    cfg = star_config(tmp_path, "star", hidden=(128, 64))
    with pytest.raises(ValueError, match="three hidden layers"):
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), fake_factory)


def test_auxiliary_dim_mismatch_names_both_numbers(tmp_path):
    cfg = star_config(tmp_path, "star", aux=True, hidden=(256, 128))
    cfg["model"]["auxiliary_dim"] = 64
    with pytest.raises(ValueError, match=r"64.*128"):
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
    cfg["model"].update(norm="ln")
    cfg["model"]["auxiliary_dim"] = 128
    with pytest.raises(ValueError, match="norm"):
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)


def test_keras_names_and_the_reference_filters(tmp_path):
    from mamdr_amd.model_zoo import MAMDR
    cfg = star_config(tmp_path, "star_meta_mamdr", "bn", "star", True, (128, 64, 64, 64))
    m = cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
    assert type(m) is MAMDR
    eng = m.model
    names = {s: eng.keras_name(s) for s in eng.segments}
    assert names["Ws3"] == "kernel_shared_3" and names["bd3"] == "bias_specific_3" and names["wo"] == "dense/kernel"
    assert names["aux_W"] == "auxiliary_net/kernel_specific" and names["aux_b"] == "auxiliary_net/bias_specific"
    assert names["bn_gamma"] == "batch_normalization/gamma" and names["bn_beta"] == "batch_normalization/beta"
    # the reference's Star filter: the prefix up to the last shared bias, no holes
    m._get_model_meta_parms()
    assert m.model_meta_parms == ["domain_emb", "Ws0", "Ws1", "Ws2", "Ws3", "bs0", "bs1", "bs2", "bs3"]
    assert eng.meta_off == 0 and eng.meta_holes == () and eng.n_meta == eng.segments["bs3"][0] + eng.segments["bs3"][1]
    assert eng.segments["bn_gamma"][0] == eng.n_meta
    m.train_config["meta_parms"] = ["kernel_specific"]           # ... selects aux_W too, as it would in Keras
    m._get_model_meta_parms()
    assert m.model_meta_parms == ["Wd0", "Wd1", "Wd2", "Wd3", "aux_W"]
    m.train_config["meta_parms"] = ["all_hidden"]
    m._get_model_meta_parms()
    assert m.model_meta_parms == [s for s in eng.segments if s != "domain_emb"]
    # dense: dense -- the numbered Keras Dense layers; the Star filter finds no kernel_shared, as in the reference
    cfg = star_config(tmp_path, "star_meta_mamdr", "pn", "dense", True, (128, 64))
    m = cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
    names = [m.model.keras_name(s) for s in m.model.segments]
    assert names[:5] == ["domain_emb/embeddings", "dense/kernel", "dense_1/kernel", "dense/bias", "dense_1/bias"]
    assert "dense_2/kernel" in names and "dense_2/bias" in names and "gamma_specific" in names
    with pytest.raises(ValueError, match="kernel_shared"):
        m._get_model_meta_parms()


def test_bn_raises_under_several_participants(tmp_path, monkeypatch):
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    cfg = star_config(tmp_path, "star", "bn", "dense", hidden=(256, 128, 64))
    with pytest.raises(NotImplementedError, match="moving statistics"):
        cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory)
    cfg = star_config(tmp_path, "star", "pn", "dense", hidden=(256, 128, 64))      # pn keeps the step engine's aux layout
    assert cli.build_model(cfg, mds.MultiDomainDataset(cfg["dataset"]), star_factory).model.kind == "star"


def test_library_checks_the_star_config_before_any_device_call():
    from mamdr_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 19 and lib.mamdr_abi_version() == 19

    def create(emb_dim=128, hidden=(256, 128, 64), norm=1, dense=1, aux=0):
        four = lambda *v: (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))
        cfg = _lib.GraphConfig(_lib.ABI_VERSION, _lib.GRAPH_STAR, 10, 10, 2, emb_dim, 64, 0, len(hidden), four(*hidden), 0, four(),
                               0, four(), 0, 0, 0, 0.5, 1e-5, 0.9, 0.999, 1e-8, 1e-5, 0, norm, dense, aux)
        h = C.c_void_p()
        return lib.mamdr_graph_create(C.byref(cfg), None, C.byref(h)), lib.mamdr_graph_last_error()
    for kw, text in ((dict(emb_dim=64), b"128 only"), (dict(aux=128), b"auxiliary_dim 128"), (dict(norm=3), b"star_norm 3"),
                     (dict(dense=2), b"star_dense 2"), (dict(hidden=(256, 100)), b"multiples of 64"),
                     (dict(aux=-64), b"auxiliary_dim")):
        rc, msg = create(**kw)
        assert rc == _lib.EINVAL and text in msg, (kw, rc, msg)
    assert int(lib.mamdr_graph_aux_count(None)) == 0
    assert lib.mamdr_graph_bind_aux(None, None) == _lib.EINVAL


def test_switch_is_registered():
    from mamdr_amd import _lib
    rows = {r[0]: r for r in _lib.env_switches()}
    assert rows["MAMDR_STAR_ENGINE"][1] == "host"


@pytest.mark.parametrize("name", ["star_meta_mamdr", "star"])
def test_epochs_on_the_stand_in_carry_aux_through_best_state(tmp_path, name):
    cfg = star_config(tmp_path, name, "pn", "star", True, (64, 64), epochs=1)
    built = []
    avg_loss, avg_auc, dl, da = cli.main(cfg, star_factory, on_model=built.append)
    model = built[0]
    eng = model.model
    assert eng.kind == "star" and eng.auxiliary_dim == 64 and sorted(da) == [0, 1, 2] and np.isfinite(avg_loss)
    steps = eng.aux[4 * 3 * 384:4 * 3 * 384 + 3].numpy()
    assert (steps > 0).all()                                     # every domain's PartitionedNorm statistics moved
    # best-state save / restore carries aux: save, disturb, restore -- from the device copy and from the file
    base = model.base_model if hasattr(model, "base_model") else model
    base.save_model(base.checkpoint_path)
    saved = eng.aux.clone()
    assert base._best_in_memory[1] is not None and torch.equal(base._best_in_memory[1], saved)
    eng.aux.add_(1.0)
    base.load_model(base.checkpoint_path)
    assert torch.equal(eng.aux, saved)
    with np.load(base.checkpoint_path if base.checkpoint_path.endswith(".npz") else base.checkpoint_path + ".npz") as z:
        assert z["aux"].shape[0] == eng.aux.numel() and np.array_equal(z["aux"], saved.numpy())
        assert "aux_W" in list(z["segment_names"])


@pytest.mark.parametrize("hidden", [(256, 128, 64), (64,), (128, 64, 64, 64)])
@pytest.mark.parametrize("pretrained", [False, True])
def test_the_two_named_initialisers_are_members_of_the_family(hidden, pretrained):
    """`initial_tensors` (pn + star) and `dense_initial_tensors` (none + dense) draw what `forms_initial_tensors` draws for
    their form from the same stream: the same keys in the same order, dtypes and bits."""
    from mamdr_amd.model_zoo import star
    tables = {}
    if pretrained:
        rs = np.random.RandomState(5)
        tables = dict(user_emb=rs.standard_normal((30, 128)).astype(np.float32),
                      item_emb=rs.standard_normal((20, 128)).astype(np.float32))
    for make, norm, dense in ((star.initial_tensors, "pn", "star"), (star.dense_initial_tensors, "none", "dense")):
        if make is star.initial_tensors and len(hidden) != 3:
            continue                                            # (the step kernels' form has three layers)
        a = make(np.random.RandomState(11), 30, 20, 3, 128, hidden, **tables)
        b = star.forms_initial_tensors(np.random.RandomState(11), 30, 20, 3, 128, hidden, norm, dense, 0, **tables)
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
