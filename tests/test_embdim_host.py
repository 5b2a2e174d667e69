"""Host side of the embedding widths other than 128 (mlp / wdl / deepfm on the generic-layer engine): the registry's
routing, the checks that name the accepted set, the dataset layer's `synthetic_emb_dim`, the shipped config and the
library's own check -- all without a device."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from mamdr_amd import cli
from mamdr_amd.utils import MultiDomainDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = {"name": "Taobao", "split": "s", "n_domain": 3, "n_user": 300, "n_item": 200, "n_train": 900, "n_val": 300,
        "n_test": 300, "pretrained": True}


class Built(Exception):
    """raised by the recording engine classes: the engine was chosen and constructed, nothing else is of interest"""


def config(tmp_path, name="mlp_meta_mamdr_finetune", dim=64, hidden=(256, 128, 64), table_dim=None, **model):
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        cfg = copy.deepcopy(json.load(f))
    cfg["model"].update(name=name, hidden_dim=list(hidden), user_dim=dim, item_dim=dim, domain_dim=dim, **model)
    cfg["train"].update(epoch=1, patience=1, sample_num=2, result_save_path=str(tmp_path / "result"),
                        checkpoint_path=str(tmp_path / "checkpoint"))
    cfg["dataset"].update(batch_size=64, synthetic=dict(TINY))
    if table_dim is None:
        table_dim = dim
    if table_dim != 128:
        cfg["dataset"]["synthetic_emb_dim"] = table_dim
    return cfg


@pytest.fixture
def recorders(monkeypatch):
    """the two engine classes replaced by recorders (this box has no device): calls[...] = (class name, args, kwargs)"""
    from mamdr_amd import engine, graph_engine
    calls = []

    def recorder(label):
        class Recorder(object):
            def __init__(self, *a, **k):
                calls.append((label, a, k))
                raise Built(label)
        return Recorder
    monkeypatch.setattr(graph_engine, "GraphEngine", recorder("GraphEngine"))
    monkeypatch.setattr(engine, "TowerEngine", recorder("TowerEngine"))
    return calls


@pytest.mark.parametrize("name", ["mlp_meta_mamdr_finetune", "wdl", "deepfm_meta_domain_negotiation"])
@pytest.mark.parametrize("dim", [32, 64, 256])
def test_other_width_routes_to_the_generic_engine(tmp_path, recorders, name, dim):
    cfg = config(tmp_path, name, dim)                   # hidden_dim [256, 128, 64]: the width alone decides
    with pytest.raises(Built, match="GraphEngine"):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    (label, args, kw), = recorders
    assert label == "GraphEngine" and args[0] == name.split("_")[0] and kw["emb_dim"] == dim
    assert kw["expert_hidden"] == (256, 128, 64) and kw["tower_hidden"] == ()


def test_width_128_with_the_reference_shape_stays_on_the_step_engine(tmp_path, recorders):
    cfg = config(tmp_path, "mlp_meta_mamdr_finetune", 128)
    with pytest.raises(Built, match="TowerEngine"):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    (label, args, kw), = recorders
    assert label == "TowerEngine" and kw["emb_dim"] == 128 and kw["hidden"] == (256, 128, 64)


REF = (256, 128, 64)
PN_STAR = dict(norm="pn", dense="star", auxiliary_net=False)
# (model name, user_dim, hidden_dim, batch size, environment, Star keys) ->
#     (engine class, first positional argument or tower=, the keyword arguments that matter) | (exception type, message fragment)
ROUTES = [
    # pnn / nfm: the step kernels at the reference shape up to 2,048 rows, the generic-layer engine beyond either limit
    ("pnn", 128, REF, 64, {}, {}, ("TowerEngine", "pnn", dict(hidden=REF, emb_dim=128))),
    ("nfm", 128, REF, 64, {}, {}, ("TowerEngine", "nfm", dict(hidden=REF, emb_dim=128))),
    ("pnn", 128, REF, 2048, {}, {}, ("TowerEngine", "pnn", {})),
    ("nfm_meta_mamdr", 128, REF, 2048, {}, {}, ("TowerEngine", "nfm", {})),
    ("pnn", 128, REF, 4096, {}, {}, ("GraphEngine", "pnn", dict(expert_hidden=REF, tower_hidden=(), emb_dim=128))),
    ("nfm", 128, REF, 4096, {}, {}, ("GraphEngine", "nfm", dict(expert_hidden=REF, tower_hidden=(), emb_dim=128))),
    ("pnn", 128, (128, 64), 64, {}, {}, ("GraphEngine", "pnn", dict(expert_hidden=(128, 64)))),
    ("nfm", 128, (128, 64), 64, {}, {}, ("GraphEngine", "nfm", dict(expert_hidden=(128, 64)))),
    # ... and under their own switch; neither tower reads the other's
    ("pnn", 128, REF, 64, {"MAMDR_PNN_ENGINE": "graph"}, {}, ("GraphEngine", "pnn", dict(expert_hidden=REF))),
    ("nfm", 128, REF, 64, {"MAMDR_NFM_ENGINE": "graph"}, {}, ("GraphEngine", "nfm", dict(expert_hidden=REF))),
    ("pnn", 128, REF, 64, {"MAMDR_NFM_ENGINE": "graph"}, {}, ("TowerEngine", "pnn", {})),
    ("nfm", 128, REF, 64, {"MAMDR_PNN_ENGINE": "graph"}, {}, ("TowerEngine", "nfm", {})),
    ("pnn", 128, REF, 64, {"MAMDR_PNN_ENGINE": "step"}, {}, ("TowerEngine", "pnn", {})),
    # ccpm / autoint: the generic-layer engine only
    ("ccpm", 128, REF, 64, {}, {}, ("GraphEngine", "ccpm", dict(expert_hidden=REF, tower_hidden=()))),
    ("autoint", 128, REF, 4096, {"MAMDR_PNN_ENGINE": "graph"}, {}, ("GraphEngine", "autoint", dict(expert_hidden=REF))),
    # mlp / wdl / deepfm: the step kernels at the reference shape and width 128 only
    ("deepfm", 128, REF, 4096, {"MAMDR_PNN_ENGINE": "graph"}, {}, ("TowerEngine", "deepfm", dict(hidden=REF, emb_dim=128))),
    ("mlp_uncertainty_weight", 128, REF, 64, {}, {}, ("TowerEngine", "mlp", dict(uncertainty_weight=True))),
    ("mlp", 128, (128, 64), 64, {}, {}, ("GraphEngine", "mlp", dict(expert_hidden=(128, 64), tower_hidden=(), emb_dim=128))),
    ("wdl", 64, (128, 64, 64, 64), 64, {}, {}, ("GraphEngine", "wdl", dict(expert_hidden=(128, 64, 64, 64), emb_dim=64))),
    ("mlp", 128, (100, 64), 64, {}, {}, (ValueError, "multiples of 64")),
    ("mlp", 128, (256, 128, 64, 64, 64), 64, {}, {}, (ValueError, "1 to 4 hidden layers")),
    # Star: the step form and its twin, one bn form, the plain-DNN form on the mlp tower without regularisers
    ("star", 128, REF, 64, {}, PN_STAR, ("TowerEngine", "star", dict(hidden=REF, dropout=0.0, emb_dim=128))),
    ("star", 128, REF, 64, {"MAMDR_STAR_ENGINE": "graph"}, PN_STAR,
     ("GraphEngine", "star", dict(norm="pn", dense="star", auxiliary_dim=0, expert_hidden=REF, tower_hidden=(), dropout=0.0))),
    ("star", 128, REF, 64, {"MAMDR_PNN_ENGINE": "graph"}, PN_STAR, ("TowerEngine", "star", {})),
    ("star", 128, (128, 64), 64, {}, PN_STAR, ("GraphEngine", "star", dict(norm="pn", dense="star", expert_hidden=(128, 64)))),
    ("star_meta_mamdr", 128, REF, 64, {}, dict(norm="bn", dense="dense", auxiliary_net=True, auxiliary_dim=64),
     ("GraphEngine", "star", dict(norm="bn", dense="dense", auxiliary_dim=64, expert_hidden=REF, dropout=0.0))),
    ("star", 128, (100, 64), 64, {}, dict(norm="bn", dense="star", auxiliary_net=False), (ValueError, "multiples of 64")),
    ("star", 128, REF, 64, {"MAMDR_STAR_ENGINE": "graph"}, dict(norm="none", dense="dense", auxiliary_net=False),
     ("TowerEngine", "mlp", dict(l2_emb=0.0, l2_linear=0.0, dropout=0.0, hidden=REF))),
    ("star", 128, (128, 64), 64, {}, dict(norm="none", dense="dense", auxiliary_net=False),
     ("GraphEngine", "mlp", dict(l2_emb=0.0, l2_linear=0.0, dropout=0.0, expert_hidden=(128, 64)))),
    ("star", 128, REF, 64, {}, dict(norm="pn", dense="star", auxiliary_net=True, auxiliary_dim=128), (ValueError, "auxiliary_dim 128")),
    # the multi-task towers: always the generic-layer engine
    ("mmoe", 128, (128, 64), 64, {"MAMDR_PNN_ENGINE": "graph"}, dict(tower_hidden_dim=[64], gate_dnn_hidden_units=[64], num_experts=2),
     ("GraphEngine", "mmoe", dict(expert_hidden=(128, 64), tower_hidden=(64,), gate_hidden=(64,), num_experts=2, emb_dim=128))),
]


@pytest.mark.parametrize("name,dim,hidden,batch,env,star,want", ROUTES)
def test_routing_table(tmp_path, monkeypatch, recorders, name, dim, hidden, batch, env, star, want):
    """which engine a config builds, and with which arguments: one literal table over the towers, shapes, batch sizes and
    the three host switches"""
    for k in ("MAMDR_PNN_ENGINE", "MAMDR_NFM_ENGINE", "MAMDR_STAR_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = config(tmp_path, name, dim, hidden, **star)
    cfg["dataset"]["batch_size"] = batch
    if isinstance(want[0], type):
        with pytest.raises(want[0], match=want[1]):
            cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
        assert recorders == []
        return
    with pytest.raises(Built, match=want[0]):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    (label, args, kw), = recorders
    assert label == want[0]
    assert (args[0] if label == "GraphEngine" else kw["tower"]) == want[1]
    assert args[-4:] == (300, 200, 3, batch)                    # n_user, n_item, n_domain, batch_size
    assert {k: kw[k] for k in want[2]} == want[2]
    assert ("hidden" in kw) == (label == "TowerEngine") and ("expert_hidden" in kw) == (label == "GraphEngine")


def test_width_outside_the_accepted_set_and_unequal_dims_are_value_errors(tmp_path, recorders):
    from mamdr_amd.model_zoo.deepctr import EMB_WIDTHS
    assert EMB_WIDTHS == (32, 64, 128, 256)
    for dim in (8, 48, 96, 512):
        cfg = config(tmp_path, "deepfm", dim)
        with pytest.raises(ValueError, match=r"\(32, 64, 128, 256\)"):
            cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    cfg = config(tmp_path, "mlp", 64)
    cfg["model"]["item_dim"] = 32
    with pytest.raises(ValueError, match="must be equal"):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    assert recorders == []                              # no engine was constructed


@pytest.mark.parametrize("name,extra", [("star", dict(norm="pn", dense="star")), ("pnn", {}), ("nfm", {}), ("ccpm", {}),
                                        ("autoint", {}), ("mmoe", dict(tower_hidden_dim=[64], gate_dnn_hidden_units=[64],
                                                                       num_experts=2))])
def test_other_towers_name_their_width_limit(tmp_path, recorders, name, extra):
    cfg = config(tmp_path, name, 64, **extra)
    with pytest.raises(NotImplementedError, match="128"):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    assert recorders == []


def test_dataset_layer_generates_tables_of_the_asked_width(tmp_path):
    cfg = config(tmp_path, dim=64)
    ds = MultiDomainDataset(cfg["dataset"])
    assert ds.user_emb.shape == (ds.n_uid, 64) and ds.item_emb.shape == (ds.n_pid, 64)
    assert ds.user_emb.dtype == np.float32
    del cfg["dataset"]["synthetic_emb_dim"]
    ds = MultiDomainDataset(cfg["dataset"])
    assert ds.user_emb.shape == (ds.n_uid, 128) and ds.item_emb.shape == (ds.n_pid, 128)


def test_pretrained_tables_of_another_width_are_a_value_error(tmp_path, recorders):
    cfg = config(tmp_path, "mlp", dim=64, table_dim=128)
    with pytest.raises(ValueError, match="128 wide.*64"):
        cli.build_model(cfg, MultiDomainDataset(cfg["dataset"]))
    assert recorders == []


def test_shipped_config_at_width_64_loads():
    with open(os.path.join(ROOT, "config", "Taobao-10", "emb64", "deepctr_DN+DR.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(ROOT, "config", "Taobao-10", "deepctr_DN+DR.json")) as f:
        base = json.load(f)
    assert [cfg["model"][k] for k in ("user_dim", "item_dim", "domain_dim")] == [64, 64, 64]
    assert cfg["dataset"]["synthetic"] == "taobao10" and cfg["dataset"]["synthetic_emb_dim"] == 64
    for k in ("user_dim", "item_dim", "domain_dim"):
        cfg["model"][k] = 128
    del cfg["dataset"]["synthetic_emb_dim"]
    assert cfg == base                                  # the MAMDR config, nothing else changed


def test_library_rejects_an_unaccepted_width_before_any_device_call():
    from mamdr_amd import _lib
    lib = _lib.load()

    def create(kind, emb_dim):
        four = lambda *v: (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))
        cfg = _lib.GraphConfig(_lib.ABI_VERSION, kind, 10, 10, 2, emb_dim, 64, 0, 2, four(128, 64), 1, four(64), 1, four(64),
                               2, 0, 0, 0.5, 1e-5, 0.9, 0.999, 1e-8, 1e-5, 0)
        h = C.c_void_p()
        return lib.mamdr_graph_create(C.byref(cfg), None, C.byref(h)), lib.mamdr_graph_last_error()
    for kind, emb_dim in ((_lib.GRAPH_MLP, 48), (_lib.GRAPH_DEEPFM, 16), (_lib.GRAPH_WDL, 512), (_lib.GRAPH_NFM, 64),
                          (_lib.GRAPH_MMOE, 64), (_lib.GRAPH_PNN, 256)):
        rc, msg = create(kind, emb_dim)
        assert rc == _lib.EINVAL, (kind, emb_dim, rc)
        assert b"32, 64, 128 or 256" in msg and b"128 only" in msg and str(emb_dim).encode() in msg, msg
