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
