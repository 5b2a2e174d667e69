"""The parts of the generic-layer engine's retrieval calls (mamdr_graph_recommend, _recommend_domain, _rank_domain,
_rank_slates) that need no device: the declarations, the null-handle refusal, the header's contract, which kinds
GraphEngine refuses by name, and that the model layer asks its engine to serve."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mamdr_amd import _lib, graph_engine      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("recommend", "recommend_domain", "rank_domain", "rank_slates")
REFUSED = ("shared_bottom", "mmoe", "ple", "star")
SERVED = ("ccpm", "nfm", "pnn", "autoint", "mlp", "wdl", "deepfm")


def test_the_four_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for call in CALLS:
        name = "mamdr_graph_" + call
        assert re.search(r"\bint %s\s*\(mamdr_graph\* g," % name, code), name
        step = _lib.SIGNATURES["mamdr_" + call]
        assert _lib.SIGNATURES[name] == step, name          # the step call's argument list, the handle in the context's place
        assert hasattr(lib, name), name


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    codes = (lib.mamdr_graph_recommend(None, 1, None, None, None, 0, None, None, 10, None, None, None),
             lib.mamdr_graph_recommend_domain(None, 0, 1, None, None, 0, None, None, 10, None, None, None),
             lib.mamdr_graph_rank_domain(None, 0, 1, None, None, 0, None, None, None, None, None, None, None),
             lib.mamdr_graph_rank_slates(None, 0, 1, None, None, None, None, None, None))
    assert codes == (_lib.EINVAL,) * 4
    assert b"null graph context" in lib.mamdr_graph_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(codes[0], graph=True)


def test_the_header_states_the_contract():
    header = open(os.path.join(ROOT, "include", "mamdr_hip.h")).read()
    comment = header[:header.index("int mamdr_graph_recommend(")]
    comment = comment[comment.rindex("/*"):]
    for phrase in ("NO REFERENCE COUNTERPART", "max_batch", "MAMDR_REC_CHUNK", "Reads the state only", "MAMDR_ENOTBUILT"):
        assert phrase in comment, phrase
    for kind in ("MAMDR_GRAPH_NFM", "_PNN", "_CCPM", "_AUTOINT", "_MLP", "_WDL", "_DEEPFM", "shared_bottom", "mmoe", "ple",
                 "MAMDR_GRAPH_STAR"):
        assert kind in comment, kind


OPT_IN = ("mlp", "wdl", "deepfm")       # also built on the step engine: an engine object of these kinds serves once asked to


def bare(kind):
    eng = graph_engine.GraphEngine.__new__(graph_engine.GraphEngine)      # (no device: `kind` alone decides)
    eng.kind = kind
    eng.ctx = None
    return eng


ARGS = {"recommend": ([0], [0], 5), "recommend_domain": ([0], 0, 5), "rank_domain": ([0], 0, [[1, 2]]),
        "rank_slates": ([0], 0, [[1, 2]])}


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("kind", REFUSED)
def test_multi_task_kinds_and_star_stay_refused_by_name(kind, call):
    eng = bare(kind)
    eng.enable_retrieval()              # (asking changes nothing for these kinds)
    with pytest.raises(NotImplementedError, match="generic-layer towers.*%s.*not built for retrieval" % kind):
        getattr(eng, call)(*ARGS[call])
    with pytest.raises(NotImplementedError, match="generic-layer towers.*%s.*not built for retrieval" % kind):
        getattr(bare(kind), call)(*ARGS[call])


class StandInLib(object):
    """records the family's retrieval calls and reports success: the launches of a host-only run."""

    def __init__(self):
        self.calls = []
        for call in CALLS:
            setattr(self, "mamdr_graph_" + call, lambda *a, _n=call: self.calls.append((_n, a)) or 0)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("kind", SERVED)
def test_single_output_kinds_reach_the_library(kind, call):
    """the served kinds do not take the refusal branch: the call marshals its arguments (on the CPU here) and arrives at
    its `mamdr_graph_*` entry point -- after the host's range checks, which still refuse a bad id before any launch."""
    eng = bare(kind)
    if kind in OPT_IN:
        with pytest.raises(NotImplementedError, match="generic-layer towers.*%s.*not built for retrieval" % kind):
            getattr(eng, call)(*ARGS[call])         # what such an object has always answered
        eng.enable_retrieval()
    eng.lib = StandInLib()
    eng.device = torch.device("cpu")
    eng.n_user, eng.n_item, eng.n_domain = 4, 9, 3
    res = getattr(eng, call)(*ARGS[call])
    assert [c[0] for c in eng.lib.calls] == [call]
    assert isinstance(res, (tuple, dict))
    del eng.lib.calls[:]
    bad = {"recommend": ([4], [0], 5), "recommend_domain": ([0], 3, 5), "rank_domain": ([0], 0, [[9]]),
           "rank_slates": ([0], 0, [[1, 1]])}[call]
    with pytest.raises(ValueError):
        getattr(eng, call)(*bad)
    assert not eng.lib.calls


def test_item_rows_of_the_generic_layer_engine():
    """the bound frozen table, or the item_emb segment of the live vector at a 16-byte offset."""
    eng = bare("ccpm")
    eng.emb_trainable, eng.n_item, eng.emb_dim = False, 3, 4
    eng.tables = {"item_emb": torch.arange(12.0).view(3, 4)}
    assert eng.item_rows() is eng.tables["item_emb"]
    eng.emb_trainable = True
    eng._weights = torch.arange(40.0)
    eng.segments = {"user_emb": (0, 8), "item_emb": (8, 12)}
    assert np.array_equal(eng.item_rows().numpy(), np.arange(8.0, 20.0).reshape(3, 4))
    eng.segments = {"item_emb": (6, 12)}
    with pytest.raises(RuntimeError, match="16-byte offset"):
        eng.item_rows()


def test_the_model_layer_asks_its_engine_to_serve():
    """BaseModel.construct_engine calls enable_retrieval() on an engine that has one, and leaves other factories alone."""
    from mamdr_amd.model_zoo import base_model

    class Route(object):
        engine, offer, args, kwargs = "graph", None, ("mlp",), {}

    made = []

    def factory(kind, *a, **kw):
        made.append(bare(kind))
        return made[-1]
    m = base_model.BaseModel.__new__(base_model.BaseModel)
    m.train_config = {"emb_trainable": False, "load_pretrain_emb": True}
    m.engine_factory, m.n_uid, m.n_pid, m.n_domain, m.batch_size = factory, 4, 9, 3, 256
    eng = m.construct_engine(Route())
    assert eng is made[0] and eng._retrieval is True
    m.engine_factory = lambda *a, **kw: object()
    assert not hasattr(m.construct_engine(Route()), "_retrieval")
