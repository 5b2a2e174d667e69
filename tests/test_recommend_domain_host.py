"""Single-domain top-K retrieval, host side (no GPU): `mamdr_recommend_domain`'s declaration, its place in the header and
its binding, the refusal that needs no device, and `BaseModel.recommend`'s choice between an engine's `recommend_domain`
and its `recommend` over CPU stand-ins of the engine (tests/test_recommend_host.py's)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mamdr_amd import _lib, cli
from test_recommend_host import RecommendingEngine, patch_emb_dim, tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    with open(os.path.join(ROOT, "include", "mamdr_hip.h")) as f:
        return f.read()


# ------------------------------------------------------------------ C ABI
def test_recommend_domain_is_declared_behind_recommend_and_bound():
    header = header_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+mamdr_recommend_domain\s*\(([^;]*)\)\s*;", code)
    assert m, "mamdr_recommend_domain is not declared in include/mamdr_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["mamdr_ctx* ctx", "int32_t domain", "int32_t n_query", "const int32_t* d_uid", "const int32_t* d_cand",
                      "int64_t n_cand", "const int64_t* d_excl_off", "const int32_t* d_excl_ids", "int32_t k",
                      "int32_t* d_ids_out", "float* d_scores_out", "float* d_scores_all"], params
    # behind mamdr_recommend's declaration, and not named before it (tests/test_recommend_host.py finds that call's
    # comment through the first "int mamdr_recommend")
    first = header.index("int mamdr_recommend")
    assert re.match(r"int mamdr_recommend\s*\(", header[first:])
    assert header.index("mamdr_recommend_domain") > first
    assert code.index("mamdr_recommend_domain") > re.search(r"\bint\s+mamdr_recommend\s*\(", code).start()
    doc = header[:header.index("int mamdr_recommend_domain")].rsplit("/*", 1)[1]
    assert "NO REFERENCE COUNTERPART" in doc
    assert "star" in doc and "MAMDR_ENOTBUILT" in doc and "domain outside [0, n_domain)" in doc
    # mamdr_recommend's own comment no longer claims that Star does not separate
    rec_doc = header[:first].rsplit("/*", 1)[1]
    assert "one domain at a time" in rec_doc
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES["mamdr_recommend_domain"] == (C.c_int, [vp, i32, i32, vp, vp, i64, vp, vp, i32, vp, vp, vp])
    assert _lib.ABI_VERSION == 19
    assert re.search(r"#define\s+MAMDR_ABI_VERSION\s+19\b", header)


def test_null_context_is_refused_without_a_device():
    lib = _lib.load()
    code = lib.mamdr_recommend_domain(None, 0, 1, None, None, 0, None, None, 10, None, None, None)
    assert code == _lib.EINVAL
    assert b"null context" in lib.mamdr_last_error()
    with pytest.raises(_lib.MamdrError):
        _lib.check(code)


def test_generic_layer_engine_refuses_by_name():
    from mamdr_amd import graph_engine
    eng = graph_engine.GraphEngine.__new__(graph_engine.GraphEngine)      # (no device: the refusal needs none)
    eng.kind = "star"
    with pytest.raises(NotImplementedError, match="generic-layer towers.*star.*not built for retrieval"):
        eng.recommend_domain([0], 0, 5)
    eng.ctx = None


# ------------------------------------------------------------------ BaseModel.recommend over CPU stand-ins
class DomainEngine(RecommendingEngine):
    """the stand-in with a `recommend_domain` as well: it records its calls and answers through the parent's numpy forward,
    whose own counter then tells whether `recommend` was reached from outside."""
    domain_calls = []
    outside_recommend = 0

    def recommend(self, *args, **kwargs):
        if not getattr(self, "_inside", False):
            type(self).outside_recommend += 1
        return RecommendingEngine.recommend(self, *args, **kwargs)

    def recommend_domain(self, uids, domain, k, candidates=None, exclude=None, want_scores=False):
        type(self).domain_calls.append(domain)
        self._inside = True
        try:
            return self.recommend(uids, np.full(np.asarray(uids).shape, domain, np.int32), k, candidates=candidates,
                                  exclude=exclude, want_scores=want_scores)
        finally:
            self._inside = False


@pytest.mark.parametrize("name", ["mlp", "mlp_meta_mamdr_finetune", "mlp_uncertainty_weight"])
def test_base_model_prefers_the_single_domain_call(tmp_path, monkeypatch, name):
    """plain model, a meta wrapper and UncertaintyWeight (their __getattr__ forwards `recommend` to the BaseModel): one
    recommend_domain call per domain with a scalar domain, `recommend` never called, and the lists are the ones the
    stand-in without recommend_domain returns."""
    patch_emb_dim(monkeypatch)
    DomainEngine.domain_calls, DomainEngine.outside_recommend = [], 0
    built = []
    out = str(tmp_path / "single.npz")
    cli.main(tiny_config(tmp_path / "single", name), DomainEngine, on_model=built.append, recommend=5, recommend_out=out)
    assert DomainEngine.outside_recommend == 0
    assert DomainEngine.domain_calls == [0, 1, 2]
    assert all(isinstance(d, int) and not isinstance(d, bool) for d in DomainEngine.domain_calls)
    model = built[0]
    DomainEngine.domain_calls = []
    r = model.recommend(1, 3, users=[4, 2], exclude_seen=False)
    assert DomainEngine.domain_calls == [1] and DomainEngine.outside_recommend == 0
    assert r["users"].tolist() == [4, 2] and r["ids"].shape == r["scores"].shape == (2, 3)
    # the existing stand-in has no recommend_domain: `recommend` with the filled domain vector, as before, same lists
    assert not hasattr(RecommendingEngine, "recommend_domain")
    RecommendingEngine.calls_recommend = 0
    old = str(tmp_path / "vector.npz")
    cli.main(tiny_config(tmp_path / "vector", name), RecommendingEngine, recommend=5, recommend_out=old)
    assert RecommendingEngine.calls_recommend == 3
    with np.load(out) as a, np.load(old) as b:
        assert sorted(a.files) == sorted(b.files)
        for f in a.files:
            assert a[f].tobytes() == b[f].tobytes(), f
