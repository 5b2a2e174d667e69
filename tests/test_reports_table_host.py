"""reports.EVAL_REPORTS, host side (no GPU): the table's keywords, config keys and order are what `DeviceEngine.evaluate`'s
signature and the tests' stand-in use, and `cli.main` refuses every entry's config key under lanes by name."""
import inspect

import numpy as np
import pytest

from fake_engine import ReportingFakeEngine
from mamdr_amd import cli, engine, utils
from mamdr_amd.reports import EVAL_REPORTS, requested
from test_gauc_host import patch_emb_dim, tiny_config


def test_the_table_is_what_evaluate_and_the_stand_in_use(tmp_path):
    assert [(e.name, e.keyword, e.config_key, e.flag) for e in EVAL_REPORTS] == [
        ("gauc", "want_gauc", "report_gauc", "--gauc"), ("exact", "want_exact", "report_exact", "--exact-metrics"),
        ("ci", "want_ci", "report_auc_ci", "--auc-ci")]
    # evaluate's keywords behind want_preds are the table's, in its order, and their defaults ask for nothing
    params = list(inspect.signature(engine.DeviceEngine.evaluate).parameters.values())
    assert [p.name for p in params] == ["self", "domain", "split", "want_preds"] + [e.keyword for e in EVAL_REPORTS]
    assert [p.default for p in params[4:]] == [False, 0, None]
    # the requests of the tiny config with every key set, then the stand-in on a 24-row split: the tail in table order
    train = tiny_config(tmp_path, "mlp", report_gauc=True, report_exact=5, report_auc_ci=12, auc_ci_seed=3)["train"]
    wanted = requested(train)
    assert [(e.name, req) for e, req in wanted] == [("gauc", True), ("exact", 5), ("ci", (12, 3, "user"))]
    rs = np.random.RandomState(1)
    eng = ReportingFakeEngine(40, 30, 3, 16, dropout=0.0, emb_dim=8, hidden=(16, 8, 4))
    eng.bind_domain_data(1, "test", rs.randint(0, 6, 24), rs.randint(0, 30, 24), np.ones(24, np.int32),
                         (np.arange(24) % 3 == 0).astype(np.float32))
    ReportingFakeEngine.seen, ReportingFakeEngine.log = [], []
    out = eng.evaluate(1, "test", **{e.keyword: req for e, req in wanted})
    assert len(out) == 5 and out[:2] == eng.evaluate(1, "test")
    assert "gauc" in out[2] and out[3]["bin_rows"].shape == (5,) and out[4]["replicates"].shape == (13,)
    assert [(name, rep is tail) for (_, _, name, _, rep), tail in zip(ReportingFakeEngine.log, out[2:])] == [
        ("gauc", True), ("exact", True), ("ci", True)]
    assert ReportingFakeEngine.seen == [{"want_gauc": True, "want_exact": 5, "want_ci": (12, 3, "user")}, {}]


@pytest.mark.parametrize("entry", EVAL_REPORTS, ids=lambda e: e.name)
def test_lanes_refuse_every_entry_by_its_key(tmp_path, monkeypatch, entry):
    patch_emb_dim(monkeypatch)
    loaded = []
    monkeypatch.setattr(utils, "MultiDomainDataset", lambda *a, **k: loaded.append(a))
    cfg = tiny_config(tmp_path, "mlp_meta_mamdr", lanes=2, **{entry.config_key: 20})
    with pytest.raises(NotImplementedError, match=r"train\.%s \(run\.py %s\): %s not gathered across processes or lanes .* "
                                                  r"train\.lanes = 1$" % (entry.config_key, entry.flag, entry.refusal)):
        cli.main(cfg, ReportingFakeEngine)
    assert not loaded                    # refused before the data is loaded
