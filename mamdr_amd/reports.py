"""The reports that run behind an evaluation (none has a reference counterpart): one table, EVAL_REPORTS, from the
train-config key to result.json, in the order of the tail of `DeviceEngine.evaluate`'s tuple.  The definitions and their
`summarise` functions stay in gauc.py, exact.py and bootstrap.py.  Below, `req` is what an entry's `request` returned, `cols`
the columns of a bound split and `reps` = {domain: report} of one mode."""
import collections
import os.path as osp

import numpy as np

from . import bootstrap, exact, gauc

Report = collections.namedtuple("Report", [
    "name", "keyword", "config_key", "flag",    # its name, keyword of `evaluate`, train-config key and the run.py flag of that key
    "refusal",          # the middle of cli.main's multi-process / multi-lane NotImplementedError
    "request",          # (train_config) -> the keyword's value, validated; None when the key is not set
    "launch",           # (engine, preds, cols, req) -> device tensors of the chain on the engine's stream, nothing read back
    "finish",           # (those tensors) -> the report dict, read back
    "host",             # (preds, cols, req) -> the same report from the host definition (the tests' stand-in engine)
    "print_summary",    # (mode, reps, req, print_metric): the lines BaseModel._summarise prints
    "save"])            # (result, result_path, reps, req): the result.json keys and the .npz sidecar of BaseModel.save_result


def _print_means(mode, reps, print_metric, overall, names):
    """per (printed name, report key) of `names`: the per-domain block, then the line of overall[key] = (mean, weighted mean)."""
    for name, key in names:
        print_metric(name, {d: r[key] for d, r in reps.items()})
        print("Overall {} {}: {}, Weighted {}: {}".format(mode, name, overall[key][0], name, overall[key][1]))


def _gauc_save(result, result_path, reps, req):
    result["avg_gauc"], result["weighted_gauc"] = gauc.summarise(reps)
    result["domain_gauc"] = {d: r["gauc"] for d, r in reps.items()}
    result["domain_gauc_users"] = {d: r["n_valid"] for d, r in reps.items()}


def _exact_save(result, result_path, reps, req):
    result["avg_auc_exact"], result["weighted_auc_exact"] = exact.summarise(reps)["auc"]
    result["domain_auc_exact"] = {d: r["auc"] for d, r in reps.items()}
    for key in ("ap", "ece", "pcoc"):
        result["domain_" + key] = {d: r[key] for d, r in reps.items()}
    # the calibration bins behind ece / pcoc: [domains][n_bins], the rows of `domains` in its order
    np.savez(osp.join(result_path, "exact_metrics.npz"), domains=np.array(list(reps), np.int64),
             **{k: np.array([r[k] for r in reps.values()]).reshape(len(reps), -1)
                for k in ("bin_rows", "bin_positives", "bin_pred_sum")})


def _ci_request(tc):
    """train.report_auc_ci / auc_ci_seed / auc_ci_unit -> the engines' want_ci = (n_rep, seed, "row" | "user")."""
    if not tc.get("report_auc_ci"):
        return None
    n_rep, unit = int(tc["report_auc_ci"]), tc.get("auc_ci_unit", "user")
    if not 1 <= n_rep <= 65535:
        raise ValueError("train.report_auc_ci %d outside 1..65535" % n_rep)
    if unit not in ("row", "user"):
        raise ValueError("train.auc_ci_unit is 'row' or 'user', got %r" % (unit,))
    return n_rep, int(tc.get("auc_ci_seed", 0)), unit


def _ci_args(preds, cols, req):
    """mamdr_auc_bootstrap's / replicates_host's arguments: "user" resamples the split's uid column, "row" its rows."""
    n_rep, seed, unit = req
    return preds, cols["label"], n_rep, seed, cols["uid"] if unit == "user" else None


def _ci_print(mode, reps, req, print_metric):
    print("Exact AUC, {} bootstrap replicates by {} (seed {}): estimate [95 % interval] standard error, valid".format(
        req[0], req[2], req[1]))
    for d, r in reps.items():
        print("{}: {} [{}, {}] {}, {}".format(d, r["auc"], r["ci_lo"], r["ci_hi"], r["se"], r["n_valid"]))


def _ci_save(result, result_path, reps, req):
    result.update(bootstrap.summarise(reps))
    # what bootstrap.paired needs to compare two runs: per domain d the replicates and their integers
    n_rep, seed, unit = req
    arrays = {"n_rep": np.int64(n_rep), "seed": np.uint64(seed & 0xFFFFFFFFFFFFFFFF), "unit": np.array(unit)}
    for d, r in reps.items():
        for k in ("replicates", "T", "P", "N"):
            arrays["%s_%s" % (k, d)] = r[k]
    np.savez(osp.join(result_path, "auc_bootstrap.npz"), **arrays)


EVAL_REPORTS = (
    Report("gauc", "want_gauc", "report_gauc", "--gauc", "the per-user grouped AUC is",
           request=lambda tc: True if tc.get("report_gauc") else None,
           launch=lambda eng, preds, cols, req: (eng._group_auc_launch(preds, cols["label"], eng._group_plan_of(cols)),),
           finish=lambda tensors: gauc.finish(*tensors[0].cpu().numpy().tolist()),
           host=lambda preds, cols, req: gauc.group_auc_host(preds, cols["label"], cols["uid"]), save=_gauc_save,
           print_summary=lambda mode, reps, req, pm: _print_means(mode, reps, pm, {"gauc": gauc.summarise(reps)}, [("GAUC", "gauc")])),
    Report("exact", "want_exact", "report_exact", "--exact-metrics", "the exact AUC, average precision and calibration are",
           request=lambda tc: int(tc["report_exact"]) if tc.get("report_exact") else None,
           launch=lambda eng, preds, cols, req: eng._exact_launch(preds, cols["label"], req)[:3],
           finish=lambda tensors: exact.finish(*[t.cpu().numpy() for t in tensors]),
           host=lambda preds, cols, req: exact.report_host(preds, cols["label"], req), save=_exact_save,
           print_summary=lambda mode, reps, req, pm: _print_means(mode, reps, pm, exact.summarise(reps),
                                                                  [("Exact AUC", "auc"), ("AP", "ap"), ("ECE", "ece")])),
    Report("ci", "want_ci", "report_auc_ci", "--auc-ci", "the bootstrap replicates of the exact AUC are",
           request=_ci_request, launch=lambda eng, preds, cols, req: eng._bootstrap_launch(*_ci_args(preds, cols, req)),
           finish=lambda tensors: bootstrap.finish(*[t.cpu().numpy() for t in tensors]),
           host=lambda preds, cols, req: bootstrap.finish(*bootstrap.replicates_host(*_ci_args(preds, cols, req))),
           print_summary=_ci_print, save=_ci_save),
)


def requested(train_config):
    """[(entry, request)] of the entries whose train-config key is set, in table order."""
    return [(e, req) for e, req in ((e, e.request(train_config)) for e in EVAL_REPORTS) if req is not None]
