"""What the per-user grouped AUC costs on top of an evaluation, on the device (mamdr_group_auc) and on the host
(device-to-host copy of every prediction + gauc.group_auc_host), per input:

    taobao10      Taobao-10's full test split: all 10 domains, 43,502 rows, one evaluate call per domain
    amazon6       Amazon-6's largest test domain
    amazon6-hot   the same with hot=dict(users=64, items=64, share=0.3): 64 users hold 30 % of the rows, groups of
                  thousands of rows

    python tools/gauc_bench.py [--inputs taobao10,amazon6,amazon6-hot] [--reps 5] [--out profiles/gauc_bench.txt]

Legs, each in a child process of its own under `timeout -k 10`:
    a  evaluate(d, "test")                      the evaluation alone: the baseline
    b  evaluate(d, "test", want_gauc=True)      + mamdr_group_auc on the engine's stream
    c  evaluate(d, "test", want_preds=True)     + the copy of the predictions + gauc.group_auc_host
Method: synthetic data of the named shape (seed 7, test split only), the mlp tower over frozen random tables, random
weights; two warm-up calls (they also build and upload leg b's plan: built once per bound split), then `reps` calls between
two HIP events recorded on the engine's stream.  Every call ends in its own read-back, so the figure is wall time per call
as a caller sees it, host work included.  Leg b also times the launches of mamdr_group_auc alone (no read-back between
them) for the bytes-over-time figure: 12 n + 8 G bytes against the 8 TB/s HBM peak of the MI355X.  Every leg hashes its
predictions; legs b and c hash T_u of every group: the parent refuses to report unless all agree.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s


def problem(name):
    """-> (engine, [domains to evaluate], {domain: columns})"""
    import torch  # noqa: F401
    from mamdr_amd import synthetic
    from mamdr_amd.engine import TowerEngine
    shape = "taobao10" if name == "taobao10" else "amazon6"
    hot = dict(users=64, items=64, share=0.3) if name.endswith("-hot") else None
    g = synthetic.generate(shape, batch_size=1024, seed=7, splits=("test",), hot=hot)
    test = g["data"]["test"]
    domains = sorted(test) if name == "taobao10" else [max(test, key=lambda d: test[d]["uid"].shape[0])]
    eng = TowerEngine(g["n_user"], g["n_item"], g["n_domain"], 1024, dropout=0.0, emb_trainable=False, tower="mlp")
    eng.bind_table("user_emb", g["tables"]["user_emb"])
    eng.bind_table("item_emb", g["tables"]["item_emb"])
    rs = np.random.RandomState(7)
    scale = {"domain_emb": 0.05, "W0": 0.06, "W1": 0.07, "W2": 0.1, "wo": 0.17, "gb": 0.0}
    eng.set_weights(eng.pack({n: (rs.standard_normal(cnt) * scale.get(n, 0.05)).astype(np.float32)
                              for n, (off, cnt) in eng.segments.items()}))
    for d in domains:
        c = test[d]
        eng.bind_domain_data(d, "test", c["uid"], c["pid"], c["domain"], c["label"])
    return eng, domains, test


def timed(eng, call, reps):
    import torch
    for _ in range(2):
        call()
    torch.cuda.synchronize(eng.device)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(eng.stream)
    for _ in range(reps):
        call()
    b.record(eng.stream)
    torch.cuda.synchronize(eng.device)
    return a.elapsed_time(b) / reps


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def leg(args):
    import torch
    from mamdr_amd import gauc
    eng, domains, test = problem(args.input)
    res = {"leg": args.leg, "input": args.input, "domains": len(domains), "reps": args.reps,
           "rows": int(sum(test[d]["uid"].shape[0] for d in domains)), "device": torch.cuda.get_device_name(eng.device)}
    if args.leg == "a":
        def call():
            for d in domains:
                eng.evaluate(d, "test")
    elif args.leg == "b":
        def call():
            for d in domains:
                eng.evaluate(d, "test", want_gauc=True)
    else:
        def call():
            for d in domains:
                _, _, _, preds = eng.evaluate(d, "test", want_preds=True)
                gauc.group_auc_host(preds, test[d]["label"], test[d]["uid"])
    res["ms"] = timed(eng, call, args.reps)
    # after the clock: the leg's predictions and T_u, for the parent's comparison
    preds = {d: eng.evaluate(d, "test", want_preds=True)[3] for d in domains}
    res["pred_sha"] = sha(preds[d] for d in domains)
    if args.leg == "b":
        reps = {d: eng.group_auc(torch.from_numpy(preds[d]).to(eng.device), eng.data[(d, "test")]["label"],
                                 eng.group_auc_plan(d, "test"), want_groups=True) for d in domains}
        # the launches alone, back to back
        dev = {d: (torch.from_numpy(preds[d]).to(eng.device), eng.data[(d, "test")]["label"], eng.group_auc_plan(d, "test"))
               for d in domains}

        def launches():
            for d in domains:
                eng._group_auc_launch(*dev[d])
        res["kernel_ms"] = timed(eng, launches, 4 * args.reps)
    elif args.leg == "c":
        reps = {d: gauc.group_auc_host(preds[d], test[d]["label"], test[d]["uid"], want_groups=True) for d in domains}
    if args.leg in ("b", "c"):
        res["T_sha"] = sha(reps[d]["T"] for d in domains)
        res["groups"] = int(sum(reps[d]["n_groups"] for d in domains))
        res["valid"] = int(sum(reps[d]["n_valid"] for d in domains))
        res["largest_group"] = int(max(np.bincount(np.unique(test[d]["uid"], return_inverse=True)[1]).max() for d in domains))
        res["gauc"] = [reps[d]["gauc"] for d in domains]
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="taobao10,amazon6,amazon6-hot")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input", default=None)
    ap.add_argument("--leg", default=None, choices=["a", "b", "c"])
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauc_bench.txt"))
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    for name in args.inputs.split(","):
        got = {}
        for which in ("a", "b", "c"):          # one child per leg, each under its own time limit; a failed leg ends the run
            cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", which,
                   "--input", name, "--reps", str(args.reps)]
            run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                raise SystemExit("input %s leg %s failed (exit %d): nothing further is started" % (name, which, run.returncode))
            got[which] = json.loads(lines[-1][7:])
        a, b, c = got["a"], got["b"], got["c"]
        if not (a["pred_sha"] == b["pred_sha"] == c["pred_sha"]):
            raise SystemExit("input %s: the legs' predictions differ: %s" % (name, [got[k]["pred_sha"] for k in "abc"]))
        if b["T_sha"] != c["T_sha"] or (b["groups"], b["valid"]) != (c["groups"], c["valid"]):
            raise SystemExit("input %s: device and host disagree on T_u: %s / %s" % (name, b["T_sha"], c["T_sha"]))
        nbytes = 12 * b["rows"] + 8 * b["groups"]
        rate = nbytes / (b["kernel_ms"] * 1e-3)
        text = ("%s  %s  input %s: %d rows, %d groups (%d valid, largest %d rows), %d evaluate call(s) per rep, %d reps "
                "(HIP events, 2 warm-up calls, a process per leg)\n"
                "  a  evaluate                                  %10.3f ms / rep\n"
                "  b  evaluate(want_gauc=True)                  %10.3f ms / rep   b - a %9.3f ms\n"
                "  c  evaluate(want_preds=True) + host GAUC     %10.3f ms / rep   c - a %9.3f ms   (c - a) / (b - a) %.1fx\n"
                "  mamdr_group_auc alone, back to back          %10.3f ms / rep   %d bytes (12 n + 8 G) -> %.1f GB/s = %.2f %% of "
                "the 8 TB/s HBM peak\n"
                "  predictions identical in all legs (sha %s); T_u of every group identical in b and c (sha %s)\n" % (
                    time.strftime("%Y-%m-%d"), b["device"], name, b["rows"], b["groups"], b["valid"], b["largest_group"],
                    b["domains"], b["reps"], a["ms"], b["ms"], b["ms"] - a["ms"], c["ms"], c["ms"] - a["ms"],
                    (c["ms"] - a["ms"]) / (b["ms"] - a["ms"]) if b["ms"] > a["ms"] else float("inf"),
                    b["kernel_ms"], nbytes, rate / 1e9, 100.0 * rate / HBM_PEAK, b["pred_sha"], b["T_sha"]))
        print(text)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
