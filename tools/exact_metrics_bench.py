"""What the exact AUC / average precision / calibration bins cost, on the device (mamdr_exact_metrics) and on the host
(exact.metrics_host), and what they add to an evaluation, at n = 10^4, 10^5, 10^6 and 10^7 rows:

    python tools/exact_metrics_bench.py [--sizes 10000,100000,1000000,10000000] [--reps 21] [--bins 20]
                                        [--out profiles/exact_metrics_bench.txt]

Per size, in a child process of its own under `timeout -k 10` (a failed size ends the run):
    device    mamdr_exact_metrics alone on device tensors: every call between two HIP events of its own on the engine's
              stream, 3 warm-up calls, the median of `reps`.  Bytes the chain moves: 5 sort passes of 24 n (the histogram reads
              8 n, the scatter reads and writes 8 n each) + 8 n for the runs + 8 n for the metrics = 136 n, against the 8 TB/s
              HBM peak of the MI355X.
    host      exact.metrics_host on the same arrays (host clock, median of min(reps, 5)).
    evaluate  evaluate(0, "test") and evaluate(0, "test", want_exact=bins) on a synthetic split of n rows (mlp tower, frozen
              random tables of 20,000 users x 5,000 items, random weights, eval batch 1,024): host clock around calls that end
              in their own read-back, 3 warm-up calls, medians, the two forms alternating.
Data: logit ~ N(-4.55, 0.5), labels drawn from the prediction (1.2 % positives), seed 7.  The child refuses to report
unless every integer of the device call equals the host's and the AP sums agree within n * 2^-52.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s
N_USER, N_ITEM = 20000, 5000


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def child(args):
    import torch
    from mamdr_amd import exact
    from mamdr_amd.engine import TowerEngine
    n, bins = args.n, args.bins
    rs = np.random.RandomState(7)
    pred = (1.0 / (1.0 + np.exp(-rs.normal(-4.55, 0.5, n)))).astype(np.float32)
    label = (rs.random_sample(n) < pred).astype(np.float32)
    eng = TowerEngine(N_USER, N_ITEM, 1, 1024, dropout=0.0, emb_trainable=False, tower="mlp")
    eng.bind_table("user_emb", (rs.standard_normal((N_USER, 128)) * 0.05).astype(np.float32))
    eng.bind_table("item_emb", (rs.standard_normal((N_ITEM, 128)) * 0.05).astype(np.float32))
    eng.set_weights(eng.pack({k: (rs.standard_normal(cnt) * 0.06).astype(np.float32) for k, (off, cnt) in eng.segments.items()}))
    eng.bind_domain_data(0, "test", rs.randint(0, N_USER, n), rs.randint(0, N_ITEM, n), np.zeros(n, np.int32), label)
    res = {"n": n, "bins": bins, "reps": args.reps, "device": torch.cuda.get_device_name(eng.device),
           "positives": int(label.sum())}
    # device: the call alone
    d_pred, d_label = torch.from_numpy(pred).to(eng.device), torch.from_numpy(label).to(eng.device)
    for _ in range(3):
        out = eng._exact_launch(d_pred, d_label, bins)
    torch.cuda.synchronize(eng.device)
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(eng.stream)
        out = eng._exact_launch(d_pred, d_label, bins)
        b.record(eng.stream)
        torch.cuda.synchronize(eng.device)
        ms.append(a.elapsed_time(b))
    res["device_ms"], res["device_ms_min"], res["device_ms_max"] = median(ms), min(ms), max(ms)
    # host: the same arrays
    ms = []
    for _ in range(min(args.reps, 5)):
        t0 = time.perf_counter()
        want = exact.metrics_host(pred, label, bins)
        ms.append(1e3 * (time.perf_counter() - t0))
    res["host_ms"] = median(ms)
    got = [t.cpu().numpy() for t in out[:3]]
    if got[0].tolist() != want[0].tolist() or not np.array_equal(got[2], want[2]):
        raise SystemExit("n %d: device and host disagree on an integer: %s / %s" % (n, got[0].tolist(), want[0].tolist()))
    if abs(float(got[1][0]) - want[1]) > n * 2.0 ** -52 * want[1]:
        raise SystemExit("n %d: AP sums differ: %.17g / %.17g" % (n, float(got[1][0]), want[1]))
    rep = exact.finish(*got)
    res.update(auc=rep["auc"], ap=rep["ap"], ece=rep["ece"])
    # evaluate with and without the key, alternating
    plain, with_exact = [], []
    for i in range(3 + args.reps):
        for store, kw in ((plain, {}), (with_exact, {"want_exact": bins})):
            t0 = time.perf_counter()
            eng.evaluate(0, "test", **kw)
            if i >= 3:
                store.append(1e3 * (time.perf_counter() - t0))
    res["eval_ms"], res["eval_exact_ms"] = median(plain), median(with_exact)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--n", type=int, default=None, help="(the child's size)")
    ap.add_argument("--size-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_metrics_bench.txt"))
    args = ap.parse_args()
    if args.n is not None:
        return child(args)
    for n in [int(s) for s in args.sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.size_timeout), sys.executable, os.path.abspath(__file__), "--n", str(n),
               "--reps", str(args.reps), "--bins", str(args.bins)]
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not lines:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            raise SystemExit("n %d failed (exit %d): nothing further is started" % (n, run.returncode))
        r = json.loads(lines[-1][7:])
        rate = 136.0 * n / (r["device_ms"] * 1e-3)
        text = ("%s  %s  n %d (%d positives), %d bins, %d reps (medians; HIP events around every device call, host clock "
                "elsewhere; 3 warm-up calls; a process per size)\n"
                "  mamdr_exact_metrics alone                 %10.3f ms   (min %.3f max %.3f)   136 n bytes -> %.1f GB/s = %.2f %% "
                "of the 8 TB/s HBM peak\n"
                "  exact.metrics_host on the same arrays     %10.3f ms   host / device %.0fx\n"
                "  evaluate                                  %10.3f ms\n"
                "  evaluate(want_exact=%d)                   %10.3f ms   difference %.3f ms = %.1f %% of the evaluation\n"
                "  every integer identical on device and host; exact AUC %.6f  AP %.6f  ECE %.2e\n" % (
                    time.strftime("%Y-%m-%d"), r["device"], n, r["positives"], r["bins"], r["reps"],
                    r["device_ms"], r["device_ms_min"], r["device_ms_max"], rate / 1e9, 100.0 * rate / HBM_PEAK,
                    r["host_ms"], r["host_ms"] / r["device_ms"], r["eval_ms"], r["bins"], r["eval_exact_ms"],
                    r["eval_exact_ms"] - r["eval_ms"], 100.0 * (r["eval_exact_ms"] - r["eval_ms"]) / r["eval_ms"],
                    r["auc"], r["ap"], r["ece"]))
        print(text)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
