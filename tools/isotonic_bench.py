"""What the isotonic fit, its application and the score sums cost on the device (mamdr_isotonic_fit, mamdr_isotonic_apply,
mamdr_score_sums), beside isotonic.fit_host and scikit-learn's IsotonicRegression on the same arrays, at n = 10^5, 10^6 and
4 * 10^6 rows of three kinds of data:

    python tools/isotonic_bench.py [--sizes 100000,1000000,4000000] [--kinds continuous,q1024,convex] [--reps 11]
                                   [--out profiles/isotonic_bench.txt]

Per (kind, size), in a child process of its own under `timeout -k 10` (a failed one ends the run):
    device    each of the three calls alone on device tensors, on torch's current stream: every call between two HIP events
              of its own, 3 warm-up calls, the median of `reps`.  The fit is applied to the rows it was fitted on.
    host      isotonic.fit_host and sklearn.isotonic.IsotonicRegression(out_of_bounds="clip").fit on the same arrays (host
              clock, one call each: fit_host walks the runs in Python).
    levels    the points alive before every level of the hull and before its final chain at the default tile of 64 points
              (isotonic.level_counts_host: the device keeps these counts to itself).
Data, seed 7.  continuous: logit ~ N(-2, 1.5), labels drawn from the prediction.  q1024: the same, predictions rounded to
1/1024.  convex: the strictly convex worst case -- one run per term a / b of the Farey sequence whose order makes the rows
add up to n, in ascending order, b rows with a positives: every run is its own block and no level drops a point.  Its
points grow as n^(2/3) only: distinct rates need distinct fractions, and the rows are the sum of their denominators.
The child refuses to report unless the device's table equals fit_host's, the applied values are apply_host's bits and the
score sums agree with score_sums_host within a relative 1e-12.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def farey_runs(n):
    """(denominators, numerators) of the Farey sequence of the smallest order whose denominators add up to >= n, cut
    where they reach n."""
    order = max(1, int(round((5.0 * n) ** (1.0 / 3.0))) - 2)
    while True:
        a, b, c, d = 0, 1, 1, order
        den, num = [1], [0]
        while c <= order:
            k = (order + b) // d
            a, b, c, d = c, d, k * c - a, k * d - b
            den.append(b)
            num.append(a)
        if sum(den) >= n:
            break
        order += 1
    den, num = np.asarray(den, np.int64), np.asarray(num, np.int64)
    keep = int(np.searchsorted(np.cumsum(den), n)) + 1
    return den[:keep], num[:keep]


def make(kind, n):
    rs = np.random.RandomState(7)
    if kind == "convex":
        den, num = farey_runs(n)
        runs = den.shape[0]
        pred = np.repeat(((np.arange(runs) + 1.0) / (runs + 1.0)).astype(np.float32), den)
        start = np.concatenate([[0], np.cumsum(den)])
        label = (np.arange(pred.shape[0]) - np.repeat(start[:-1], den) < np.repeat(num, den)).astype(np.float32)
        assert np.unique(pred).shape[0] == runs
        return pred, label
    logit = rs.normal(-2.0, 1.5, n)
    pred = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    label = (rs.random_sample(n) < pred).astype(np.float32)
    if kind == "q1024":
        pred = (np.round(pred * 1024) / 1024).astype(np.float32)
    return pred, label


def child(args):
    import torch
    from sklearn.isotonic import IsotonicRegression
    from mamdr_amd import _lib as L
    from mamdr_amd import isotonic
    lib = L.load()
    pred, label = make(args.kind, args.n)
    n = int(pred.shape[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    d_pred, d_label = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    fk = torch.empty(n, dtype=torch.int32, device=dev)
    rows, pos = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    res = {"kind": args.kind, "n": n, "reps": args.reps, "device": torch.cuda.get_device_name(dev), "positives": int(label.sum())}

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b))
        return [median(ms), min(ms), max(ms)]

    res["fit_ms"] = timed(lambda: L.check(lib.mamdr_isotonic_fit(ptr(d_pred), ptr(d_label), n, ptr(counts), ptr(fk), ptr(rows),
                                                                 ptr(pos), stream())))
    got_counts = counts.cpu().numpy()
    nb = int(got_counts[0])
    res["apply_ms"] = timed(lambda: L.check(lib.mamdr_isotonic_apply(ptr(fk), ptr(rows), ptr(pos), nb, ptr(d_pred), n, ptr(out),
                                                                     stream())))
    res["sums_ms"] = timed(lambda: L.check(lib.mamdr_score_sums(ptr(d_pred), ptr(d_label), n, ptr(sums), stream())))
    t0 = time.perf_counter()
    want = isotonic.fit_host(pred, label)
    res["host_ms"] = 1e3 * (time.perf_counter() - t0)
    x64, y64 = pred.astype(np.float64), label.astype(np.float64)
    t0 = time.perf_counter()
    IsotonicRegression(out_of_bounds="clip").fit(x64, y64)
    res["sklearn_ms"] = 1e3 * (time.perf_counter() - t0)
    got = (got_counts, fk[:nb].cpu().numpy().view(np.uint32), rows[:nb].cpu().numpy(), pos[:nb].cpu().numpy())
    if not all(np.array_equal(g, w) for g, w in zip(got, want)):
        raise SystemExit("%s n %d: the device's fit and fit_host disagree: %s / %s" % (args.kind, n, got[0].tolist(), want[0].tolist()))
    if out.cpu().numpy().tobytes() != isotonic.apply_host(want[1], want[2], want[3], pred).tobytes():
        raise SystemExit("%s n %d: the applied values differ from apply_host's" % (args.kind, n))
    host_sums, dev_sums = isotonic.score_sums_host(pred, label), sums.cpu().numpy()
    if not all(abs(g - w) <= 1e-12 * w for g, w in zip(dev_sums.tolist(), host_sums)):
        raise SystemExit("%s n %d: score sums differ: %s / %s" % (args.kind, n, dev_sums.tolist(), host_sums))
    res.update(zip(isotonic.COUNTS, [int(v) for v in got_counts]))
    res["alive"] = isotonic.level_counts_host(pred, label, isotonic.HULL_TILE)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--kinds", default="continuous,q1024,convex")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--n", type=int, default=None, help="(the child's size)")
    ap.add_argument("--kind", default=None, help="(the child's data)")
    ap.add_argument("--case-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isotonic_bench.txt"))
    args = ap.parse_args()
    if args.n is not None:
        return child(args)
    for kind in args.kinds.split(","):
        for n in [int(s) for s in args.sizes.split(",")]:
            cmd = ["timeout", "-k", "10", str(args.case_timeout), sys.executable, os.path.abspath(__file__), "--n", str(n),
                   "--kind", kind, "--reps", str(args.reps)]
            run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                raise SystemExit("%s n %d failed (exit %d): nothing further is started" % (kind, n, run.returncode))
            r = json.loads(lines[-1][7:])
            text = ("%s  %s  %s, n %d (%d positives): %d runs, %d blocks, %d NaN; %d reps (medians; HIP events around every "
                    "device call, host clock elsewhere; 3 warm-up calls; a process per case)\n"
                    "  mamdr_isotonic_fit                        %10.3f ms   (min %.3f max %.3f)\n"
                    "  mamdr_isotonic_apply (the fitted rows)    %10.3f ms   (min %.3f max %.3f)\n"
                    "  mamdr_score_sums                          %10.3f ms   (min %.3f max %.3f)\n"
                    "  isotonic.fit_host on the same arrays      %10.3f ms   host / device %.0fx\n"
                    "  sklearn IsotonicRegression.fit            %10.3f ms   sklearn / device %.1fx\n"
                    "  points alive before each level of 64-point tiles, then before the final chain: %s\n"
                    "  the device's table equals fit_host's; applied values bit-equal; score sums within 1e-12\n" % (
                        time.strftime("%Y-%m-%d"), r["device"], r["kind"], r["n"], r["positives"], r["n_runs"], r["n_blocks"],
                        r["n_nan"], r["reps"], *r["fit_ms"], *r["apply_ms"], *r["sums_ms"], r["host_ms"],
                        r["host_ms"] / r["fit_ms"][0], r["sklearn_ms"], r["sklearn_ms"] / r["fit_ms"][0],
                        " -> ".join(str(a) for a in r["alive"])))
            print(text, flush=True)
            with open(args.out, "a") as f:
                f.write(text)


if __name__ == "__main__":
    main()
