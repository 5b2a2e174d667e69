"""What the bootstrap replicates of the exact AUC cost on the device (mamdr_auc_bootstrap, units = rows and units = users),
beside mamdr_exact_metrics alone on the same tensors and bootstrap.replicates_host on the CPU:

    python tools/auc_bootstrap_bench.py [--n 200000] [--n-rep 1000] [--reps 21] [--out profiles/auc_bootstrap.txt]

Every device call sits between two HIP events of its own on torch's current stream; 3 warm-up calls, the median, minimum and
maximum of `reps`.  The host restatement runs once per unit (it takes seconds), on the host clock.  Data: logit ~
N(-4.55, 0.5), labels drawn from the prediction (1.2 % positives), users drawn uniformly from n / 10 ids, seed 7.  The tool
refuses to report unless every word of the device call equals the host's.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--n-rep", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_bootstrap.txt"))
    args = ap.parse_args()
    import torch
    from mamdr_amd import _lib as L
    from mamdr_amd import bootstrap
    lib = L.load()
    n, n_rep = args.n, args.n_rep
    rs = np.random.RandomState(7)
    pred = (1.0 / (1.0 + np.exp(-rs.normal(-4.55, 0.5, n)))).astype(np.float32)
    label = (rs.random_sample(n) < pred).astype(np.float32)
    uid = rs.randint(0, max(n // 10, 1), n).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_pred, d_label, d_uid = [torch.from_numpy(a).to(dev) for a in (pred, label, uid)]
    T, P, N = [torch.empty(n_rep + 1, dtype=torch.int64, device=dev) for _ in range(3)]
    counts = torch.empty(5, dtype=torch.int64, device=dev)
    ap_sum = torch.empty(1, dtype=torch.float64, device=dev)
    bins = torch.empty((3, 20), dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731

    def boot(unit):
        L.check(lib.mamdr_auc_bootstrap(p(d_pred), p(d_label), p(unit), n, n_rep, args.seed, p(T), p(P), p(N), stream()))

    def exact_call():
        L.check(lib.mamdr_exact_metrics(p(d_pred), p(d_label), n, 20, p(counts), p(ap_sum), p(bins), None, stream()))

    lines = ["%s  %s  n %d (%d positives, %d users), %d replicates, tile %d, group %d; %d reps (median, min, max; HIP events "
             "around every call; 3 warm-up calls)" % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(dev), n,
                                                      int(label.sum()), np.unique(uid).size, n_rep, bootstrap.TILE,
                                                      bootstrap.GROUP, args.reps)]
    lines.append("  mamdr_exact_metrics alone                       %10.3f ms   (min %.3f max %.3f)" % timed(exact_call, args.reps))
    for name, d_unit, unit in (("rows", None, None), ("users", d_uid, uid)):
        dev_ms = timed(lambda: boot(d_unit), args.reps)
        got = [t.cpu().numpy() for t in (T, P, N)]
        t0 = time.perf_counter()
        want = bootstrap.replicates_host(pred, label, n_rep, args.seed, unit)
        host_ms = 1e3 * (time.perf_counter() - t0)
        if not all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want)):
            raise SystemExit("units = %s: device and host disagree on an integer" % name)
        rep = bootstrap.finish(*want)
        lines.append("  mamdr_auc_bootstrap, units = %-5s               %10.3f ms   (min %.3f max %.3f)   %.1f ps per (row, "
                     "replicate)" % ((name,) + dev_ms + (1e9 * dev_ms[0] / (n * float(n_rep + 1)),)))
        lines.append("  bootstrap.replicates_host, units = %-5s         %10.1f ms   host / device %.0fx; every word identical; "
                     "AUC %.6f se %.6f [%.6f, %.6f], %d valid" % (name, host_ms, host_ms / dev_ms[0], rep["auc"], rep["se"],
                                                                 rep["ci_lo"], rep["ci_hi"], rep["n_valid"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
