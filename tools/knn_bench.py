"""mamdr_row_neighbours beside torch on the same GPU:

    python tools/knn_bench.py [--out profiles/knn_bench.txt]          every leg, one process each
    python tools/knn_bench.py --leg ours:6932:10                      one leg: <ours|torch>:<rows>:<k>

Problems: an all-against-all call (every row a query, every row a candidate, self excluded) over a standard-normal fp32
table (seed 7) of 6,932 x 128 -- the shape of Taobao-10's item table -- and of 100,000 x 128, at k = 10 and k = 100.
The yardstick: torch on the same device -- the rows normalised once (inside the timed call: the device call forms its norms
inside too), `matmul` of blocks of 4,096 queries against all rows, the diagonal set to -inf, `topk`.
Method: two warm-up calls, then five calls, each between two HIP events of its own on the current stream; the median is
reported.  One process per leg, so that no leg inherits another's allocator or clocks.  Per leg: ms per call, pairs / s,
and the contraction's 2 E flop per pair as a share of the 157.3 Tflop/s fp32 matrix peak.  Before a time is reported, the
first 256 queries' device lists are checked against the float64 definition (neighbours_host's rules: every pick within two
error bounds of the float64 k-th best).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 157.3e12
LEGS = [(who, n, k) for n in (6932, 100000) for k in (10, 100) for who in ("ours", "torch")]
E = 128


def timed(fn):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def leg(who, n, k):
    import ctypes as C
    import torch
    from mamdr_amd import _lib
    from mamdr_amd import list_metrics as lm
    if not torch.cuda.is_available():
        sys.exit("knn_bench: no HIP device (a CPU run gives no time)")
    rows = np.random.RandomState(7).standard_normal((n, E)).astype(np.float32)
    d_rows = torch.from_numpy(rows).cuda()
    ids = torch.empty((n, k), dtype=torch.int32, device="cuda")
    sims = torch.empty((n, k), dtype=torch.float32, device="cuda")
    if who == "ours":
        lib = _lib.load()
        q = torch.arange(n, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        run = lambda: _lib.check(lib.mamdr_row_neighbours(p(d_rows), n, E, p(q), n, None, n, 1, k, p(ids), p(sims), s))     # noqa: E731
    else:
        def run():
            x = d_rows / d_rows.norm(dim=1, keepdim=True)
            for b0 in range(0, n, 4096):
                c = x[b0:b0 + 4096] @ x.T
                c[torch.arange(c.shape[0], device="cuda"), torch.arange(b0, b0 + c.shape[0], device="cuda")] = float("-inf")
                v, i = torch.topk(c, k, dim=1)
                sims[b0:b0 + 4096], ids[b0:b0 + 4096] = v, i.to(torch.int32)
    run()
    got = ids[:256].cpu().numpy()
    x = rows.astype(np.float64)
    norm = np.sqrt((x * x).sum(1))
    ref = (x[:256] @ x.T) / (norm[:256, None] * norm[None, :])
    ref[np.arange(256), np.arange(256)] = -np.inf
    kth = -np.sort(-ref, axis=1)[:, k - 1]
    worst = float((kth[:, None] - np.take_along_axis(ref, got.astype(np.int64), 1)).max())
    assert worst <= 2 * lm.error_bound(E), (who, n, k, worst)
    med, lo, hi = timed(run)
    pairs = float(n) * n
    print("%-5s %7d x %3d all-against-all  k = %3d   median %10.3f ms  (min %10.3f  max %10.3f)   %9.3e pairs/s   "
          "%5.1f %% of the fp32 matrix peak" % (who, n, E, k, med, lo, hi, pairs / (med * 1e-3),
                                                 100.0 * pairs * 2 * E / (med * 1e-3) / PEAK), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        who, n, k = args.leg.split(":")
        return leg(who, int(n), int(k))
    lines = ["row neighbours: all-against-all over a standard-normal fp32 table, self excluded; 5 calls after 2 warm-up calls, "
             "one process per leg"]
    for who, n, k in LEGS:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "%s:%d:%d" % (who, n, k)], stdout=subprocess.PIPE,
                             universal_newlines=True, timeout=240)
        if res.returncode != 0:
            sys.exit("knn_bench: leg %s:%d:%d ended with %d" % (who, n, k, res.returncode))
        lines.append("  " + res.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
