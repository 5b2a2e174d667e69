"""mamdr_gram beside what a user would otherwise write on the same device tensor, `V.double() @ V.double().T`:

    taobao10-mlp   30 vectors x the flat-vector length of the Taobao-10 mlp tower (frozen tables)
    16M            30 vectors x 16,777,216 columns

    python tools/conflict_bench.py [--shapes taobao10-mlp,16M] [--reps 5] [--out profiles/conflict_bench.txt]

Method: standard-normal fp32 data (seed 7), one range = the whole vector, the workspace allocated before the timed region
(FlatVectorOps.gram keeps it).  Two warm-up calls, then `reps` calls, each between two HIP events of its own on the current
stream: min / median / max in ms.  The kernel reads every fp32 value once (GB/s = 4 D n bytes over the median); the torch
route writes a converted fp64 copy and reads it back.  Both results are checked against each other within the summation
bound 2 n 2^-53 |V| |V|^T before anything is reported.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 30


def columns(shape):
    if shape == "16M":
        return 1 << 24
    from mamdr_amd import synthetic
    from mamdr_amd.engine import TowerEngine
    s = synthetic.SHAPES["taobao10"]
    eng = TowerEngine(s["n_user"], s["n_item"], s["n_domain"], 1024, emb_trainable=False, tower="mlp")
    n = eng.n_params
    eng.close()
    return n


def timed(fn, reps):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms)), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="taobao10-mlp,16M")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mamdr_amd import _lib
    from mamdr_amd.engine import FlatVectorOps
    ops = FlatVectorOps()
    ops.lib, ops.stream = _lib.load(), torch.cuda.current_stream()
    lines = []
    for shape in args.shapes.split(","):
        n = columns(shape)
        gen = torch.Generator(device="cuda").manual_seed(7)
        V = torch.randn((D, n), dtype=torch.float32, device="cuda", generator=gen)
        ranges = [(0, n)]
        got = ops.gram(V, ranges)[0]
        Vd = V.double()
        ref = Vd @ Vd.T
        bound = 2 * n * 2.0 ** -53 * (Vd.abs() @ Vd.abs().T)
        worst = float(((got - ref).abs() / bound).max())
        assert worst <= 1.0, worst
        assert torch.equal(got, got.T)
        del Vd, ref, bound
        k = timed(lambda: ops.gram(V, ranges), args.reps)
        t = timed(lambda: V.double() @ V.double().T, args.reps)
        slabs = -(-n // _lib.GRAM_SLAB)
        verdict = "not slower" if k[1] <= t[1] + (t[2] - t[0]) + (k[2] - k[0]) else "SLOWER"
        lines += ["%s: %d vectors x %d columns (%d slabs, %.1f MB workspace), %d reps after 2 warm-up calls" %
                  (shape, D, n, slabs, slabs * D * D * 8 / 1e6, args.reps),
                  "  mamdr_gram                   min %8.3f  median %8.3f  max %8.3f ms   %7.1f GB/s of fp32 read once" %
                  (k + (4.0 * D * n / (k[1] * 1e-3) / 1e9,)),
                  "  V.double() @ V.double().T    min %8.3f  median %8.3f  max %8.3f ms" % t,
                  "  kernel / torch = %.3f (medians): the kernel is %s than the torch route beyond the spread of the repeats; "
                  "worst |G - G_torch| / (2 n u |V| |V|^T) = %.2e" % (k[1] / t[1], verdict, worst)]
        del V
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
