"""mamdr_list_similarity and mamdr_id_counts beside the numpy host definitions on the same machine:

    python tools/list_metrics_bench.py [--lists 8192] [--k 100] [--emb-dim 128] [--items 200000] [--reps 20]
                                       [--host-lists 512] [--out profiles/list_metrics.txt]

Method: a standard-normal fp32 item table (seed 7) of `items` rows, `lists` lists of uniformly drawn ids (seed 8), every tenth
list short (padded with -1).  The device calls: two warm-up calls, then `reps` calls, each between two HIP events of
its own on the current stream -- min / median / max in ms; the lists and the table are already on the device, as they are
when the report runs.  The host route: list_metrics.list_similarity_host (float64 numpy) on the first `host-lists` lists,
timed with a host clock and scaled to all lists (it is linear in the lists), plus the device-to-host gather it would need
(Q * K * E floats) counted in bytes, not timed.  Before anything is reported the device result is checked against the host
definition within the derived bound pairs * (2 E + 8) * 2^-24 on those lists.
Work: per list 10 upper-triangle 32 x 32 tiles x E / 2 v_mfma_f32_32x32x2_f32 = 2 * 32 * 32 * E flop per tile; bytes: K rows
of 4 E bytes per list, gathered once.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--lists", type=int, default=8192)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--emb-dim", type=int, default=128)
    ap.add_argument("--items", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-lists", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C
    import torch
    from mamdr_amd import _lib
    from mamdr_amd import list_metrics as lm
    if not torch.cuda.is_available():
        sys.exit("list_metrics_bench: no HIP device (a CPU run gives no time)")
    lib = _lib.load()
    Q, K, E, n = args.lists, args.k, args.emb_dim, args.items
    rows = np.random.RandomState(7).standard_normal((n, E)).astype(np.float32)
    rs = np.random.RandomState(8)
    ids = rs.randint(0, n, (Q, K)).astype(np.int32)
    for q in range(0, Q, 10):
        ids[q, rs.randint(1, K):] = -1
    d_rows, d_ids = torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda()
    sim = torch.empty(Q, dtype=torch.float64, device="cuda")
    pairs = torch.empty(Q, dtype=torch.int32, device="cuda")
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    run_sim = lambda: _lib.check(lib.mamdr_list_similarity(p(d_ids), Q, K, p(d_rows), n, E, p(sim), p(pairs), s))      # noqa: E731
    run_cnt = lambda: _lib.check(lib.mamdr_id_counts(p(d_ids), None, Q * K, n, p(counts), s))      # noqa: E731
    run_sim()
    run_cnt()
    H = min(args.host_lists, Q)
    t0 = time.perf_counter()
    h_sim, h_pairs = lm.list_similarity_host(ids[:H], rows)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    h_counts = lm.id_counts_host(ids, n)
    host_cnt_s = time.perf_counter() - t0
    got_sim, got_pairs = sim.cpu().numpy(), pairs.cpu().numpy()
    assert np.array_equal(got_pairs[:H], h_pairs)
    worst = float((np.abs(got_sim[:H] - h_sim) / np.maximum(h_pairs, 1) / lm.error_bound(E)).max())
    assert worst <= 1.0, worst
    assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), h_counts)
    k_sim, k_cnt = timed(run_sim, args.reps), timed(run_cnt, args.reps)
    tiles = sum(t * (t + 1) // 2 for t in (-(-(int(L)) // 32) for L in (ids >= 0).sum(1)))
    flop = tiles * 2.0 * 32 * 32 * E
    gathered = float((ids >= 0).sum()) * 4 * E
    host_all = host_s * Q / H
    lines = ["list similarity: %d lists of K = %d (every tenth short) over a %d x %d fp32 table, %d reps after 2 warm-up calls" %
             (Q, K, n, E, args.reps),
             "  mamdr_list_similarity        min %8.3f  median %8.3f  max %8.3f ms   %6.2f TFLOP/s on the fp32 matrix cores "
             "(upper-triangle tiles), %6.1f GB/s of rows gathered" % (k_sim + (flop / (k_sim[1] * 1e-3) / 1e12,
                                                                              gathered / (k_sim[1] * 1e-3) / 1e9)),
             "  list_similarity_host (numpy) %8.1f ms for %d lists on the host -> %.1f ms for all %d (linear in the lists); "
             "it would first copy %.1f MB of gathered rows off the device" % (host_s * 1e3, H, host_all * 1e3, Q, gathered / 1e6),
             "  device / host = 1 / %.0f (median over scaled host time); worst |sim_sum - host| / (pairs * (2 E + 8) * 2^-24) = %.4f"
             % (host_all * 1e3 / k_sim[1], worst),
             "id counts: %d ids into %d bins" % (Q * K, n),
             "  mamdr_id_counts              min %8.3f  median %8.3f  max %8.3f ms" % k_cnt,
             "  id_counts_host (np.bincount) %8.3f ms" % (host_cnt_s * 1e3)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
