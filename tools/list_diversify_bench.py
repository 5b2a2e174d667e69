"""mamdr_list_diversify beside mamdr_list_similarity at the same shape and beside the numpy host definition on the same machine:

    python tools/list_diversify_bench.py [--lists 7133] [--emb-dim 128] [--items 6932] [--reps 20] [--host-lists 256]
                                         [--lam 0.7] [--out profiles/list_diversify.txt]

Shapes: Q = `lists` = the users of one full-size taobao10 domain (synthetic.py: 3 / 10 of 23,778 users; the report makes one call
per domain), pools of n = 50 and 128 DISTINCT uniformly drawn ids (seed 8) over a standard-normal fp32 item table (seed 7) of
`items` rows, every tenth list short (padded with -1), k = 10 and 20.  Relevance: sigmoid(N(-3, 1)) scores in descending order
(a pool arrives ranked), min-max scaled per list (list_metrics.minmax_relevance).
Method: two warm-up calls, then `reps` calls, each between two HIP events of its own on the current stream -- min / median /
max in ms; lists, relevance and table are already on the device, as they are when the report runs.  mamdr_list_similarity at
the same (Q, n, E) is timed the same way: what mamdr_list_diversify costs beyond it is phase 2 (the k greedy steps) and the LDS
cosine matrix.  The host route: list_metrics.diversify_host (float64 numpy) on the first `host-lists` lists, timed with a
host clock and scaled to all lists (it is linear in the lists).  Before anything is reported every device pick of those lists
is checked against the float64 definition: within 2 tol of its step's best (list_metrics.diversify_audit, diversify_tol).
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


def pools(Q, n, n_item, seed):
    rs = np.random.RandomState(seed)
    ids = np.stack([rs.choice(n_item, n, replace=False) for _ in range(Q)]).astype(np.int32)
    for q in range(0, Q, 10):
        ids[q, rs.randint(1, n + 1):] = -1
    scores = -np.sort(-(1.0 / (1.0 + np.exp(-rs.normal(-3.0, 1.0, (Q, n))))), axis=1)
    return ids, scores.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=7133)
    ap.add_argument("--emb-dim", type=int, default=128)
    ap.add_argument("--items", type=int, default=6932)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-lists", type=int, default=256)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        sys.exit("list_diversify_bench: at least 5 timed calls")
    import ctypes as C
    import torch
    from mamdr_amd import _lib
    from mamdr_amd import list_metrics as lm
    if not torch.cuda.is_available():
        sys.exit("list_diversify_bench: no HIP device (a CPU run gives no time)")
    lib = _lib.load()
    Q, E, n_item, lam = args.lists, args.emb_dim, args.items, args.lam
    rows = np.random.RandomState(7).standard_normal((n_item, E)).astype(np.float32)
    d_rows = torch.from_numpy(rows).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H = min(args.host_lists, Q)
    tol = lm.diversify_tol(E, lam)
    lines = ["list diversify: %d lists (every tenth short) over a %d x %d fp32 table, lambda %g, %d reps after 2 warm-up calls"
             % (Q, n_item, E, lam, args.reps)]
    for n in (50, 128):
        ids, scores = pools(Q, n, n_item, 8 + n)
        rel = lm.minmax_relevance(scores, ids, n_item)
        d_ids, d_rel = torch.from_numpy(ids).cuda(), torch.from_numpy(rel).cuda()
        sim = torch.empty(Q, dtype=torch.float64, device="cuda")
        pairs = torch.empty(Q, dtype=torch.int32, device="cuda")
        run_sim = lambda: _lib.check(lib.mamdr_list_similarity(p(d_ids), Q, n, p(d_rows), n_item, E, p(sim), p(pairs), s))    # noqa: E731
        k_sim = timed(run_sim, args.reps)
        lines.append("  n = %3d  mamdr_list_similarity          min %8.3f  median %8.3f  max %8.3f ms   (phase 1 alone, summed)"
                     % ((n,) + k_sim))
        for k in (10, 20):
            pos = torch.empty((Q, k), dtype=torch.int32, device="cuda")
            val = torch.empty((Q, k), dtype=torch.float32, device="cuda")
            run_div = lambda: _lib.check(lib.mamdr_list_diversify(p(d_ids), p(d_rel), Q, n, k, lam, p(d_rows), n_item, E,   # noqa: E731
                                                                  p(pos), p(val), s))
            run_div()
            got = pos.cpu().numpy()
            t0 = time.perf_counter()
            h_pos, _ = lm.diversify_host(ids[:H], rel[:H], rows, k, lam)
            host_s = time.perf_counter() - t0
            worst = float(lm.diversify_audit(ids[:H], rel[:H], rows, got[:H], lam)[0].max())
            assert worst <= 2 * tol, (n, k, worst, tol)
            same = float((got[:H] == h_pos).all(axis=1).mean())
            k_div = timed(run_div, args.reps)
            lines.append("  n = %3d  mamdr_list_diversify k = %2d   min %8.3f  median %8.3f  max %8.3f ms   = similarity + %.3f ms"
                         % ((n, k) + k_div + (k_div[1] - k_sim[1],)))
            lines.append("           diversify_host (numpy)        %8.1f ms for %d lists -> %.1f ms for all %d; device / host = 1 / %.0f; "
                         "%.1f %% of those lists equal the host's, worst float64 shortfall / (2 tol) = %.4f"
                         % (host_s * 1e3, H, host_s * 1e3 * Q / H, Q, host_s * 1e3 * Q / H / k_div[1], 100.0 * same,
                            worst / (2 * tol)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
