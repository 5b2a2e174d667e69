"""bench.py -- domain-steps/sec of the MAMDR hot path on N MI355X GPUs of one node.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`.  For N > 1 the driver launches it as
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (one rank per GPU, RCCL); started
WITHOUT a rendezvous (`python bench.py --gpus N`, no WORLD_SIZE) it starts that launcher itself as a child
process -- before anything touches the GPU -- and relays the child's one JSON line and exit code.
Rank 0 prints ONE JSON line.

Workload (BASELINE.json configs[1]): mlp_meta_mamdr, Taobao-10 shaped synthetic click logs, batch 1024,
pretrained 128-d tables frozen, Adam lr 1e-3, dropout 0.5, meta lr 0.1, 5 sampled support domains + the query
domain (config/Taobao-10/deepctr_DN+DR.json).  ONE bench "step" = one full MAMDR meta-epoch (DN phase over all
domains, then the DR phase: for every query domain and every support domain, a pass over the support domain
and a pass over the query domain, with all outer updates), i.e. `domain_steps_per_epoch` inner optimisation
steps (gather + MLP fwd/bwd + BCE + Adam).  value = inner domain-steps executed by all ranks / wall time of
the K epochs (max over ranks), inputs resident in HBM, the epoch's shuffles generated on the host and uploaded
(one copy per epoch) inside the timed region, no eval inside it.

N > 1: every epoch's DR query domains and DN passes are dealt to the ranks by longest-processing-time on the
cost THAT epoch's sampled plan will execute (mamdr_amd/parallel.py: BalancedMAMDR), with ONE all-reduce per
epoch (DN displacement + the phi hand-over); total work is fixed -> "scaling": "strong".

A plain run does only what the headline needs: set up, warm up, time the K epochs, print the line.  With `--full` the
JSON also carries the per-kernel figures of one more profiled epoch (`roofline`, `kernels_avg_us`, ...), `targets`
(Taobao-30 bs 4096 = BASELINE.json configs[3] / north_star, Amazon-6 and Amazon-13, same run), `gather` (the embedding
gather on Amazon-6-sized tables, 316 MB > the 256 MiB infinity cache), `cpu_baseline` (torch-CPU fp32 restatement of
the TF1.12 step on the host's cores) and `lanes`.

`--dump-outputs DIR` writes what the last timed epoch computed -- theta, phi [domains, P] and the engine's live weights
-- as DIR/<name>.npy (float32, 64 MB at most: larger vectors are cut to a fixed, seeded sample of positions).  The
timed epochs start from the same state in every run, so two builds can be compared output for output.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3    # MI355X_MICROARCH.md: dense fp32-input MFMA (= vector peak)
PEAK_HBM_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E spec
# algorithmic flops per batch row of k_tower<train> (kernel table):
#   forward 384*256 + 256*128 + 128*64 + 64 MACs, backward chain dz3->dz2->dz1: 64*128 + 128*256 MACs
#   (the per-row contraction with W0[256:384] is gone: the domain-table gradient uses linearity)
TOWER_TRAIN_FLOPS_PER_ROW = 2 * ((384 * 256 + 256 * 128 + 128 * 64 + 64) + (64 * 128 + 128 * 256))


def tower_flops_per_row(dx_width):
    """+ the input-gradient contraction dz1 . W0[0:dx_width, :]^T of the towers whose tables train: 256 columns
    ([user | item] rows, deepctr towers) or all 384 (Star: PartitionedNorm's backward needs d loss / d x)."""
    return TOWER_TRAIN_FLOPS_PER_ROW + 2 * 256 * dx_width


GATHER_BYTES_PER_ROW = 3 * 128 * 4 * 2 + 16   # read 3 rows + write 384 floats + 4 index/label words

WORKLOADS = {
    "taobao10": dict(shape="taobao10", batch=1024, name="mlp_meta_mamdr Taobao-10 bs=1024 (frozen pretrained tables)"),
    "taobao30": dict(shape="taobao30", batch=4096, name="mlp_meta_mamdr Taobao-30 bs=4096 (frozen pretrained tables)"),
    # trainable 128-d tables (79 M parameters): every step ends with TF1's dense Adam over all rows
    # (BASELINE.json configs[2]: DeepFM tower under Domain Negotiation)
    "amazon6": dict(shape="amazon6", batch=1024, emb_trainable=True, wrapper="dn", tower="deepfm",
                    name="deepfm_meta_domain_negotiation Amazon-6 bs=1024 (trainable tables, full-size tables, "
                         "{rows} of the rows per epoch)"),
    # (BASELINE.json configs[4]: Star tower under MAMDR, theta / phi over the tables + shared kernels / biases)
    "amazon13": dict(shape="amazon13", batch=8192, emb_trainable=True, wrapper="mamdr", tower="star",
                     name="star_meta_mamdr Amazon-13 bs=8192 (PartitionedNorm + StarFCN, trainable tables, "
                          "full-size tables, {rows} of the rows per epoch)"),
}
TARGET_KEYS = ("workload", "value", "unit", "us_per_domain_step", "ms_per_step", "epochs_timed", "domain_steps_per_epoch",
               "roofline", "tower", "table_update", "kernels_avg_us", "cpu_baseline", "gpu_over_cpu",
               "partition_speedup_bound", "host_ms_per_epoch", "host_prep_ms_per_epoch", "gather_in_step")
TRAIN = dict(learning_rate=1e-3, meta_learning_rate=0.1, sample_num=5, add_query_domain=True, dropout=0.5,
             merged_method="plus", shuffle_buffer_size=10000, seed=123)


def init_params(g, seed=1024):
    """random-init weights of the reference architecture (deepctr.py:118-136 initialisers)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    p = {"domain_emb": (rs.standard_normal((g["n_domain"], 128)) * 1e-4).astype(np.float32)}
    dims = (384, 256, 128, 64)
    for l in range(3):
        s = np.sqrt(2.0 / (dims[l] + dims[l + 1]))
        p["W%d" % l] = (np.clip(rs.standard_normal((dims[l], dims[l + 1])), -2, 2) * s).astype(np.float32)
        p["b%d" % l] = np.zeros(dims[l + 1], np.float32)
    p["wo"] = (np.clip(rs.standard_normal((64, 1)), -2, 2) * np.sqrt(2.0 / 65)).astype(np.float32)
    p["gb"] = np.zeros(1, np.float32)
    # DeepFM 1-d linear tables start at zero (deepctr get_linear_logit); ignored by the mlp tower
    p["lin_user"] = np.zeros(g["n_user"], np.float32)
    p["lin_item"] = np.zeros(g["n_item"], np.float32)
    p["lin_domain"] = np.zeros(g["n_domain"], np.float32)
    return p


if os.environ.get("MAMDR_LIB_PATH"):          # a diagnostic build of the library (tools/build_variant.sh): A/B measurements
    from mamdr_amd import _lib as _L
    _L.LIB_PATH = os.environ["MAMDR_LIB_PATH"]


def setup_engine(g, batch, emb_trainable=False, tower="mlp"):
    from mamdr_amd import engine
    eng = engine.TowerEngine(g["n_user"], g["n_item"], g["n_domain"], batch, dropout=TRAIN["dropout"],
                             emb_trainable=emb_trainable, tower=tower)
    if not emb_trainable:
        eng.bind_table("user_emb", g["tables"]["user_emb"])
        eng.bind_table("item_emb", g["tables"]["item_emb"])
    for d in range(g["n_domain"]):
        c = g["data"]["train"][d]
        eng.bind_domain_data(d, "train", c["uid"], c["pid"], c["domain"], c["label"])
    return eng


# ---------------------------------------------------------------------------------------------- CPU baseline
def _cpu_sample(g, batch, shuffle_perm):
    """the inner steps the CPU legs run: passes over the largest domain of the same synthetic workload."""
    import numpy as np
    d = max(range(g["n_domain"]), key=lambda k: g["data"]["train"][k]["uid"].shape[0])
    cols = g["data"]["train"][d]
    n = cols["uid"].shape[0]
    perm = np.asarray(shuffle_perm(n, TRAIN["shuffle_buffer_size"], 1))
    return d, cols, n, perm


def _time_steps(step_fn, cols, n, perm, batch, budget_s):
    steps, t0 = 0, time.time()
    while time.time() - t0 < budget_s:
        for s in range(-(-n // batch)):
            idx = perm[s * batch:(s + 1) * batch]
            step_fn(cols["uid"][idx], cols["pid"][idx], cols["domain"][idx], cols["label"][idx])
            steps += 1
            if time.time() - t0 >= budget_s:
                break
    return steps, time.time() - t0


def _pin_to_one_socket():
    """pin every thread of this process to one hardware thread per physical core of ONE socket (the socket of the first
    allowed cpu).  -> (cpus pinned to, restore()).  Falls back to no pinning when the topology cannot be read."""
    def no():
        pass
    try:
        allowed = sorted(os.sched_getaffinity(0))
        base = "/sys/devices/system/cpu/cpu%d/topology/"

        def rd(c, f):
            with open(base % c + f) as fh:
                return fh.read().strip()
        pkg0 = rd(allowed[0], "physical_package_id")
        seen, cpus = set(), []
        for c in allowed:
            if rd(c, "physical_package_id") != pkg0:
                continue
            core = rd(c, "core_id")
            if core not in seen:                 # first hardware thread of each physical core
                seen.add(core)
                cpus.append(c)
        if len(cpus) < 2:
            return [], no
        tids = [int(t) for t in os.listdir("/proc/self/task")]
        old = {}
        for t in tids:
            try:
                old[t] = os.sched_getaffinity(t)
                os.sched_setaffinity(t, cpus)
            except OSError:
                pass

        def restore():
            for t in os.listdir("/proc/self/task"):      # threads created meanwhile inherited the narrow mask
                try:
                    os.sched_setaffinity(int(t), old.get(int(t), allowed))
                except OSError:
                    pass
        return cpus, restore
    except Exception:
        return [], no


def cpu_baseline(g, batch, budget_s=15.0, params=None, emb_trainable=False, tower="mlp"):
    """The reference's CPU path (TF1.12, not installable here) is represented by restatements of the same step
    (oracle/, test infrastructure), timed on this box's host cores on a bounded sample of the same workload:
      * "value": torch-CPU fp32, autograd + dense TF1 Adam, at the fastest thread count of a sweep --
        the reported baseline;
      * "numpy_oracle": the numpy fp32 parity oracle on the same steps (a checker, not tuned for speed)."""
    import numpy as np
    import torch
    from oracle import rng as orng
    from oracle import torch_ref as tref
    from oracle import tower as otower
    if params is None:
        params = init_params(g)
        params["user_emb"], params["item_emb"] = g["tables"]["user_emb"], g["tables"]["item_emb"]
    d, cols, n, perm = _cpu_sample(g, batch, orng.shuffle_perm)
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    if tower == "star":
        from oracle import star as ostar
        names = sum(ostar.param_names(emb_trainable), ())
    else:
        names = otower.param_names(emb_trainable, {"deepfm": 1, "wdl": 2}.get(tower, 0), False)
    model = tref.TorchCpuModel({k: v for k, v in params.items()}, names, tower=tower, dropout=TRAIN["dropout"],
                               lr=TRAIN["learning_rate"])

    def one(s):
        idx = perm[(s % (n // batch or 1)) * batch:(s % (n // batch or 1) + 1) * batch]
        t = time.time()
        model.train_on_batch(cols["uid"][idx], cols["pid"][idx], cols["domain"][idx], cols["label"][idx])
        return time.time() - t
    # The thread count is the baseline's own tuning knob: at these sizes (0.4 - 3.4 GFLOP per step) all hardware
    # threads of a big host are far slower than a fraction of them (fork / join per small op; with every SMT
    # sibling busy a step took SECONDS on the 256-thread GPU host).  Every thread of this process is pinned to the
    # PHYSICAL cores of ONE socket for this leg (one hardware thread per core: no SMT siblings, no cross-socket
    # traffic; restored afterwards); doubling sweep from 8 threads up to that core count, each trial 1 warm + 5
    # timed steps (median), stopped once a trial is clearly slower than the best so far; the timed sample then runs
    # at the best count in THREE repeats: value = the median repeat, spread = [min, max].
    pinned, restore = _pin_to_one_socket()
    quota = _cpu_quota()
    try:
        cap = len(pinned) if pinned else (cores // 2 if cores >= 16 else cores)
        # (round 5: the container's cgroup may grant fewer CPUs of TIME than it shows cores -- the GPU box: 256 hardware
        # threads, cpu.max = 16 CPUs.  More runnable threads than that are throttled for whole 100 ms periods: that is the
        # "cliff" rounds 3 - 4 measured -- single steps of 84 - 1,597 ms at 62 - 64 threads -- not OpenMP's spinning.  The
        # sweep stops at the quota: what lies beyond measures the throttle, not the CPU path.)
        if quota is not None:
            cap = max(1, min(cap, int(quota)))
        # counts tried: 8, 16, 32, ..., 3/4 of the cap, the cap.  Each trial = 1 warm + 9 timed steps, scored by the mean
        # WITHOUT its two slowest steps: on this shared host single steps stall at any count (tests/diag_cpu_cliff.py,
        # profiles/r04_cpu_cliff.jsonl: outliers of 8 - 1,600 ms; near the pinned core count OpenMP's spinning workers lose
        # a core to any other runnable thread and the whole team waits at the next barrier -- 64 threads on 64 cores took
        # 0.9 - 1.8 s per step in BENCH_r03 and in round 4's runs; OMP_WAIT_POLICY=passive removes that and costs 2 - 3 x
        # everywhere).  The baseline runs at the SMALLEST count within 10 % of the best score: fewer threads = less
        # exposure to the neighbours, and the counts near the optimum differ by less than the run-to-run spread.
        counts, nt = [], min(8, cap)
        while nt < cap:
            counts.append(nt)
            nt *= 2
        if cap >= 16 and (3 * cap) // 4 not in counts:
            counts.append((3 * cap) // 4)
        counts = sorted(set(counts + [cap]))
        trials, unstable = [], []
        for nt in counts:
            torch.set_num_threads(nt)
            warm = one(0)
            # (9 timed steps per count; 5 where a step takes longer than 0.1 s -- the table-sized Adam of the Amazon workloads)
            ts = sorted(one(k) for k in range(1, 10 if warm < 0.1 else 6))
            score = float(np.mean(ts[:-2]))
            trials.append((nt, score))
            if ts[-1] > 2.5 * float(np.median(ts)):
                unstable.append((nt, ts[-1]))
            if score > 2.0 * min(t for _, t in trials) and nt >= 32:     # clearly past the optimum
                break
        best_t = min(t for _, t in trials)
        best_nt = min(n for n, t in trials if t <= 1.10 * best_t)
        torch.set_num_threads(best_nt)
        reps = []
        for _ in range(3):
            steps_r, dt_r = _time_steps(model.train_on_batch, cols, n, perm, batch, budget_s * 0.2)
            reps.append((steps_r / dt_r, steps_r, dt_r))
    finally:
        restore()
    reps.sort()
    value, steps, dt = reps[1]
    out = {"value": value, "unit": "domain-steps/s", "cores": int(best_nt), "kind": "port",
           "host_cores_visible": int(cores), "cpu_quota_cpus": quota, "pinned_to": "%d physical cores of one socket" % len(pinned) if pinned else "not pinned",
           "repeats": [round(r[0], 2) for r in reps], "spread": [round(reps[0][0], 2), round(reps[-1][0], 2)],
           # scoring rule of this record (ratios across rounds are comparable only under the same rule).
           # v1 (r01-r02) unpinned, fastest of a doubling sweep; v2 (r03) pinned to one socket, new sample + initialiser;
           # v3 (r04-) trimmed-mean trials (a trial's two slowest steps dropped), smallest thread count within 10 % of the best
           # v4 (r05): as v3, the sweep capped at the container's CPU quota (cpu_quota_cpus)
           "method": "v4: pinned to one socket, trimmed-mean thread sweep up to the cgroup CPU quota, smallest count within 10 % of the best, median of 3",
           "thread_sweep_ms_per_step": {str(k): round(v * 1e3, 2) for k, v in trials},
           "thread_sweep_unstable": {str(k): round(v * 1e3, 1) for k, v in unstable},     # count -> slowest step of its trial, ms
           "sample": "median of 3 repeats of ~%d inner steps each (bs=%d, domain %d of the same synthetic workload, %.1f s per "
                     "repeat): torch-CPU fp32 restatement of the TF1.12 step (gather, tower forward, Keras BCE, autograd "
                     "backward, dense TF1 Adam, dropout masks from a pre-drawn pool; oracle/torch_ref.py) on %d threads "
                     "(the fastest of a doubling sweep), pinned to one socket's physical cores (%d of the %d visible "
                     "hardware threads); a restatement, not TF" % (steps, batch, d, dt, best_nt, len(pinned) or cores, cores)}
    del model
    # second leg: the numpy parity oracle
    if tower == "star":
        from oracle import star as ostar
        omodel = ostar.OracleStar(params, emb_trainable=emb_trainable, lr=TRAIN["learning_rate"])
    else:
        omodel = otower.OracleModel(params, emb_trainable=emb_trainable, dropout=TRAIN["dropout"],
                                    lr=TRAIN["learning_rate"], tower=tower)
    osteps, odt = _time_steps(omodel.train_on_batch, cols, n, perm, batch, budget_s * 0.25)
    out["numpy_oracle"] = {"value": osteps / odt, "unit": "domain-steps/s",
                           "sample": "%d steps of the numpy fp32 oracle in %.1f s" % (osteps, odt)}
    return out


# ---------------------------------------------------------------------------------------------- committed profiles
def _cpu_quota():
    """CPUs of time the container's cgroup grants (cgroup v2 cpu.max / v1 cfs quota); None = unlimited."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
        if q != "max":
            return max(1.0, float(q) / float(per))
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = float(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = float(f.read())
        if q > 0:
            return max(1.0, q / per)
    except Exception:
        pass
    return None


def pmc_traffic(kernel_key):
    """HBM bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
    (tools/rocpd_summary.py pmc, gfx950 corrections applied); None if no summary is committed."""
    path = os.path.join(ROOT, "profiles", "pmc_hbm_latest.json")
    try:
        with open(path) as f:
            return json.load(f)[kernel_key]["hbm_bytes_per_launch"]
    except Exception:
        return None


def pmc_sq(kernel_key):
    """SQ / TCP counters per launch of `kernel_key` from the committed rocprofv3 --pmc passes (tools/r06_measure.sh stage `sq`,
    profiles/pmc_sq_latest.json), turned into the two figures DESIGN.md section 5 argues with: the share of the kernel's
    cycles its MFMA pipes were busy, and the bytes its workgroups pulled from L2 into their L1s (TCP_TCC_READ_REQ x 128 B).
    None if no summary is committed."""
    path = os.path.join(ROOT, "profiles", "pmc_sq_latest.json")
    try:
        with open(path) as f:
            c = json.load(f)[kernel_key]
    except Exception:
        return None
    out = {"source": "profiles/pmc_sq_latest.json (separate rocprofv3 --pmc passes, counters per launch)"}
    if c.get("SQ_VALU_MFMA_BUSY_CYCLES") and c.get("SQ_BUSY_CYCLES"):
        # SQ_BUSY_CYCLES sums the shader engines' busy clocks (32 on this part); MFMA-busy sums over the 1,024 SIMDs
        kernel_cycles = c["SQ_BUSY_CYCLES"] / 32.0
        out.update({"mfma_busy_cycles_per_simd": c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0, "kernel_cycles": kernel_cycles,
                    "mfma_busy_frac": c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0 / max(kernel_cycles, 1.0)})
    if c.get("TCP_TCC_READ_REQ"):
        out.update({"tcp_tcc_read_req": c["TCP_TCC_READ_REQ"], "l2_to_l1_bytes": c["TCP_TCC_READ_REQ"] * 128.0,
                    "l1_fill_cycles_per_cu_at_64B_clk": c["TCP_TCC_READ_REQ"] * 128.0 / 256.0 / 64.0})
    if c.get("SQ_WAIT_INST_ANY") and c.get("SQ_WAVE_CYCLES"):
        out["wave_cycles_in_waitcnt_frac"] = c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"]
    return out


def stamped_gather(shape):
    """the gather PHASE of a tower kernel as s_memtime stamps of a -DMAMDR_STAMPS build measured it (tools/r06_gather_in_step.py,
    profiles/gather_in_step_latest.json): cycles from kernel start to `rows in LDS`, median over the workgroups."""
    try:
        with open(os.path.join(ROOT, "profiles", "gather_in_step_latest.json")) as f:
            return json.load(f)[shape]
    except Exception:
        return None


def rocprof_avg_us(kernel, shape):
    """average duration of `kernel` in the newest committed rocprofv3 summary of this workload
    (profiles/r*_kernel_stats_<shape>.csv), for comparison with the HIP-event average measured live;
    None if no summary is committed."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_kernel_stats_%s.csv" % shape)))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            for row in csv.DictReader(f):
                if kernel in row["Name"]:
                    return float(row["AverageNs"]) / 1e3
    except Exception:
        pass
    return None


def finish_roofline(kernel, total_ms, launches, rows, flops_per_row=TOWER_TRAIN_FLOPS_PER_ROW):
    """achieved = algorithmic flops of all profiled launches / their summed device time
    (= flops per average launch / average launch duration)."""
    flops = rows * flops_per_row
    ach = flops / (total_ms * 1e-3) / 1e12
    return {"kernel": kernel, "bound": "mfma", "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": ach / PEAK_F32_MFMA_TFLOPS, "traffic": pmc_traffic(kernel),
            "traffic_unit": "HBM bytes per launch (profiles/pmc_hbm_latest.json: separate rocprofv3 --pmc passes)",
            "launches": launches,
            "avg_us": total_ms / max(launches, 1) * 1e3, "rows_per_launch": rows / max(launches, 1),
            "flops_per_row": flops_per_row}


# ---------------------------------------------------------------------------------------------- gather evidence
def gather_hbm_record(device, n_rows=1 << 19, reps=12):
    """the embedding gather (k_gather = the tile code the step kernels use) on Amazon-6-sized tables: 445,789 +
    172,653 rows x 128 fp32 = 316 MB, beyond the 256 MiB infinity cache, uniformly random rows, 2^19 positions
    per launch (0.81 GB of output).  HIP-event timed on the launch stream; `traffic` = HBM bytes per launch from
    the committed PMC passes of tools/gather_hbm.py (same sizes)."""
    import numpy as np
    import torch
    from mamdr_amd import _lib as L
    from mamdr_amd import engine, synthetic
    spec = synthetic.SHAPES["amazon6"]
    n_user, n_item, D = spec["n_user"], spec["n_item"], spec["n_domain"]
    eng = engine.TowerEngine(n_user, n_item, D, 1024, dropout=0.0)
    gen = torch.Generator(device=device)
    gen.manual_seed(5)
    for name, n in (("user_emb", n_user), ("item_emb", n_item)):
        t = torch.randn((n, 128), generator=gen, device=device, dtype=torch.float32) * 0.1
        eng.tables[name] = t
        seg = {"user_emb": L.SEG_USER_EMB, "item_emb": L.SEG_ITEM_EMB}[name]
        L.check(eng.lib.mamdr_bind_table(eng.ctx, seg, engine._ptr(t), n))
    rs = np.random.RandomState(9)
    eng.bind_domain_data(0, "train", rs.randint(0, n_user, n_rows), rs.randint(0, n_item, n_rows),
                         rs.randint(0, D, n_rows), rs.randint(0, 2, n_rows).astype(np.float32))
    out = torch.empty((n_rows, 384), dtype=torch.float32, device=device)
    for _ in range(3):
        eng.gather(0, "train", out=out)
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        eng.gather(0, "train", out=out)
    ms, cnt = eng.profile_read(L.KERNEL_GATHER)
    eng.profile(False)
    eng.close()
    nbytes = n_rows * GATHER_BYTES_PER_ROW
    ach = nbytes / (ms / cnt * 1e-3) / 1e9
    return {"kernel": "k_gather", "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": ach / PEAK_HBM_GBS, "traffic": pmc_traffic("k_gather@amazon6"),
            "traffic_unit": "HBM bytes per launch (profiles/pmc_hbm_latest.json, tools/gather_hbm.py)",
            "avg_us": ms / cnt * 1e3, "launches": cnt, "rows_per_launch": n_rows, "bytes_per_row": GATHER_BYTES_PER_ROW,
            "algorithmic_bytes_per_launch": nbytes, "table_bytes": (n_user + n_item) * 512,
            "note": "Amazon-6-sized tables (316 MB, beyond the 256 MiB infinity cache), uniformly random rows; "
                    "3 x 512-B rows read + 384 floats written per position"}


# ---------------------------------------------------------------------------------------------- outputs of the timed path
DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, budget=DUMP_BYTES):
    """arrays: {name: device tensor [P] or list of device tensors [P] (one row each)} -> out_dir/<name>.npy, float32.  Each name
    gets an equal share of `budget`; where a name's rows hold more elements than its share, every row is cut to the same
    fixed, seeded sample of positions (sorted), the same in every run."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    cap = budget // 4 // max(len(arrays), 1)
    for k, (name, rows) in enumerate(sorted(arrays.items())):
        one = torch.is_tensor(rows)
        rows = [rows] if one else list(rows)
        n, per_row = rows[0].numel(), cap // max(len(rows), 1)
        idx = None
        if n > per_row:
            idx = np.unique(np.random.RandomState(1000 + k).randint(0, n, size=per_row))
            idx = torch.from_numpy(idx).to(rows[0].device)
        host = [(r.reshape(-1) if idx is None else r.reshape(-1).index_select(0, idx)).float().cpu().numpy() for r in rows]
        np.save(os.path.join(out_dir, name + ".npy"), host[0] if one else np.stack(host))


# ---------------------------------------------------------------------------------------------- one workload
def run_workload(wl_name, steps, warmup, rank, world, profile=True, cpu_budget=0.0, dump_dir=None):
    import numpy as np
    import torch
    import torch.distributed as dist
    from mamdr_amd import _lib as L
    from mamdr_amd import meta, parallel, plan as mplan, synthetic

    wl = WORKLOADS[wl_name]
    batch = int(os.environ.get("MAMDR_BENCH_BATCH", wl["batch"]))      # (exploration only: the named config fixes it)
    row_scale = float(os.environ.get("MAMDR_BENCH_ROW_SCALE", wl.get("row_scale", 1.0)))
    trainable = bool(wl.get("emb_trainable"))
    # (only the train split is bound here; val / test are not drawn: 17 M rows less to generate on Amazon-6)
    g = synthetic.generate(wl["shape"], batch_size=batch, seed=TRAIN["seed"], row_scale=row_scale, splits=("train",))
    D = g["n_domain"]
    tower = wl.get("tower", "mlp")

    def full_params(seed=1024):
        if tower == "star":      # Keras defaults of the Star layers (mamdr_amd/model_zoo/star.py)
            from mamdr_amd.model_zoo.star import initial_tensors
            return initial_tensors(np.random.RandomState(seed), g["n_user"], g["n_item"], D, 128, (256, 128, 64),
                                   None if trainable else g["tables"]["user_emb"],
                                   None if trainable else g["tables"]["item_emb"])
        p = init_params(g, seed)
        if trainable:      # Amazon: no pretraining, N(0, 1e-4^2) tables (deepctr.py:115 SparseFeat default)
            rs_ = np.random.RandomState(seed + 7)
            p["user_emb"] = (rs_.standard_normal((g["n_user"], 128)) * 1e-4).astype(np.float32)
            p["item_emb"] = (rs_.standard_normal((g["n_item"], 128)) * 1e-4).astype(np.float32)
        return p

    def new_run():
        """engine, model state and epoch() of one run of this workload, from its initial state: the same bits in every
        run, which the timed epochs start from (the prewarm below runs on a run of its own)."""
        eng = setup_engine(g, batch, trainable, tower)
        sizes = [eng.n_rows(d, "train") for d in range(D)]
        steps_per_domain = [-(-n // batch) for n in sizes]

        def initial_vector(seed=1024):
            """one random initialisation of the whole model as a flat device vector.  Frozen-table workloads: packed on
            the host (0.56 MB).  Trainable tables (79 - 92 M floats): the dense tensors come from the same host
            initialisers, the two big tables are drawn ON the device with their layer's distribution (deepctr
            SparseFeat N(0, 1e-4^2), Keras Embedding U(-0.05, 0.05) for the Star tower) -- D + 1 host draws of 92 M
            normals would cost the default run half a minute."""
            if not trainable:
                return eng.pack(full_params(seed))
            keep = (g["n_user"], g["n_item"])
            g["n_user"], g["n_item"] = 8, 8                      # host initialisers for everything but the two tables
            try:
                small = full_params(seed)
            finally:
                g["n_user"], g["n_item"] = keep
            v = torch.zeros(eng.n_params, dtype=torch.float32, device=eng.device)
            gen = torch.Generator(device=eng.device)
            gen.manual_seed(seed)
            for name, (off, cnt) in eng.segments.items():
                if name in ("user_emb", "item_emb"):
                    if tower == "star":
                        v[off:off + cnt].uniform_(-0.05, 0.05, generator=gen)
                    else:
                        v[off:off + cnt].normal_(0.0, 1e-4, generator=gen)
                elif name in ("lin_user", "lin_item"):
                    pass                                             # DeepFM linear tables start at zero
                else:
                    v[off:off + cnt] = torch.from_numpy(np.ascontiguousarray(small[name], np.float32).ravel()).to(eng.device)
            return v

        full0 = initial_vector()
        eng.set_weights(full0)                 # tensors outside theta (Star: PN, specific kernels, output unit)
        theta = full0[:eng.n_meta].clone()
        del full0
        wrapper = wl.get("wrapper", "mamdr")
        # phi_d starts as a second random init of the whole model (mamdr.py:31-33); every rank draws all of them
        balanced = None
        if wrapper == "mamdr":
            phis = {d: initial_vector(seed=2000 + d)[:eng.n_meta] for d in range(D)}
            balanced = parallel.BalancedMAMDR(eng, meta, theta, phis, steps_per_domain,
                                              dn_mode=os.environ.get("MAMDR_BENCH_DN_MODE", "sharded"))
            del phis
        delta, zero = eng.new_vector(meta=True), eng.new_vector(meta=True)
        planner = mplan.EpochPlanner(range(D), TRAIN["sample_num"], TRAIN["add_query_domain"], True, TRAIN["seed"])
        shuffles = mplan.EpochShuffles(mplan.PassShuffler(sizes, TRAIN["shuffle_buffer_size"], TRAIN["seed"] + rank),
                                       eng.device)
        loads = []
        host_prep_s = [0.0]
        next_plan = [None]
        prefetch = os.environ.get("MAMDR_BENCH_NO_PREFETCH", "0") in ("", "0")      # A/B switch

        def epoch():
            th0 = time.perf_counter()
            if wrapper == "dn":               # Domain Negotiation only (domain_negotiation.py:37-88)
                p = next_plan[0] if next_plan[0] is not None else planner.next_epoch(with_dr=False)
                owner = parallel.lpt_partition(steps_per_domain, world)
                local = [d for d in p["seq"] if owner[d] == rank]
                shuffles.prepare([(d, 0) for d in local])
                host_prep_s[0] += time.perf_counter() - th0
                tr = []
                parallel.dn_phase_sharded(eng, meta, theta, local, shuffles, batch, TRAIN["learning_rate"],
                                          TRAIN["meta_learning_rate"], tr, delta, zero)
                eng.set_weights(theta)
                if prefetch:
                    th1 = time.perf_counter()
                    next_plan[0] = planner.next_epoch(with_dr=False)
                    shuffles.prefetch([(d, 0) for d in next_plan[0]["seq"] if owner[d] == rank])
                    host_prep_s[0] += time.perf_counter() - th1
                return tr, mplan.plan_steps(p, steps_per_domain)
            p = next_plan[0] if next_plan[0] is not None else planner.next_epoch()    # same seed on every rank -> same global plan
            next_plan[0] = None
            host_prep_s[0] += time.perf_counter() - th0

            # the NEXT epoch's plan is a function of the seed alone: its shuffles are drawn on a worker thread while this epoch is
            # enqueued and run (plan.EpochShuffles.lookahead: a few passes in; the work stays inside the timed region, off the
            # critical path of the epoch boundary, whose run-ahead margin is 2 - 3 ms of queued launches)
            def look():
                th1 = time.perf_counter()
                next_plan[0] = planner.next_epoch()
                shuffles.prefetch(balanced.local_passes(next_plan[0]))
                host_prep_s[0] += time.perf_counter() - th1
            shuffles.lookahead = look if prefetch else None
            tr = balanced.epoch(p, shuffles.prepare, shuffles, batch, TRAIN["learning_rate"], TRAIN["meta_learning_rate"],
                                TRAIN["merged_method"])
            if balanced.last_load is not None:
                loads.append(balanced.last_load)
            return tr, mplan.plan_steps(p, steps_per_domain)

        return types.SimpleNamespace(eng=eng, epoch=epoch, theta=theta, balanced=balanced, shuffles=shuffles, loads=loads,
                                     host_prep_s=host_prep_s, sizes=sizes)

    def barrier():
        if world > 1:
            parallel.barrier()          # (ranks of a process group, or the lanes of this process)
        torch.cuda.synchronize()

    # device warm-up before the W warm-up epochs the contract asks for: the first process on a box that has just come up runs
    # its first second at lower clocks (measured: 43.3 K on such a run against 44.6 K on every later one, kernel times of the
    # later profile pass identical) -- W = 3 epochs are 85 ms.  Untimed, reported as `prewarm_s`.  How many epochs fit in that
    # time varies from run to run, so they run on a run of their own, closed afterwards: the W warm-up and the timed epochs
    # start from the initial state in every run (their results are comparable across runs and builds: --dump-outputs).
    prewarm_s = float(os.environ.get("MAMDR_BENCH_PREWARM_S", "0.75"))
    if prewarm_s > 0:
        pre = new_run()
        tw = time.perf_counter()
        while True:
            pre.epoch()
            torch.cuda.synchronize()
            go_on = torch.tensor([1.0 if time.perf_counter() - tw < prewarm_s else 0.0], device=pre.eng.device)
            if world > 1:
                parallel.all_reduce(go_on, "min")        # (ranks / lanes leave the loop together)
            if float(go_on.item()) == 0.0:
                break
        pre.shuffles.cancel()
        pre.eng.close()
        del pre
    run = new_run()
    eng, epoch, theta, balanced, shuffles = run.eng, run.epoch, run.theta, run.balanced, run.shuffles
    loads, host_prep_s, sizes = run.loads, run.host_prep_s, run.sizes
    for _ in range(warmup):
        epoch()
    barrier()
    del loads[:]
    host_prep0 = host_prep_s[0] + (balanced.host_prep_s if balanced is not None else 0.0)
    t0 = time.perf_counter()
    local_steps, global_steps, local_passes, host_s = 0, 0, 0, 0.0
    for _ in range(steps):
        th = time.perf_counter()
        tr, b = epoch()
        host_s += time.perf_counter() - th       # enqueue-only: plan, LPT, shuffles + upload, the launches (no sync)
        local_steps += sum(t[2] for t in tr)
        local_passes += len(tr)
        global_steps += b
    barrier()
    dt = time.perf_counter() - t0
    host_ms = [host_s / steps * 1e3]
    if world > 1:
        t = torch.tensor([dt, float(local_steps), float(local_passes), host_s], dtype=torch.float64, device=eng.device)
        tmax = t.clone()
        parallel.all_reduce(tmax, "max")
        parallel.all_reduce(t)
        dt = float(tmax[0])
        assert int(round(float(t[1]))) == global_steps, (float(t[1]), global_steps)
        local_passes = int(round(float(t[2])))
        host_ms = [float(t[3]) / world / steps * 1e3, float(tmax[3]) / steps * 1e3]      # mean, max over ranks
    if dump_dir is not None:
        # what the caller of the timed path holds after its last epoch, before anything else runs: theta, every phi_d
        # (gathered onto every rank first) and the live weights of the engine
        if balanced is not None:
            balanced.sync_phis()
        weights = eng.weights                   # (flushes the lazily updated table rows)
        torch.cuda.synchronize()
        if rank == 0:
            out = {"theta": theta, "weights": weights}
            if balanced is not None:
                out["phi"] = [balanced.phis[d] for d in sorted(balanced.phis)]
            dump_outputs(dump_dir, out)
        del weights

    # ---- per-kernel device time (HIP events on the launch stream) over one more epoch of
    #      the same workload; reported for the dominant kernel, k_tower<train>
    roofline, kernels, sweep_info, table_info, l2_gather, gather_in_step = None, {}, None, None, None, None
    if profile:
        eng.profile(True)
        eng.profile_reset()
        epoch()                       # fills the library's event pool: the measured epoch below creates no events
        eng.profile_reset()
        torch.cuda.synchronize()
        tp0 = time.perf_counter()
        prof_trace, _ = epoch()
        torch.cuda.synchronize()
        prof_wall_us = (time.perf_counter() - tp0) * 1e6
        names = {L.KERNEL_EMB_SWEEP: L.KERNEL_NAMES[L.KERNEL_EMB_SWEEP]}
        names.update(eng.step_kernel_names(batch))
        if trainable and os.environ.get("MAMDR_DENSE_ADAM", "0") in ("", "0"):
            names[L.KERNEL_EMB_SWEEP] = "k_emb_reduce"
        names[L.KERNEL_AUX] = {"star": "k_star_stats+prep | k_star_pnb_* (PartitionedNorm backward) | k_emb_rows | "
                                       "k_emb_catchup | k_star_catchup (timed groups)",
                               "deepfm": "k_emb_rows | k_emb_catchup | k_lin_sweep"}.get(tower, "k_pass_prep_multi (once per window of passes)")
        names[L.KERNEL_FLUSH] = "k_emb_flush"
        prof_steps = sum(n for (_, _, n) in prof_trace)
        accounted = 0.0
        for k in (L.KERNEL_FWD_BWD, L.KERNEL_WGRAD, L.KERNEL_UPDATE, L.KERNEL_EMB_SWEEP, L.KERNEL_AUX, L.KERNEL_FLUSH):
            ms, cnt = eng.profile_read(k)
            if cnt:
                kernels[names[k]] = {"launches": cnt, "avg_us": ms / max(cnt, 1) * 1e3,
                                     "us_per_domain_step": ms * 1e3 / max(prof_steps, 1)}
                accounted += ms * 1e3 / max(prof_steps, 1)
        # (the profiled epoch launches every kernel on its own -- the timed epochs fuse the tails of a step with
        # trainable tables -- so the slots add up to the profiled epoch's device time, not to us_per_domain_step)
        kernels["_sum_us_per_domain_step"] = accounted
        kernels["_profiled_epoch_wall_us_per_domain_step"] = prof_wall_us / max(prof_steps, 1)
        dense_adam = os.environ.get("MAMDR_DENSE_ADAM", "0") not in ("", "0")
        if trainable and not dense_adam:
            # default: lazy replay of TF1's dense table Adam (csrc/emb_kernels.hip) -- per step only the rows of
            # the batch move through HBM; MAMDR_DENSE_ADAM=1 measures the per-step sweep instead
            ms, cnt = eng.profile_read(L.KERNEL_EMB_SWEEP)
            table_info = {"mode": "lazy (bit-identical to the per-step dense sweep)",
                          "kernel": "k_emb_reduce (+ Adam step of the touched rows)",
                          "avg_us": ms / max(cnt, 1) * 1e3, "launches": cnt}
        if trainable and dense_adam:
            # HBM-bound dense optimiser pass: 24 B per table element (read p, m, v; write p, m, v) + 4 B
            # of row map per 512-B row, one launch per step over both tables
            ms, cnt = eng.profile_read(L.KERNEL_EMB_SWEEP)
            # (DeepFM's 1-d linear tables ride in the same launches: 24 more bytes per row, < 1 %, not counted)
            sweep_bytes = (g["n_user"] + g["n_item"]) * (128 * 24 + 4) * cnt
            ach = sweep_bytes / (ms * 1e-3) / 1e9
            sweep_info = {"kernel": "k_emb_sweep", "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS,
                          "unit": "GB/s", "frac": ach / PEAK_HBM_GBS, "traffic": pmc_traffic("k_emb_sweep<0>"),
                          "avg_us": ms / max(cnt, 1) * 1e3, "launches": cnt,
                          "bytes_per_step": (g["n_user"] + g["n_item"]) * (128 * 24 + 4)}
        roofline_ms, cnt = eng.profile_read(L.KERNEL_FWD_BWD)
        eng.profile(False)
        eng.profile_reset()
        # every launch is one batch; a pass of n_steps launches covers min(rows of the domain, n_steps*batch) rows
        prof_rows = sum(min(sizes[d], n * batch) for (_, d, n) in prof_trace)
        assert cnt == sum(n for (_, _, n) in prof_trace)
        # the 4-row-tile kernel (mamdr_api.hip: use4 / tower4_max_rows): up to one round of workgroups (4 rows x CUs) for
        # the frozen-table mlp tower, up to 2,048 rows with trainable tables / DeepFM; template <DX, FM, W1L, PRE>
        n_cu = torch.cuda.get_device_properties(eng.device).multi_processor_count
        t4_max = min(2048, max(256, 4 * n_cu)) if (tower == "mlp" and not trainable) else 2048
        use4 = batch <= t4_max and tower != "star" and os.environ.get("MAMDR_TOWER_TILE", "") != "16"
        fm = ", true>" if tower == "deepfm" else ", false>"
        if use4:
            # template <DX, FM, W1L>; W1L (the W1 image in LDS) at one 4-row tile per CU or less (tower4_kernels.hip)
            tiles4 = -(-batch // 16) * 4
            w1l = tiles4 <= torch.cuda.get_device_properties(eng.device).multi_processor_count
            # ... PRE (the instance for pre-gathered passes) on the k_wgrad_adam path
            pre4 = not trainable and tower == "mlp" and os.environ.get("MAMDR_NO_PREGATHER", "0") in ("", "0") and \
                eng.step_kernel_names(batch)[L.KERNEL_WGRAD] == "k_wgrad_adam"
            # (5th parameter W2D: the call's FIRST tower reads W2 in place -- 1 launch in 9; the steady-state instance is named)
            kname = ("k_tower4<true" if trainable else "k_tower4<false") + fm[:-1] + (", true" if w1l else ", false") + \
                (", true" if pre4 else ", false") + ", false>"
        else:
            # template <TRAIN, DXW, FM, FZ>; FZ (k_wgrad_adam's duties compiled in) only on that path
            fz = ", true>" if (not trainable and tower == "mlp" and eng.step_kernel_names(batch)[L.KERNEL_WGRAD] == "k_wgrad_adam") \
                else ", false>"
            kname = ("k_tower<true, 256" if trainable else "k_tower<true, 0") + fm[:-1] + fz
        if tower == "star":
            kname = "k_tower<true, 384, false, false>"
        roofline = finish_roofline(kname, roofline_ms, cnt, prof_rows,
                                   tower_flops_per_row(384 if tower == "star" else (256 if trainable else 0)))
        roofline["rocprofv3_avg_us"] = rocprof_avg_us(kname, wl["shape"])
        if kname == "k_tower4<false, false, true, true, false>":
            # what this three-phase, 4-row-tile design can reach: the kernel's measured time minus
            # what the diagnostic builds of round 2 showed each single remedy can return at most (DESIGN.md section 6:
            # no W1 traffic at all 0.6 us, no split-k exchange through LDS 0.3 us, no cold paths 0.2 us)
            # (this is NOT an independent floor -- it moves with avg_us by construction -- hence its name; the
            # two hardware-derived figures beside it are: 4 rows x 360,576 flop on one CU's fp32 MFMA rate, and the 0.59 MB
            # weight stream of one workgroup at the L1 fill peak of 64 B / clk)
            roofline["avg_us_minus_ablation_bounds"] = max(roofline["avg_us"] - (0.6 + 0.3 + 0.2), 0.0)
            roofline["hardware_floors_us"] = {"mfma_4_row_tile_per_cu": 2.35, "weight_stream_at_l1_fill_peak": 3.8}
            roofline["floor_note"] = ("avg_us_minus_ablation_bounds = avg_us minus the sum of the measured ablation bounds (no W1 "
                                      "stream 0.6, no split-k exchange 0.3, no cold paths 0.2 us: diagnostic builds, DESIGN.md "
                                      "section 5) -- what this three-phase four-row-tile design can reach, not a floor of the problem")
        # ---- the other kernels of a step against the roof that bounds each of them
        props = torch.cuda.get_device_properties(eng.device)
        # parameters one k_update launch steps: the dense block (the tables and DeepFM's 1-d linear tables have kernels of
        # their own); of the Star tower's per-domain tensors only the batch's slice (the others are replayed lazily)
        per_domain = ("Wd0", "Wd1", "Wd2", "bd0", "bd1", "bd2", "pn_gamma_spec", "pn_beta_spec")
        p_dense = sum((c // D if n in per_domain else c) for n, (_, c) in eng.segments.items()
                      if n not in ("user_emb", "item_emb", "lin_user", "lin_item"))
        rows_avg = prof_rows / max(cnt, 1)
        rated = []
        for key, kn in names.items():
            if kn not in kernels or key == L.KERNEL_FWD_BWD:
                continue
            k_us, k_n = kernels[kn]["avg_us"], kernels[kn]["launches"]
            if key == L.KERNEL_WGRAD:
                # weight gradients: 2 x rows x 139,777 flop per launch; with k_wgrad_adam the optimiser step of
                # the dense block rides in the same launch
                ach = 2.0 * rows_avg * 139777 / (k_us * 1e-6) / 1e12
                ent = {"kernel": kn, "bound": "mfma", "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                       "frac": ach / PEAK_F32_MFMA_TFLOPS, "avg_us": k_us, "launches": k_n}
                if not kn.startswith("k_wgrad_adam"):
                    # the split-K form is as much a memory kernel: it reads the tower's activations /
                    # gradients [rows][832 + 448] once and writes one partial slab of the dense block per row group
                    # (mamdr_api.hip: 256-row groups up to 4,096 rows, 512 beyond, at most 16) -- rated against HBM too, on
                    # these algorithmic bytes and on the PMC counter bytes of the committed passes
                    rpg = 256 if batch <= 4096 else 512
                    groups = min(16, -(-batch // rpg))
                    alg = rows_avg * (832 + 448) * 4.0 + groups * p_dense * 4.0
                    ent.update({"hbm_bytes_algorithmic": alg, "hbm_frac_algorithmic": alg / (k_us * 1e-6) / 1e9 / PEAK_HBM_GBS,
                                "row_groups": groups})
                    # (with trainable tables the launch is k_wgrad_reduce: the table reduce's workgroups ride in it and
                    # its counter bytes are theirs too)
                    tr = pmc_traffic(kn + "@" + wl["shape"]) or pmc_traffic(kn + "_reduce@" + wl["shape"]) or pmc_traffic(kn)
                    if tr:
                        ent.update({"hbm_bytes_pmc": tr, "hbm_frac": tr / (k_us * 1e-6) / 1e9 / PEAK_HBM_GBS,
                                    "hbm_note": "counter bytes per launch (profiles/pmc_hbm_latest.json) / this run's avg_us / 8 TB/s"})
                rated.append(ent)
            elif key == L.KERNEL_UPDATE and kn.startswith("k_update"):
                # dense optimiser step: 28 B per parameter (read p, m, v, g; write p, m, v); the gradient arrives as G
                # slabs (4 G P more bytes read: not algorithmic)
                ach = 28.0 * p_dense / (k_us * 1e-6) / 1e9
                rated.append({"kernel": kn, "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": ach / PEAK_HBM_GBS, "avg_us": k_us, "launches": k_n, "bytes_per_launch": 28.0 * p_dense})
            elif key == L.KERNEL_FLUSH:
                # lazy table Adam's replay: every missed step of every element exactly once -> (steps between two
                # flushes) x table elements per launch (rows a batch touched in between replay fewer: < 10 % of the
                # rows), against the issue bound of its two quarter-rate instructions per element-step (v_sqrt_f32 +
                # v_rcp_f32: 16 cycles each per 64-lane wave on a SIMD)
                el_steps = (g["n_user"] + g["n_item"]) * 128.0 * (prof_steps / max(k_n, 1))
                peak = props.multi_processor_count * 4 * getattr(props, "clock_rate", 2400000) * 1e3 * 64.0 / 32.0 / 1e12
                ach = el_steps / (k_us * 1e-6) / 1e12
                rated.append({"kernel": kn, "bound": "alu (quarter-rate v_sqrt_f32 + v_rcp_f32)", "achieved": ach, "peak": peak,
                              "unit": "T element-steps/s", "frac": ach / peak, "avg_us": k_us, "launches": k_n,
                              "element_steps_per_launch": el_steps})
        # ---- the gather WHERE IT RUNS.  k_wgrad_adam path: k_pass_prep_multi resolves and gathers a window
        # of <= 16 passes per launch -- per row it reads the permutation entry, uid / pid / domain / label (20 B), the two
        # 512-B table rows, and writes them with the domain and label (1,032 B): 2,076 algorithmic bytes -- timed live by the
        # HIP events above.  Everywhere else the gather is the first phase of the tower kernel: its duration comes from the
        # stamps of a diagnostic build (profiles/gather_in_step_latest.json), the rows per launch from this run.
        gather_in_step = None
        aux_name = names.get(L.KERNEL_AUX, "")
        if aux_name.startswith("k_pass_prep_multi") and aux_name in kernels:
            k_us, k_n = kernels[aux_name]["avg_us"], kernels[aux_name]["launches"]
            by = prof_rows / max(k_n, 1) * 2076.0
            ach = by / (k_us * 1e-6) / 1e9
            gather_in_step = {"kernel": "k_pass_prep_multi", "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": ach / PEAK_HBM_GBS, "avg_us": k_us, "launches": k_n, "rows_per_launch": prof_rows / max(k_n, 1),
                              "bytes_per_row": 2076, "traffic": pmc_traffic("k_pass_prep_multi"),
                              "served_from": "tables of %.1f MB: L2 / infinity cache reads, HBM writes" % ((g["n_user"] + g["n_item"]) * 512 / 1e6),
                              "share_of_step_us": kernels[aux_name]["us_per_domain_step"]}
            rated.append(dict(gather_in_step))
        else:
            st = stamped_gather(wl["shape"])
            if st and st.get("kernel") == roofline["kernel"]:
                secs = st["gather_phase_cycles"] / (st["clock_ghz"] * 1e9)
                by = rows_avg * GATHER_BYTES_PER_ROW
                ach = by / secs / 1e9
                gather_in_step = {"kernel": roofline["kernel"] + " (gather phase)", "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS,
                                  "unit": "GB/s", "frac": ach / PEAK_HBM_GBS, "phase_us": secs * 1e6, "phase_cycles": st["gather_phase_cycles"],
                                  "rows_per_launch": rows_avg, "bytes_per_row": GATHER_BYTES_PER_ROW,
                                  "share_of_kernel": secs * 1e6 / max(roofline["avg_us"], 1e-9),
                                  "source": "profiles/gather_in_step_latest.json (s_memtime stamps of a -DMAMDR_STAMPS build, median "
                                            "over the workgroups: %s)" % st.get("note", ""),
                                  "table_bytes": (g["n_user"] + g["n_item"]) * 512}
        # counter-backed reading of the two headline kernels: MFMA-busy share and L2 -> L1 traffic
        sq = pmc_sq(roofline["kernel"] + "@" + wl["shape"]) or pmc_sq(roofline["kernel"])
        if sq:
            roofline["counters"] = sq
        for ent in rated:
            sq = pmc_sq(ent["kernel"] + "@" + wl["shape"]) or pmc_sq(ent["kernel"])
            if sq:
                ent["counters"] = sq
        kernels["_rated"] = rated
        if not trainable:
            # the workload's own gather: pass-sized, the frozen Taobao tables live in L2 / infinity cache
            dbig = max(range(D), key=lambda k: sizes[k])
            perm = torch.from_numpy(shuffles.sh(dbig)).to(eng.device)
            out = torch.empty((sizes[dbig], 384), dtype=torch.float32, device=eng.device)
            for _ in range(3):
                eng.gather(dbig, "train", perm=perm, out=out)
            eng.profile(True)
            eng.profile_reset()
            for _ in range(20):
                eng.gather(dbig, "train", perm=perm, out=out)
            gms, gcnt = eng.profile_read(L.KERNEL_GATHER)
            eng.profile(False)
            eng.profile_reset()
            gach = sizes[dbig] * GATHER_BYTES_PER_ROW / (gms / gcnt * 1e-3) / 1e9
            l2_gather = {"kernel": "k_gather", "served_from": "L2 / infinity cache (tables of %.1f MB)" %
                         ((g["n_user"] + g["n_item"]) * 512 / 1e6), "achieved": gach, "unit": "GB/s",
                         "rows_per_launch": sizes[dbig], "bytes_per_row": GATHER_BYTES_PER_ROW,
                         "note": "cache-resident tables: NOT an HBM figure (the HBM-bound gather is `gather`)"}
    cpu = None
    if rank == 0 and world == 1 and cpu_budget > 0:
        cpu = cpu_baseline(g, batch, cpu_budget, full_params() if trainable else None, trainable, tower)
    rec = {
        "value": global_steps / dt, "unit": "domain-steps/s", "ms_per_step": dt / steps * 1e3,
        "workload": wl["name"].format(rows="%g %%" % (row_scale * 100)), "global_batch": batch, "domains": D,
        "domain_steps_per_epoch": global_steps / steps, "epochs_timed": steps,
        "us_per_domain_step": dt / global_steps * 1e6 * world,
        "domain_passes_per_sec": local_passes / dt,
        "roofline": sweep_info if (sweep_info and sweep_info["avg_us"] * 2 > (roofline or {}).get("avg_us", 0)) else roofline,
        "tower": roofline, "table_update": table_info or sweep_info, "gather_l2": l2_gather,
        "kernels_avg_us": kernels, "cpu_baseline": cpu, "gather_in_step": gather_in_step if profile else None,
        # host side of an epoch.  host_ms_per_epoch = wall time spent inside the epoch call before any synchronisation
        # (plan + LPT + shuffle generation / upload + every launch; [mean, max] over ranks when world > 1): an UPPER
        # bound -- the HIP queue blocks the host once it is a few hundred launches ahead, so at N = 1 this tracks the
        # device time.  host_prep_ms_per_epoch = the part that does not shrink with the rank count (drawing the epoch's
        # plan, the per-epoch assignment, drawing + uploading this rank's shuffles), timed on its own.
        "host_ms_per_epoch": host_ms, "prewarm_s": prewarm_s, "prewarm_note": "untimed epochs before the W warm-up epochs (device clocks)",
        "host_prep_ms_per_epoch": (host_prep_s[0] + (balanced.host_prep_s if balanced is not None else 0.0) - host_prep0) / steps * 1e3,
    }
    if balanced is not None and balanced.wire_bytes:
        # payload this rank put on the wire per epoch: the DN all-reduce (+ Star tail) and the phi slots it sent
        wb = balanced.wire_bytes[-steps:]
        rec["wire_bytes_per_epoch_rank0"] = float(np.mean(wb))
        rec["dn_mode"] = balanced.dn_mode
    if loads:
        # what the per-epoch partition allows: sum of the ranks' planned steps / the largest rank's
        rec["partition_speedup_bound"] = float(np.mean([sum(l) / max(l) for l in loads]))
    if cpu:
        rec["gpu_over_cpu"] = rec["value"] / cpu["value"]
    if os.environ.get("MAMDR_BENCH_PREP_TIMING"):
        print("prep timing (ms summed over %d epochs): %s" % (steps + warmup, {k: round(v * 1e3, 2) for k, v in shuffles.timing.items()}), file=sys.stderr)
    shuffles.cancel()           # the prefetch of an epoch that will not run
    eng.close()
    return rec


def run_lanes(wl_name, steps, warmup, lanes, outer=(0, 1)):
    """the same epochs by `lanes` LANES of this process (mamdr_amd/parallel.LaneGroup): the sharded epoch of SURVEY 8e -- per-epoch
    LPT of the DR query domains and DN passes, one sum of the DN displacements -- with the ranks as host threads, one engine
    and one HIP stream each, on ONE GPU.  Same timed region as the ranks' (barrier + device synchronise on both sides,
    max over lanes).  NOT the reference's single sequential chain (its Adam slots and shuffle streams are per lane, its
    DN update sums per-lane displacements): reported beside `value`, never as `value`."""
    from mamdr_amd import parallel
    # (outer = (rank, world) of a multi-process run: RANKS x LANES, one world of world * lanes participants -- parallel.py)
    recs = parallel.LaneGroup(lanes, outer=outer).run(
        lambda lane: run_workload(wl_name, steps, warmup, outer[0] * lanes + lane, outer[1] * lanes, False, 0.0))
    r = recs[0]
    out = {k: r[k] for k in ("value", "unit", "ms_per_step", "us_per_domain_step", "workload", "domain_steps_per_epoch",
                             "partition_speedup_bound", "host_ms_per_epoch", "dn_mode") if k in r}
    out.update({"lanes": lanes, "participants": outer[1] * lanes,
                "semantics": "the %d-participant sharded epoch (SURVEY 8e), %d lane(s) per GPU: lanes = host threads, one engine + "
                             "one HIP stream each; not the single chain `value` times" % (outer[1] * lanes, lanes),
                "us_per_domain_step": r["ms_per_step"] * 1e3 / r["domain_steps_per_epoch"],
                # (every lane's stream on a hardware queue of its own needs this set BEFORE the HIP runtime initialised: ADVICE r05)
                "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")})
    return out


# ---------------------------------------------------------------------------------------------- launcher
def spawn_ranks(args):
    """`python bench.py --gpus N` without a rendezvous: start N ranks through torch.distributed.run as a CHILD
    process (this process has not touched the GPU and never will), relay its JSON line and exit code."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    sys.stdout.flush()
    return proc.returncode if (proc.returncode != 0 or line is not None) else 1


def summary_block(result, targets, lanes_rec):
    """compact per-workload digest: value, us per domain-step, the dominant kernel with its roofline fraction (and, where the
    counters are committed, its MFMA-busy share), the in-step gather, the CPU baseline of the same run, lanes."""
    def brief(rec, lanes=None):
        if "error" in rec:
            return {"error": rec["error"][:120]}
        roof = rec.get("roofline") or {}
        out = {"value": round(rec["value"], 1), "us_per_step": round(rec["us_per_domain_step"], 2),
               "kernel": roof.get("kernel"), "bound": roof.get("bound"), "frac": round(roof.get("frac", 0.0), 4),
               "kernel_us": round(roof.get("avg_us", 0.0), 2)}
        if (roof.get("counters") or {}).get("mfma_busy_frac") is not None:
            out["mfma_busy"] = round(roof["counters"]["mfma_busy_frac"], 3)
        gi = rec.get("gather_in_step")
        if gi:
            out["gather_in_step"] = {"kernel": gi["kernel"].split("<")[0], "GBps": round(gi["achieved"], 1), "frac": round(gi["frac"], 3)}
        cpu = rec.get("cpu_baseline")
        if cpu:
            out["cpu"] = {"value": round(cpu["value"], 2), "cores": cpu["cores"], "kind": cpu["kind"]}
        lanes = lanes if lanes is not None else rec.get("lanes")
        if lanes:
            out["lanes"] = {"n": lanes.get("lanes"), "value": round(lanes["value"], 1)} if "value" in lanes else {"error": lanes.get("error", "")[:80]}
        return out
    out = {"taobao10": brief(dict(result, us_per_domain_step=result["us_per_domain_step"]), lanes_rec)}
    for name, rec in targets.items():
        out[name] = brief(rec)
    g_ = result.get("gather")
    if g_ and "frac" in g_:
        out["gather_hbm_microbench"] = {"GBps": round(g_["achieved"], 1), "frac": round(g_["frac"], 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed MAMDR meta-epochs (>= 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="taobao10", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: the per-kernel HIP-event pass, the other workloads and the "
                         "Amazon-6-sized gather (Taobao-10), the CPU baseline, the lanes.  Without it a run sets up, warms up, "
                         "times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (theta, phi, the live weights) as DIR/<name>.npy")
    ap.add_argument("--cpu-budget", type=float, default=None,
                    help="seconds of CPU-baseline work (0 = skip; default 20 with --full, else 0)")
    ap.add_argument("--no-profile", action="store_true", help="--full: skip the per-kernel HIP-event pass")
    ap.add_argument("--no-targets", action="store_true", help="--full: skip the other workloads and the Amazon-6-sized gather")
    ap.add_argument("--lanes", type=int, default=None,
                    help="single GPU: also time the same epochs sharded over this many lanes of one process "
                         "(0 = skip; default 4 with --full, else 0)")
    ap.add_argument("--rank-lanes", type=int, default=0,
                    help="several ranks: also time the epochs with this many lanes PER RANK (ranks x lanes: one world of "
                         "gpus * rank-lanes participants; 0 = skip)")
    ap.add_argument("--no-preflight", action="store_true",
                    help="several ranks: skip the first-contact check of the communicator (all-reduce, send / recv ring, broadcast)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_budget is None:
        args.cpu_budget = 20.0 if args.full else 0.0
    if args.lanes is None:
        args.lanes = 4 if args.full else 0
    args.no_profile = args.no_profile or not args.full
    args.no_targets = args.no_targets or not args.full

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.lanes > 1:
        # every lane's stream on a hardware queue of its own (the runtime's default of 4 is shared with torch's other
        # streams): 4 lanes 67 K instead of 46 K domain-steps/s, the single chain unchanged (profiles/r05_lanes_bench.txt).
        # Read by the HIP runtime when it initialises, i.e. at the first device call below.
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # MAMDR_BENCH_SHARE_GPU=1 (testing on a 1-GPU box only): all ranks use device 0 and gloo
        share = os.environ.get("MAMDR_BENCH_SHARE_GPU") == "1"
        import datetime
        if not share and torch.cuda.device_count() < world:
            # (one process per GPU: a rank without a device of its own must not fall back onto somebody else's)
            print("rank %d: %d ranks but %d visible GPUs" % (rank, world, torch.cuda.device_count()), file=sys.stderr)
            sys.exit(3)
        torch.cuda.set_device(0 if share else local_rank)
        backend = "gloo" if share else "nccl"
        # a collective that hangs (first contact with RCCL on a new machine) ends the rank after this long, non-zero
        limit = datetime.timedelta(seconds=int(os.environ.get("MAMDR_BENCH_COMM_TIMEOUT", "300")))
        if share:
            dist.init_process_group("gloo", timeout=limit)
        else:
            try:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=limit)
            except TypeError:
                dist.init_process_group("nccl", timeout=limit)
    else:
        torch.cuda.set_device(0)
    preflight = None
    if world > 1 and not args.no_preflight:
        from mamdr_amd import parallel as mpar
        preflight = mpar.preflight(torch.device("cuda", torch.cuda.current_device()))
        if rank == 0:
            print("preflight: %s" % json.dumps(preflight), file=sys.stderr)
    if args.gpus != world and rank == 0:
        print("warning: --gpus %d but WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)

    main_rec = run_workload(args.workload, args.steps, args.warmup, rank, world, not args.no_profile,
                            args.cpu_budget * (0.5 if not args.no_targets and args.workload == "taobao10" else 1.0),
                            dump_dir=args.dump_outputs)
    targets, gather = {}, None
    if not args.no_targets and args.workload == "taobao10":
        # north_star's target configuration in the same run: Taobao-30 bs 4096
        t30 = run_workload("taobao30", max(3, args.steps // 4), min(args.warmup, 2), rank, world, not args.no_profile,
                           args.cpu_budget * 0.3)
        targets["taobao30"] = {k: t30[k] for k in TARGET_KEYS if k in t30}
    if not args.no_targets and args.workload == "taobao10" and world == 1:
        # BASELINE.json configs[2] and configs[4] at FULL rows in the same run (single GPU: their multi-GPU numbers
        # come from `--workload amazon6|amazon13 --gpus N`): one warm-up epoch + two timed ones
        for wname in ("amazon6", "amazon13"):
            if os.environ.get("MAMDR_BENCH_SKIP_" + wname.upper()):
                continue
            try:        # (single process: an extra workload that fails is reported, the headline above stands)
                rec = run_workload(wname, 2, 1, rank, world, not args.no_profile, min(args.cpu_budget * 0.3, 8.0))
                targets[wname] = {k: rec[k] for k in TARGET_KEYS if k in rec}
            except Exception as e:      # noqa: BLE001
                import traceback
                traceback.print_exc(file=sys.stderr)
                targets[wname] = {"error": "%s: %s" % (type(e).__name__, e)}
    if not args.no_targets and rank == 0 and world == 1 and not args.no_profile:
        try:
            gather = gather_hbm_record(torch.device("cuda", torch.cuda.current_device()))
        except Exception as e:      # noqa: BLE001
            gather = {"error": "%s: %s" % (type(e).__name__, e)}
    lanes_rec = None
    if world > 1 and args.rank_lanes > 1:
        # ranks x lanes (every rank takes part; a failure here fails the run: the ranks must stay in step)
        lanes_rec = run_lanes(args.workload, args.steps, args.warmup, args.rank_lanes, outer=(rank, world))
    if world == 1 and args.lanes > 1:
        # (an extra beside `value`: a failure here is reported in the line, it does not cost the run its headline)
        try:
            lanes_rec = run_lanes(args.workload, args.steps, args.warmup, args.lanes)
            if "taobao30" in targets:
                t30l = run_lanes("taobao30", max(3, args.steps // 2), min(args.warmup, 2), args.lanes)
                t30l["over_single_chain"] = t30l["value"] / targets["taobao30"]["value"]
                targets["taobao30"]["lanes"] = t30l
        except Exception as e:      # noqa: BLE001
            import traceback
            traceback.print_exc(file=sys.stderr)
            if lanes_rec is None:
                lanes_rec = {"lanes": args.lanes, "error": "%s: %s" % (type(e).__name__, e)}
            else:
                targets["taobao30"]["lanes"] = {"lanes": args.lanes, "error": "%s: %s" % (type(e).__name__, e)}
    if rank == 0:
        r = main_rec
        result = {
            "metric": "domain-steps/sec", "value": r["value"], "unit": "domain-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": r["ms_per_step"], "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": r["workload"], "global_batch": r["global_batch"], "domains": r["domains"],
                       "domain_steps_per_epoch": r["domain_steps_per_epoch"],
                       "step_definition": "one MAMDR meta-epoch (DN + DR phases, all outer updates)",
                       "parallelism": ("per-epoch LPT of DR query domains + DN passes over %d ranks, 1 all-reduce per "
                                       "epoch (DN displacement + phi hand-over)" % world) if world > 1 else "single GPU"},
            "us_per_domain_step": r["us_per_domain_step"],
            # also domain-passes/sec (one pass = one domain's re-initialised iterator run to its end or
            # cap) and the epoch time (= ms_per_step: a bench step is one meta-epoch)
            "domain_passes_per_sec": r["domain_passes_per_sec"], "epoch_time_ms": r["ms_per_step"],
            "roofline": r["roofline"], "tower": r["tower"], "table_update": r["table_update"],
            "gather": gather, "gather_l2": r["gather_l2"], "gather_in_step": r.get("gather_in_step"),
            "kernels_avg_us": r["kernels_avg_us"],
            "cpu_baseline": r["cpu_baseline"], "host_ms_per_epoch": r["host_ms_per_epoch"],
            "host_prep_ms_per_epoch": r["host_prep_ms_per_epoch"], "prewarm_s": r["prewarm_s"], "targets": targets,
        }
        for rec_ in [result] + [t for t in targets.values() if isinstance(t, dict)]:
            if rec_.get("tower") is rec_.get("roofline") or rec_.get("tower") == rec_.get("roofline"):
                rec_["tower"] = "= roofline"
        if lanes_rec is not None:
            if "value" in lanes_rec:
                lanes_rec["over_single_chain"] = lanes_rec["value"] / r["value"]
            result["lanes"] = lanes_rec
        if world > 1:
            result["rccl_ranks"] = dist.get_world_size() if backend == "nccl" else 0
            result["backend"] = backend
            result["preflight"] = preflight
            for k in ("wire_bytes_per_epoch_rank0", "dn_mode"):
                if k in r:
                    result[k] = r[k]
            if "partition_speedup_bound" in r:
                # (Taobao-10 has 10 query domains: the partition itself bounds the speed-up, ~5x on 8 ranks)
                result["partition_speedup_bound"] = r["partition_speedup_bound"]
        if r.get("gpu_over_cpu") is not None:
            result["gpu_over_cpu"] = r["gpu_over_cpu"]
        # LAST key of the line: every workload of the run in a few hundred bytes each, so that a record which keeps only the
        # tail of stdout still carries all of them (round 5's record lost `targets.taobao30`); the bulky blocks sit above
        result["summary"] = summary_block(result, targets, lanes_rec)
        print(json.dumps(result))
        sys.stdout.flush()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
