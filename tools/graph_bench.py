"""Throughput of the generic-layer engine (csrc/graph_engine.hip) on the reference's Taobao-10 multi-task configurations
and on the deepctr single-output towers it hosts: domain-steps/s of the alternate training loop (deep_mtl_ctr.py:69-96 /
deepctr.py:63-93: one full pass per domain per epoch), synthetic Taobao-10 logs, batch 1024, inputs resident in HBM.
usage: python tools/graph_bench.py [epochs [tower,tower...|all [inproc|- [emb_dim [hidden [norm dense aux [split [batch [scale]]]]]]]]]
-> one JSON line per tower
(`inproc`: every tower in THIS process -- what a profiler needs, which must not see a process that has initialised the GPU
start another program; emb_dim: user_dim = item_dim = domain_dim of the run and the width of the generated tables, for
the towers that take one -- mlp / wdl / deepfm, named explicitly, e.g. `3 mlp - 64 128x64`; hidden: hidden_dim as AxBxC;
norm dense aux: the Star form of tower `star`, e.g. `3 star - 128 256x128x64 bn dense 0` -- pn star 0 at 256x128x64 is the step
kernels' form unless MAMDR_STAR_ENGINE=graph sends it to this engine; split: a directory of config/, e.g. Amazon_13; batch:
dataset.batch_size, then dataset.synthetic_scale; `-` keeps a default)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mamdr_amd import cli, synthetic  # noqa: E402
from mamdr_amd.plan import PassShuffler  # noqa: E402
from mamdr_amd.utils import MultiDomainDataset  # noqa: E402

EPOCHS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ONLY = sys.argv[2].split(",") if len(sys.argv) > 2 and sys.argv[2] != "all" else None
INPROC = len(sys.argv) > 3 and sys.argv[3] == "inproc"
def _arg(i):
    return sys.argv[i] if len(sys.argv) > i and sys.argv[i] != "-" else None


EMB_DIM = int(_arg(4)) if _arg(4) else None
HIDDEN = [int(h) for h in _arg(5).split("x")] if _arg(5) else None
STAR_FORM = dict(norm=_arg(6), dense=_arg(7), auxiliary_net=_arg(8) not in ("0", "false")) if _arg(6) and _arg(7) and _arg(8) else None
SPLIT = _arg(9) or "Taobao-10"
BATCH = int(_arg(10)) if _arg(10) else None
SCALE = float(_arg(11)) if _arg(11) else None       # dataset.synthetic_scale (rows of the generated logs; the tables keep their size)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step_macs_per_row(eng, domain=0):
    """forward multiply-adds per batch row of the dense layers on ONE step's path (a step of task d runs the shared
    experts and task d's own experts / gate / tower); a training step costs 6 flop per such MAC (forward, d input,
    d weights).  AutoInt's attention projections run on 3 token rows per batch row."""
    if hasattr(eng, "shapes"):
        ranges = eng.task_ranges(domain) if hasattr(eng, "task_ranges") else [(0, eng.n_params)]
        macs = 0
        for name, (rows, cols) in eng.shapes.items():
            off = eng.segments[name][0]
            if not any(o <= off < o + c for o, c in ranges) or rows <= 1 or name.endswith("_emb") or name.startswith("lin_"):
                continue
            if name.startswith(("Wd", "bd", "pn_", "bn_")):      # Star: ONE contraction per layer on Ws (.) Wd[d] (counted at Ws)
                continue
            if name == "aux_W":                                  # ... and one on the slice aux_W[d]
                rows //= eng.n_domain
            macs += rows * cols * (3 if name.startswith("att") else 1)
        return macs
    return sum(c for n, (_, c) in eng.segments.items() if n in ("W0", "W0x", "W1", "W2", "wo"))


PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md (bench.py uses the same figure)


TOWERS = ("shared_bottom", "mmoe", "ple", "nfm", "pnn", "ccpm", "autoint")
if not INPROC and (ONLY is None or len(ONLY) > 1):
    # one process per tower (started before this one touches the GPU): in one process a tower measured after a bigger one
    # now and then runs 3x slower than on its own (nfm after ple: 113 us, 113 us, 367 us, ... in five identical runs)
    import subprocess
    for name in TOWERS:
        if ONLY is None or name in ONLY:
            subprocess.run([sys.executable, os.path.abspath(__file__), str(EPOCHS), name, "-"] + sys.argv[4:], check=False)
    sys.exit(0)

# (mlp / wdl / deepfm run here when named: on this engine with a width or a hidden_dim the step kernels are not built for)
for cfg_name in TOWERS + tuple(n for n in (ONLY or ()) if n not in TOWERS):
    if ONLY is not None and cfg_name not in ONLY:
        continue
    path = os.path.join(ROOT, "config", SPLIT, cfg_name + ".json")
    if cfg_name == "star" and not os.path.exists(path):
        path = os.path.join(ROOT, "config", SPLIT, "star_taobao.json")
    if os.path.exists(path):
        cfg = json.load(open(path))
    else:
        cfg = json.load(open(os.path.join(ROOT, "config", SPLIT, "deepctr_taobao_10.json" if SPLIT == "Taobao-10" else "deepctr.json")))
        cfg["model"]["name"] = cfg_name
    if STAR_FORM is not None and cfg_name == "star":
        cfg["model"].update(STAR_FORM)
    if BATCH is not None:
        cfg["dataset"]["batch_size"] = BATCH
    if SCALE is not None:
        cfg["dataset"]["synthetic_scale"] = SCALE
    cfg["train"].update(result_save_path="/tmp/graph_bench/result", checkpoint_path="/tmp/graph_bench/ckpt")
    if EMB_DIM is not None:
        cfg["model"].update(user_dim=EMB_DIM, item_dim=EMB_DIM, domain_dim=EMB_DIM)
        cfg["dataset"]["synthetic_emb_dim"] = EMB_DIM
    if HIDDEN is not None:
        cfg["model"]["hidden_dim"] = HIDDEN
    ds = MultiDomainDataset(cfg["dataset"])
    model = cli.build_model(cfg, ds)
    eng = model.model
    D = ds.n_domain
    sizes = {d: v["n_data"] for d, v in ds.train_dataset.items()}
    sh = PassShuffler(sizes, 10000, 123)
    perms = {d: torch.from_numpy(sh(d)).to(eng.device) for d in range(D)}
    steps_per_epoch = sum(-(-sizes[d] // ds.batch_size) for d in range(D))

    def epoch():
        for d in range(D):
            eng.train_steps(d, perm=perms[d], lr=cfg["train"]["learning_rate"])
    epoch()
    torch.cuda.synchronize()
    graph = hasattr(eng, "shapes")
    l0 = int(eng.lib.mamdr_graph_launch_count())
    t0 = time.perf_counter()
    for _ in range(EPOCHS):
        epoch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    launches = (int(eng.lib.mamdr_graph_launch_count()) - l0) / float(steps_per_epoch * EPOCHS) if graph else None
    n_path = 0
    if hasattr(eng, "task_ranges") and cfg_name in ("shared_bottom", "mmoe", "ple"):
        n_path = sum(c for _, c in eng.task_ranges(0))
    rows = sum(sizes.values()) * EPOCHS
    macs = step_macs_per_row(eng)
    ach = 6.0 * macs * rows / dt / 1e12
    roofline = {"bound": "mfma", "scope": "whole step (every launch of a domain-step; the engine has no single dominant kernel)"
                if graph else "whole step (k_tower4<DX, FM> + k_wgrad + k_update)",
                "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_F32_MFMA_TFLOPS,
                "flops_per_row": 6 * macs, "launches_per_step": launches if graph else 3}
    print(json.dumps({"tower": cfg_name, "engine": "generic-layer (mamdr_graph_*)" if graph else "step kernels (mamdr_*)",
                      "value": steps_per_epoch * EPOCHS / dt, "unit": "domain-steps/s",
                      "us_per_domain_step": dt / (steps_per_epoch * EPOCHS) * 1e6, "batch": ds.batch_size, "roofline": roofline,
                      "params": int(eng.n_params), "params_on_a_step_path": int(n_path) or int(eng.n_params),
                      "emb_dim": cfg["model"]["user_dim"], "split": SPLIT,
                      "star_form": {k: cfg["model"].get(k) for k in ("norm", "dense", "auxiliary_net")} if cfg_name == "star" else None,
                      "model": {k: cfg["model"][k] for k in cfg["model"] if "hidden" in k or "expert" in k}}))
    eng.close()
