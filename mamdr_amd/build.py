"""Build libmamdr_hip.so (gfx950) in-tree with hipcc.

Used by __graft_entry__.build().  The shared library lands next to this file
(mamdr_amd/libmamdr_hip.so): git-ignored, but it travels to the GPU box.

Diagnostic variants (extra -D flags on every compile) come from the same SOURCES and COMMON:
python -m mamdr_amd.build --variant <name> <flags...>, which tools/build_variant.sh wraps.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libmamdr_hip.so")
BUILD = os.path.join(HERE, "build")

# (source, extra flags).  outer_kernels must not fuse multiply-adds (bit-exact vs numpy).
SOURCES = [
    # (kernarg preload: the leading scalar arguments of k_tower / k_tower4 arrive in SGPRs with the wave)
    ("step_kernels.hip", ["-mllvm", "-amdgpu-kernarg-preload-count=14"]),
    # emb_kernels: the lazy and the dense table updates must round identically -> no implicit fma fusion
    # (HIP's __fmul_rn / __fadd_rn are plain operators; explicit __fmaf_rn where an fma is wanted)
    ("emb_kernels.hip", ["-ffp-contract=off"]),
    ("tower4_kernels.hip", ["-mllvm", "-amdgpu-kernarg-preload-count=14"]),
    ("fused_kernels.hip", []),
    ("star_kernels.hip", []),
    ("outer_kernels.hip", ["-ffp-contract=off"]),
    ("graph_engine.hip", []),
    # recommend_kernels: its register / LDS / scratch report: profiles/rank_bench.txt
    ("recommend_kernels.hip", ["-Rpass-analysis=kernel-resource-usage"]),
    # gauc_kernels: the fp64 terms are a division, a multiplication and additions as the host definition computes them
    # -> no fma fusion; its register / LDS / scratch report: profiles/gauc_bench.txt
    ("gauc_kernels.hip", ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"]),
    # exact_kernels: the AP term is the host definition's one division -> no fma fusion; its register / LDS / scratch
    # report: profiles/exact_metrics_bench.txt
    ("exact_kernels.hip", ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"]),
    # bootstrap_kernels: integers only; its register / LDS / scratch report: profiles/auc_bootstrap.txt
    ("bootstrap_kernels.hip", ["-Rpass-analysis=kernel-resource-usage"]),
    # isotonic_kernels: the fit is integers only; the score sums' terms are the host definition's operations -> no fma
    # fusion; its register / LDS / scratch report: profiles/isotonic_bench.txt
    ("isotonic_kernels.hip", ["-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage"]),
    # gram_kernels: its register / LDS / scratch report: profiles/conflict_bench.txt
    ("gram_kernels.hip", ["-Rpass-analysis=kernel-resource-usage"]),
    # list_kernels: the cosines' square root and divisions are IEEE (correctly rounded; hipcc's default, spelled out here);
    # its register / LDS / scratch report: profiles/list_metrics.txt
    ("list_kernels.hip", ["-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage"]),
    # diversify_kernels: list_kernels' cosines (same flag), and a value is three separately rounded operations -> no fma
    # fusion; its register / LDS / scratch report: profiles/list_diversify.txt
    ("diversify_kernels.hip", ["-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=off",
                               "-Rpass-analysis=kernel-resource-usage"]),
    # knn_kernels: list_kernels' cosines (same flag); its register / LDS / scratch report: profiles/knn_bench.txt
    ("knn_kernels.hip", ["-fhip-fp32-correctly-rounded-divide-sqrt", "-Rpass-analysis=kernel-resource-usage"]),
    # baseline_kernels: a similarity is a product, a sum and an IEEE division, separately rounded -> no fma fusion, correctly
    # rounded square root and division; its register / LDS / scratch report: profiles/baselines_bench.txt
    ("baseline_kernels.hip", ["-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=off",
                              "-Rpass-analysis=kernel-resource-usage"]),
    # host code only: the step engine's C ABI (map: csrc/step_ctx.h)
    ("mamdr_api.hip", []),
    ("step_context.hip", []),
    ("step_queries.hip", []),
    ("eval_metrics.hip", []),
    ("step_stateless.hip", []),
]
COMMON = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]
JOBS = 16       # compiles at a time, at most


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, out=OUT, build_dir=BUILD, extra_flags=()):
    """Compile SOURCES with COMMON (+ each file's own flags + extra_flags) into build_dir and link them into `out`."""
    os.makedirs(build_dir, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "mamdr_hip.h"))
    objs, todo = [], []
    for src, extra in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(build_dir, src.replace(".hip", ".o"))
        objs.append(o)
        cmd = [hipcc] + COMMON + extra + list(extra_flags) + ["-c", s, "-o", o]
        # a change of flags rebuilds too: the command line is kept next to the object
        stamp = o + ".cmd"
        same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
        if force or not same_cmd or _stale(o, [s] + headers):
            todo.append((cmd, stamp))

    def compile_one(job):
        cmd, stamp = job
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(stamp, "w") as f:
            f.write(" ".join(cmd))

    with ThreadPoolExecutor(max_workers=JOBS) as pool:
        list(pool.map(compile_one, todo))
    if force or _stale(out, objs):
        cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", out] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_variant(name, flags, force=False, verbose=True):
    """A diagnostic build of the same sources with extra flags on every compile: build/variants/lib<name>.so (load it with
    MAMDR_LIB_PATH); its objects live in build/variants/<name>/."""
    vdir = os.path.join(BUILD, "variants")
    return build(force=force, verbose=verbose, out=os.path.join(vdir, "lib%s.so" % name),
                 build_dir=os.path.join(vdir, name), extra_flags=flags)


if __name__ == "__main__":
    argv = sys.argv[1:]
    force = "--force" in argv
    if "--variant" in argv:      # python -m mamdr_amd.build --variant <name> <flags...>   (tools/build_variant.sh)
        rest = [a for a in argv[argv.index("--variant") + 1:] if a != "--force"]
        if not rest:
            sys.exit("usage: python -m mamdr_amd.build --variant <name> <flags...>")
        print("built", os.path.relpath(build_variant(rest[0], rest[1:], force=force)))
    else:
        build(force=force)
