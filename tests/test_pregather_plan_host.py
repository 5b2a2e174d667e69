"""The slice planner of k_wgrad_adam's riders (mamdr_amd/csrc/pregather_plan.h) is host code without HIP dependencies:
tests/host/pregather_plan_check.cpp, a stand-alone program, walks it over all pass-size lists over {0, 1, 15, 16, 17, 1025} up to
length 4 with quotas {1, 64, 896} under the host compiler's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def test_planner_covers_every_position_once(tmp_path):
    exe = str(tmp_path / "pregather_plan_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "pregather_plan_check.cpp"), "-o", exe]
    comp = subprocess.run(cmd, capture_output=True, text=True)
    assert comp.returncode == 0, comp.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    # 1 + 6 + 36 + 216 + 1296 lists
    assert run.stdout.startswith("1555 pass lists, ") and run.stdout.strip().endswith(" 0 failures"), run.stdout
