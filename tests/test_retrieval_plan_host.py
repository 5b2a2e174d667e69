"""The host driver of the retrieval calls (mamdr_amd/csrc/retrieval_host.h) is host code without HIP dependencies:
tests/host/retrieval_plan_check.cpp, a stand-alone program, drives retrieval_call in its three forms (top-K, ranks, slates) with a recording
backend over n_query {1, 255, 256, 257, 513} x rec_chunk {64, 128} x seven candidate counts x five target / slate layouts and
through the table of refusals, under the host compiler's address and undefined-behaviour sanitizers."""
import os
import subprocess

from test_pregather_plan_host import ROOT, host_compiler


def test_driver_plans_and_refuses_as_the_c_abi_states(tmp_path):
    exe = str(tmp_path / "retrieval_plan_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "retrieval_plan_check.cpp"), "-o", exe]
    comp = subprocess.run(cmd, capture_output=True, text=True)
    assert comp.returncode == 0, comp.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    # 5 x 2 x 7 x (3 top-K + 5 rank) + 5 x 5 x 2 slates calls; 26 + 23 + 17 rows of refusals
    assert run.stdout.startswith("610 calls walked, 66 refusals, ") and run.stdout.strip().endswith(" 0 failures"), run.stdout
