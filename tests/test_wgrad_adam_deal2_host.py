"""Both dealings of k_wgrad_adam (mamdr_amd/csrc/wgrad_adam_deal.h) as maps of the launch's 242 own workgroups to roles:
tests/host/wgrad_adam_deal2_check.cpp, a stand-alone program, checks under the host compiler's address and undefined-behaviour
sanitizers that each is a bijection onto the 32 S blocks, the 208 tiles and the 2 output-unit workgroups, that every residue
mod 8 (one XCD) holds 30 or 31 of them with its S workgroups first, and the line model with the output units' h3 lines: the
distinct 128-B operand lines per batch row and residue are 12 (13 where an output unit sits), 98 over the chip, under the
residue dealing, and 7 - 10, 69 over the chip, under the dealing by matrix (required: worst <= 10, total <= 74)."""
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


def test_both_dealings_are_bijections_and_the_one_by_matrix_reads_fewer_lines(tmp_path):
    exe = str(tmp_path / "wgrad_adam_deal2_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "wgrad_adam_deal2_check.cpp"), "-o", exe]
    comp = subprocess.run(cmd, capture_output=True, text=True)
    assert comp.returncode == 0, comp.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.strip() == ("lines per row and residue: residue dealing 13 13 12 12 12 12 12 12 worst 13 total 98; "
                                  "in order 15 15 14 14 14 14 14 14 worst 15 total 114; "
                                  "by matrix 8 9 10 7 7 9 9 10 worst 10 total 69; 0 failures"), run.stdout
