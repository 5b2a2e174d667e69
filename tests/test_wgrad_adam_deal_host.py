"""The dealing arithmetic of k_wgrad_adam (mamdr_amd/csrc/wgrad_adam_deal.h) is host code without HIP dependencies:
tests/host/wgrad_adam_deal_check.cpp, a stand-alone program, checks under the host compiler's address and undefined-behaviour
sanitizers that the S workgroups' column blocks are a bijection of [0, 32) inside the half of dz1 their XCD's tiles read,
that every tile is dealt exactly once (26 per residue mod 8), and the line model: 12 distinct 128-B operand lines per batch
row and residue from the tiles, + 0 from the S workgroups as dealt, + 2 on every residue under blk = b."""
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


def test_dealing_is_a_bijection_and_keeps_the_s_blocks_on_their_xcd(tmp_path):
    exe = str(tmp_path / "wgrad_adam_deal_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "wgrad_adam_deal_check.cpp"), "-o", exe]
    comp = subprocess.run(cmd, capture_output=True, text=True)
    assert comp.returncode == 0, comp.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.strip() == ("32 S blocks, 208 tiles, 12 lines per row and residue; S workgroups' extra lines over "
                                  "8 residues: 0 dealt, 16 in order; 0 failures"), run.stdout
