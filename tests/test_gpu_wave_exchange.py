"""mamdr_amd/csrc/wave_exchange.h: the cross-lane exchanges of the step kernels' short reduction chains on the vector ALU
(v_permlane32_swap, v_permlane16_swap, DPP) instead of the LDS crossbar (`__shfl`, ds_bpermute_b32).

tests/device/wave_exchange_check.hip is a stand-alone HIP program (its own main; the header and nothing of the engine).
It runs every helper and the `__shfl` form kept beside it on the same 64-lane vectors -- random floats, +-0, denormals,
+-inf and NaN payloads, one distinct bit pattern per lane, so that a wrong pairing shows -- and compares the results as
uint32 bit patterns, lane by lane; where the host knows the answer (a pure move of the input's bits) the `__shfl` form
itself is checked too.  The program runs once, under a time limit; its report is printed.
(Sums over a wave that holds two DIFFERENT NaN payloads are not compared: see the program's header.)
"""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = ["wave_xor_get<%d>" % o for o in (1, 2, 4, 8, 16, 32)] + ["wave_xor_add<%d>" % o for o in (1, 2, 4, 8, 16, 32)] + \
          ["wave_xor_sum64", "wave_xor_sum_16_32", "wave_xor_dot64"] + ["wave_gather_rows16[%d]" % q for q in range(4)]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def test_valu_exchanges_match_their_shfl_forms_bit_for_bit(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    exe = str(tmp_path / "wave_exchange_check")
    cmd = [hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mamdr_amd", "csrc"),
           os.path.join(ROOT, "tests", "device", "wave_exchange_check.hip"), "-o", exe]
    comp = subprocess.run(cmd, capture_output=True, text=True)
    assert comp.returncode == 0, comp.stderr[-4000:]
    run = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-2000:])
    assert run.returncode == 0, (run.returncode, run.stdout[-4000:], run.stderr[-2000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ALL EQUAL", lines[-1]
    report = {l.split()[0]: l for l in lines[:-1]}
    for h in HELPERS:          # every helper was compared over whole waves, and nothing differs
        assert h in report, (h, sorted(report))
        words = report[h].split()
        assert int(words[1]) >= 64 * 20 and words[5] == "0" and words[11] == "0", report[h]
