"""CPU: the recoder of batched MSMs over an SRS table with 16 or 32 blocks of odd-multiple rows (dot_ring_amd/csrc/msm_recode.hip.h:
for_each_wnaf_multiple_digit<16> and <32>), compiled for the host as it is.  tests/native/recode_multiples_wide_check.cpp holds it
against big integers for w = 9..13: sum +-(2 t + 1) b 2^row = k on the edge scalars of recode_check.cpp, single bits +- 1 .. 64, r - 1
and random scalars; one digit per slot, rows <= 255, b odd and below 2^(w-1), t < M; every multiplier inverse times its multiplier is
1 mod 2^32; the digit counts over 20 000 uniformly random scalars lie within 0.1 of the planner's figures (msm_plan.hpp:
NAF_MULTIPLE_DIGITS — 15.87 and 15.15 at w = 13, where 8 multiples have 16.60); the fullest bucket of a 6145-scalar vector holds at most
six times the mean list.  The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_wide_multiples_recoder_reconstructs_every_scalar(tmp_path, flags):
    exe = tmp_path / "recode_multiples_wide_check"
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "recode_multiples_wide_check.cpp"), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True)
    print(proc.stdout)
    assert proc.returncode == 0, proc.stderr[-4000:]
    assert "recoding with 16 and 32 multiples ok" in proc.stdout
