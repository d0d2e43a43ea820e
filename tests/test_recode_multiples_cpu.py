"""CPU: the recoder of batched MSMs over an SRS table with odd-multiple rows (dot_ring_amd/csrc/msm_recode.hip.h:
for_each_wnaf_multiple_digit), compiled for the host as it is.  tests/native/recode_multiples_check.cpp holds it against big integers
for w = 9..13 and 2, 4 and 8 multipliers: sum +-(2 t + 1) b 2^row = k on the edges of the field, small values, single bits and their
neighbours, runs of ones across every slot boundary, alternating patterns, 2^w - 1 and the sign thresholds at every position and
random scalars; one digit per slot, rows <= 255, b odd and below 2^(w-1); 18.06 / 17.31 / 16.61 +- 0.1 digits per scalar at w = 13
over 20 000 uniformly random scalars; the fullest bucket of a 6145-scalar vector at most six times the mean list.  The same program
runs once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_multiples_recoder_reconstructs_every_scalar(tmp_path, flags):
    exe = tmp_path / "recode_multiples_check"
    subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "recode_multiples_check.cpp"), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-4000:]
    assert "recoding with multiples ok" in proc.stdout
