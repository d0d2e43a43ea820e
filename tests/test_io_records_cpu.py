"""The host-only shaping of what the single-launch entry points upload (dot_ring_amd/csrc/hostrecords.hpp): decoder inputs zero-padded to
their records, and Curve25519's identities split into flag words and cleaned points.  tests/native/io_records_check.cpp is built
stand-alone with g++ under the address and undefined-behaviour sanitizers and checks n = 0, 1, 3, records of 33 -> 36 and 32 -> 32 bytes,
and flags all zero, all one and mixed, given as flag bytes and as points of 0xff bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")


def test_records_and_identity_flags_under_sanitizers(tmp_path):
    exe = tmp_path / "io_records_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "io_records_check.cpp"), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    lines = proc.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 6 + 14 + 3 + 1 + 1
    assert "pad n=3 33->36" in lines and 'split "101" ff' in lines and 'split "010" given' in lines and 'split "000" null' in lines
