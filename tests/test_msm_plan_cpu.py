"""CPU: the plan of the G1 Pippenger (dot_ring_amd/csrc/msm_plan.hpp), compiled for the host as it is.
tests/native/msm_plan_check.cpp checks the plan's invariants over a sweep of sizes, batches, table shapes and knobs (the non-adjacent form
only with the LDS sort and the set scan, bucket and digit counts below 2^32, the workgroup scan's span dividing its sets, the table row
bound) and pins the sort, reduction and finish path of every shape the GPU tests and bench.py name."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msm_plan_invariants_and_named_paths(tmp_path):
    exe = tmp_path / "msm_plan_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "msm_plan_check.cpp"), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert "msm plan ok" in proc.stdout
