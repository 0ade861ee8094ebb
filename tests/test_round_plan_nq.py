"""The network-quiet fact of the host-side round plan (csrc/round_plan.h nq_ok) checked on the CPU:
host/round_plan_nq_test.cpp is a stand-alone program over the header alone (nq_ok after each named
transition of RecordFacts, the plan's net_quiet_out / net_quiet_in over shapes, knobs and facts)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "round_plan_nq_test.cpp")


def test_round_plan_nq_program(tmp_path):
    exe = str(tmp_path / "round_plan_nq_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
