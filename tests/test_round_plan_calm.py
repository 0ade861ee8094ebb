"""The calm-tiles flag of the host-side round plan (csrc/round_plan.h RoundPlan::calm) checked on the
CPU: host/round_plan_calm_test.cpp is a stand-alone program over the header alone (the flag over
shapes, knobs and facts: klazy sweep rounds at k = 8 that may leave stale votes, not the uniform-only
form, the option on; through a network's life; an option write clears nq_ok)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "round_plan_calm_test.cpp")


def test_round_plan_calm_program(tmp_path):
    exe = str(tmp_path / "round_plan_calm_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
