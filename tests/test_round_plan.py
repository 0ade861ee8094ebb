"""The host-side round plan (csrc/round_plan.h) checked on the CPU: host/round_plan_test.cpp is a
stand-alone program over the header alone (plan invariants over the full cross product of facts,
shapes and knobs; the fact sequences of the usual runs; the sweep grid against the two formulas it
replaced). The header must stay free of HIP: it is compiled here with plain g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "round_plan_test.cpp")


def test_round_plan_program(tmp_path):
    exe = str(tmp_path / "round_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
