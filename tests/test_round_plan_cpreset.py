"""The preset-consider-planes fact of the host-side round plan (csrc/round_plan.h c_preset) checked on
the CPU: host/round_plan_cpreset_test.cpp is a stand-alone program over the header alone (random walks
over the named transitions as the engine drives them: c_preset implies fresh, never survives a cleared
fresh, the plan asks for the un-preset exactly when the planes are preset and the round is not the fresh
sweep round, never set for capped, compat or first-generation shapes)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "round_plan_cpreset_test.cpp")


def test_round_plan_cpreset_program(tmp_path):
    exe = str(tmp_path / "round_plan_cpreset_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
