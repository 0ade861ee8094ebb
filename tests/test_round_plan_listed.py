"""Rule R6 (per-node peer lists) in the host-side round plan, checked on the CPU:
host/round_plan_listed_test.cpp is a stand-alone program over csrc/round_plan.h alone, compiled here
with plain g++ (what a listed round plans and writes back first, with and without R5, the unsupported
combinations, replay rounds, the plans without lists, the facts after it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "round_plan_listed_test.cpp")


def test_round_plan_listed_program(tmp_path):
    exe = str(tmp_path / "round_plan_listed_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
