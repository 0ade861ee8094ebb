"""The host-side validation of av_set_peer_lists (rule R6), checked on the CPU:
host/peer_list_check_test.cpp is a stand-alone program over csrc/peer_list_check.h alone, compiled here
with plain g++ (what is accepted, every refusal, nothing changed after one)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "peer_list_check_test.cpp")


def test_peer_list_check_program(tmp_path):
    exe = str(tmp_path / "peer_list_check_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
