"""The Hash catalog's host module (csrc/catalog.h) checked on the CPU: host/catalog_test.cpp is a
stand-alone program over the header alone (random walks of intern / retire / find against a std::map
model, the lowest-free-slot rule, duplicates, the full catalog, the keys 0, -1, INT64_MIN, INT64_MAX and
keys equal to slot numbers, churn at 33 and 64 slots that rebuilds the table image several times, the
image walked with the probe function the device shares after every step). Built plain and, where the
compiler links them, with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "catalog_test.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def sanitizers_link(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", *SAN, str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", *SAN]], ids=["plain", "sanitized"])
def test_catalog_program(tmp_path, flags):
    if SAN[0] in flags and not sanitizers_link(tmp_path):
        pytest.skip("this g++ does not link the sanitizer runtimes")
    exe = str(tmp_path / "catalog_test")
    subprocess.run([*BASE, *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS catalog" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
