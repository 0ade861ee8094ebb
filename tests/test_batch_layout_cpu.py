"""The batch layouts (csrc/batch_layout.h) checked on the CPU: host/batch_layout_test.cpp is a
stand-alone program over the header alone. For every layout (the Response table, the grouping scratch,
the slot-vote, hashed and add batch heads, the admission table, the census sums, the catalog lookup's
staging) over m in {1 .. 4097}, 1 .. 64 Responses in every number of groups and several radix-temp
sizes: the measured size is the placed extent, every region is inside the buffer, aligned and disjoint,
the copy prefix ends with the table, and two instances agree on every offset. The placing pass fills
every region of a heap block of exactly the measured size, so an undersized layout is a sanitizer
report. Built plain and, where the compiler links them, with the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "go-avalanche_amd", "host", "batch_layout_test.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def sanitizers_link(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", *SAN, str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", *SAN]], ids=["plain", "sanitized"])
def test_batch_layout_program(tmp_path, flags):
    if SAN[0] in flags and not sanitizers_link(tmp_path):
        pytest.skip("this g++ does not link the sanitizer runtimes")
    exe = str(tmp_path / "batch_layout_test")
    subprocess.run([*BASE, *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS batch_layout" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
