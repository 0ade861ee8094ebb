"""CPU test of the admission calls' drop-in boundary: av_admit_targets and
av_add_targets_batch are exported by libavhip.so, declared in include/avhip.h
and listed in the binding's tables (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import avhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("av_admit_targets", "av_add_targets_batch")


def test_library_exports_admission_symbols():
    lib = ctypes.CDLL(avhip.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declares_admission_symbols():
    with open(os.path.join(ROOT, "include", "avhip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^int\s+(av_\w+)\(", src, re.M))
    assert set(SYMBOLS) <= declared
    assert re.search(r"^#define AV_INIT_GIVEN 5\b", src, re.M)
    assert re.search(r"^#define AVHIP_ABI_VERSION 1\b", src, re.M)  # additive change


def test_binding_lists_admission_symbols():
    assert set(SYMBOLS) <= set(avhip.EXPORTED)
    L = avhip.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s  # in the signature table
    assert avhip.INIT_GIVEN == 5
    assert callable(avhip.Engine.admit_targets) and callable(avhip.Engine.add_targets_batch)
