"""The Hash catalog's entry points at the C boundary, without a GPU: exported by libavhip.so, declared
in include/avhip.h and listed in the binding, under the unchanged ABI version."""
import ctypes
import os
import re

import avhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["av_catalog_intern", "av_catalog_find", "av_catalog_find_device", "av_catalog_hashes", "av_catalog_retire",
           "av_register_votes_hashed"]
METHODS = ["catalog_intern", "catalog_find", "catalog_find_device", "catalog_hashes", "catalog_retire",
           "register_votes_hashed"]


def test_catalog_symbols_exported_declared_and_bound():
    with open(os.path.join(ROOT, "include", "avhip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(avhip.LIB_PATH)
    L = avhip.lib()
    for s in SYMBOLS:
        assert re.search(rf"^int {s}\(av_engine\* e, ", header, re.M), s
        assert hasattr(lib, s), s
        assert s in avhip.EXPORTED, s
        assert getattr(L, s).restype is ctypes.c_int32 and getattr(L, s).argtypes, s
    for m in METHODS:
        assert callable(getattr(avhip.Engine, m)), m
    # the hashed vote call takes the batch call's arguments
    assert L.av_register_votes_hashed.argtypes == L.av_register_votes_batch.argtypes


def test_abi_version_unchanged():
    with open(os.path.join(ROOT, "include", "avhip.h")) as f:
        assert re.search(r"^#define AVHIP_ABI_VERSION 1$", f.read(), re.M)
    assert avhip.lib().av_abi_version() == 1
