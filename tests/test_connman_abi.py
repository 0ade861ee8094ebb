"""CPU test of the peer-list calls' drop-in boundary (rule R6): av_set_peer_lists and av_unsent_polls
are exported by libavhip.so, declared in include/avhip.h and listed in the binding's tables (no
compute calls: there is no GPU here)."""
import ctypes
import os
import re

import avhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("av_set_peer_lists", "av_unsent_polls")


def test_library_exports_peer_list_symbols():
    lib = ctypes.CDLL(avhip.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declares_peer_list_symbols():
    with open(os.path.join(ROOT, "include", "avhip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^int\s+(av_\w+)\(", src, re.M))
    assert set(SYMBOLS) <= declared
    assert re.search(r"^#define AV_NO_PEER \(-1\)", src, re.M)
    assert re.search(r"^#define AVHIP_ABI_VERSION 1\b", src, re.M)  # additive change
    assert "av_set_peer_lists   <- Connman.AddNode / NodesIDs" in src  # the replaced-interfaces table


def test_binding_lists_peer_list_symbols():
    assert set(SYMBOLS) <= set(avhip.EXPORTED)
    L = avhip.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, s  # in the signature table
    assert avhip.NO_PEER == -1
    assert callable(avhip.Engine.set_peer_lists) and callable(avhip.Engine.unsent_polls)
