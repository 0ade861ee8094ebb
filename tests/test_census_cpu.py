"""Network census, the parts that need no GPU: the entry point is exported, and
the numpy reference (census_ref.py) the GPU tests compare against does what
include/avhip.h defines, on hand-written words and on oracle networks."""
import ctypes

import numpy as np

import avhip
from census_ref import census_from_words, check_identities

P97 = int(0.97 * 2**32)


def word(count, a, v=0, c=0xFF):
    return v | (c << 8) | (((count << 1) | a) << 16)


ABSENT0, ABSENT1 = 0xFFFE0000, 0xFFFF0000


def test_census_exported():
    assert "av_census" in avhip.EXPORTED
    assert hasattr(ctypes.CDLL(avhip.LIB_PATH), "av_census")


def test_reference_hand_written():
    w = np.array([
        [word(0, 0), word(1, 1), ABSENT0, ABSENT1, word(127, 1)],
        [word(127, 0), word(1, 0, v=0x55), ABSENT1, ABSENT1, word(0, 1)],
        [ABSENT0, word(0, 1), ABSENT0, word(1, 1), word(127, 1, c=0x0F)],
    ], np.uint32)
    c = census_from_words(w)
    assert c["target_classes"].tolist() == [[2, 0, 1, 0], [1, 2, 0, 0], [0, 0, 2, 1], [0, 1, 0, 2], [0, 3, 0, 0]]
    assert c["target_count_sum"].tolist() == [127, 2, 0, 1, 254]
    assert c["node_classes"].tolist() == [[1, 2, 1, 1], [2, 1, 0, 2], [0, 3, 2, 0]]
    hist = np.zeros((2, 128), np.int64)
    hist[0, 0], hist[0, 1], hist[0, 127] = 1, 1, 1
    hist[1, 0], hist[1, 1], hist[1, 127] = 2, 2, 2
    assert np.array_equal(c["count_hist"], hist)
    check_identities(c, 3, 5)
    # honest mask: node 1 not counted
    mask = np.array([True, False, True])
    h = census_from_words(w, mask)
    assert h["target_classes"].tolist() == [[1, 0, 1, 0], [0, 2, 0, 0], [0, 0, 2, 0], [0, 1, 0, 1], [0, 2, 0, 0]]
    assert h["node_classes"].tolist() == [[1, 2, 1, 1], [0, 0, 0, 0], [0, 3, 2, 0]]
    assert h["target_count_sum"].tolist() == [0, 1, 0, 1, 254]
    check_identities(h, 2, 5, mask)


def test_reference_on_oracle_network(oracle):
    n, m = 50, 40
    sim = oracle.Sim(n, m, 8, seed=7, init_mode=3, init_param=P97)
    c = census_from_words(sim.dump())
    check_identities(c, n, m)
    assert c["target_classes"][:, 2:].sum() == 0  # every record live after init
    assert c["count_hist"].sum() == n * m and c["count_hist"][:, 1:].sum() == 0
    for _ in range(30):
        sim.run_round()
    c = census_from_words(sim.dump())
    check_identities(c, n, m)
    assert c["target_classes"][:, 2:].sum() > 0  # records finalized and deleted
    assert c["count_hist"].sum() == c["target_classes"][:, :2].sum()
