"""CPU checks of tests/lossy_ref.py, the restated round with lost Responses (rule R5) that
tests/test_gpu_lossy.py compares the engine with: at zero loss both of its routes are the oracle's
own round, under loss the two neutral routes agree, and the loss draw reproduces a fixed table."""
import numpy as np
import pytest

import lossy_ref as L

SEED = 0xA7A1A9C4
P80 = int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)


def make(oracle, n, m, k, byz=0):
    return oracle.Sim(n, m, k, seed=SEED, byz_threshold=byz, init_mode=3, init_param=P80)


def same_state(a, b, what):
    np.testing.assert_array_equal(a.dump(), b.dump(), err_msg=what)
    np.testing.assert_array_equal(a.pref(), b.pref(), err_msg=what)
    assert a.round == b.round


@pytest.mark.parametrize("byz", [0, BYZ20], ids=["honest", "byz20"])
def test_zero_loss_is_the_oracle_round(oracle, byz):
    """Both routes reproduce Sim.run_round() bit for bit when nothing is lost, through finalization."""
    plain, a, b = (make(oracle, 24, 40, 8, byz) for _ in range(3))
    ra, rb = L.LossyRef(a, SEED), L.LossyRef(b, SEED)
    applied = 0
    for r in range(30):
        exp, ap = plain.run_round()
        applied += ap
        np.testing.assert_array_equal(ra.round(0, L.SKIP), exp, err_msg=f"register_votes route, round {r}")
        np.testing.assert_array_equal(rb.round_replay(0), exp, err_msg=f"replay route, round {r}")
        same_state(plain, a, f"round {r}")
        same_state(plain, b, f"round {r}")
    assert ra.applied == applied and rb.applied == applied and ra.lost == 0 and rb.lost == 0
    assert ((plain.dump() >> 17) >= 128).any()  # some records finalized and were deleted on the way


def test_zero_loss_nonpolling_nodes_and_literal_responder(oracle):
    """The same identity with nodes that no longer poll (they still answer) and responder 1
    (IsAccepted literally: false once the record is deleted), the oracle's own notions of both."""
    plain, a, b = (make(oracle, 24, 40, 8) for _ in range(3))
    ra, rb = L.LossyRef(a, SEED), L.LossyRef(b, SEED)
    plain.set_responder(1)
    for j in (2, 11):
        plain.set_polling(j, 0)
    for ref in (ra, rb):
        ref.set_responder(1)
        for j in (2, 11):
            ref.set_polling(j, 0)
    applied = 0
    for r in range(40):
        exp, ap = plain.run_round()
        applied += ap
        np.testing.assert_array_equal(ra.round(0, L.SKIP), exp, err_msg=f"register_votes route, round {r}")
        np.testing.assert_array_equal(rb.round_replay(0), exp, err_msg=f"replay route, round {r}")
        same_state(plain, a, f"round {r}")
        same_state(plain, b, f"round {r}")
    assert ra.applied == applied and rb.applied == applied
    w = plain.dump()
    assert ((w >> 17) >= 128).any() and ((w[[2, 11]] >> 17) < 128).all()  # deletions; none on the idle nodes


@pytest.mark.parametrize("n,m,k,byz", [(24, 40, 8, 0), (21, 37, 3, BYZ20), (20, 33, 12, 0)])
def test_neutral_routes_agree_under_loss(oracle, n, m, k, byz):
    a, b = make(oracle, n, m, k, byz), make(oracle, n, m, k, byz)
    ra, rb = L.LossyRef(a, SEED), L.LossyRef(b, SEED)
    for ref in (ra, rb):
        ref.set_responding([1, 4], 0)
    thr = L.threshold(0.15)
    for r in range(40):
        np.testing.assert_array_equal(ra.round(thr, L.NEUTRAL), rb.round_replay(thr), err_msg=f"round {r}")
        same_state(a, b, f"round {r}")
    assert ra.applied == rb.applied and ra.lost == rb.lost > 0
    # a neutral vote was shifted into some record that is still live: a consider byte that is not
    # a run of ones from bit 0 (which is all a perfect network ever produces)
    w = a.dump()
    cons = (w >> 8) & 0xFF
    live = (w >> 17) < 128
    assert (live & ((cons & (cons + 1)) != 0)).any() or not live.any()


def test_skip_differs_from_neutral(oracle):
    """The two modes are different rules: the same lost mask, other records."""
    a, b = make(oracle, 24, 40, 8), make(oracle, 24, 40, 8)
    ra, rb = L.LossyRef(a, SEED), L.LossyRef(b, SEED)
    thr = L.threshold(0.25)
    for _ in range(6):
        ra.round(thr, L.SKIP)
        rb.round(thr, L.NEUTRAL)
    assert ra.lost == rb.lost > 0
    assert ra.applied < rb.applied
    assert not np.array_equal(a.dump(), b.dump())


def test_loss_draw_table(oracle):
    """philox4x32-10(ctr = {node, round, slot >> 2, 6}, key = seed), word slot & 3, against values
    worked out once and committed here."""
    key = [SEED & 0xFFFFFFFF, SEED >> 32]
    table = {
        (0, 0, 0): [0x285B73CD, 0x71DCFF3D, 0x607CA3F2, 0xD13052F3],
        (5, 1, 1): [0xE6435A50, 0xBCAD916C, 0xF89160C6, 0xF1715353],
        (96, 2**32 - 1, 2): [0xA9D56A8A, 0x7D2256D9, 0xB3DB6ADD, 0x894868BB],
    }
    for (node, rnd, blk), words in table.items():
        assert [int(v) for v in oracle.philox([node, rnd, blk, L.DOM_LOSS], key)] == words
    thr = L.threshold(0.25)
    assert L.drawn_lost(SEED, 0, 0, 8, thr).tolist() == [True, False, False, False, True, False, True, False]
    assert L.drawn_lost(SEED, 5, 1, 8, thr).tolist() == [False] * 8
    assert L.drawn_lost(SEED, 96, 2**32 - 1, 8, thr).tolist() == [True, False, True, False, False, True, False, False]
    assert not L.drawn_lost(SEED, 0, 0, 12, 0).any()
    assert L.drawn_lost(SEED, 0, 0, 12, 2**32 - 1).all()
    # a peer that is down loses its slot whatever the draw says
    peers = oracle.sample_peers(SEED, 7, 3, 30, 8)
    t = L.lost_table(SEED, 30, 8, 3, 0, down=[int(peers[2]), int(peers[5])])
    assert t[7].tolist() == [False, False, True, False, False, True, False, False]
