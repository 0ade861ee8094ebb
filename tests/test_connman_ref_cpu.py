"""CPU checks of tests/connman_ref.py, the restated round over per-node peer lists (rule R6) that
tests/test_gpu_connman.py compares the engine with: complete lists draw what R1 draws and run the
oracle's own round, short lists come out in order with empty slots behind them, drawn lists give
distinct members, and a network of empty lists does nothing."""
import numpy as np
import pytest

import connman_ref as CR

SEED = 0xA7A1A9C4
P80 = int(0.8 * 2**32)


@pytest.mark.parametrize("n,k", [(n, k) for n in (9, 10, 13, 97) for k in (3, 8, 12) if n - 1 >= k])
def test_complete_lists_draw_r1(oracle, n, k):
    """A list of every other node (N - 1 >= k) is AV_PEERS_RANDOM's draw, k = N - 1 included (with
    fewer than k other nodes R1 repeats peers and R6 leaves slots empty: not the same rule)."""
    lists = CR.complete_lists(n)
    for rnd in (0, 1, 5, 2**32 - 1):
        for node in range(n):
            got = CR.listed_peers(SEED, node, rnd, k, lists[node])
            np.testing.assert_array_equal(got, oracle.sample_peers(SEED, node, rnd, n, k), err_msg=f"{node} {rnd}")


@pytest.mark.parametrize("k", [3, 8, 12])
def test_short_lists_come_in_order(k):
    for d in range(k + 1):
        peers = sorted(range(5, 5 + 3 * d, 3))
        got = CR.listed_peers(SEED, 2, 7, k, peers)
        assert got[:d].tolist() == peers and (got[d:] == CR.NO_PEER).all()


@pytest.mark.parametrize("k", [3, 8, 12])
@pytest.mark.parametrize("extra", [1, None], ids=["k_plus_1", "d20"])
def test_drawn_lists_give_distinct_members(k, extra):
    d = k + 1 if extra else 20
    peers = sorted(range(100, 100 + 7 * d, 7))
    seen = set()
    for node in range(40):
        for rnd in (0, 3, 2**32 - 1):
            got = CR.listed_peers(SEED, node, rnd, k, peers).tolist()
            assert len(set(got)) == k and set(got) <= set(peers)
            seen.add(tuple(got))
    assert len(seen) >= 20  # and it is a draw (k = 3 of 4 has 24 outcomes): not the list's head every time


@pytest.mark.parametrize("n,m,k", [(37, 33, 8), (30, 20, 3)])
def test_complete_lists_are_the_oracle_round(oracle, n, m, k):
    """The restated round with complete lists and no loss is Sim.run_round: updates and records."""
    plain = oracle.Sim(n, m, k, seed=SEED, init_mode=3, init_param=P80)
    sim = oracle.Sim(n, m, k, seed=SEED, init_mode=3, init_param=P80)
    ref = CR.ConnmanRef(sim, SEED, CR.complete_lists(n))
    applied = 0
    for r in range(10):
        exp, ap = plain.run_round()
        applied += ap
        np.testing.assert_array_equal(ref.round(), exp, err_msg=f"round {r}")
        np.testing.assert_array_equal(sim.dump(), plain.dump(), err_msg=f"round {r}")
        np.testing.assert_array_equal(sim.pref(), plain.pref(), err_msg=f"round {r}")
        assert sim.round == plain.round
    assert ref.applied == applied and ref.unsent == 0 and ref.lost == 0


def test_empty_lists_change_nothing(oracle):
    n, m, k = 20, 33, 8
    sim = oracle.Sim(n, m, k, seed=SEED, init_mode=3, init_param=P80)
    ref = CR.ConnmanRef(sim, SEED, [[] for _ in range(n)])
    before, pref = sim.dump().copy(), sim.pref().copy()
    assert len(ref.round()) == 0
    np.testing.assert_array_equal(sim.dump(), before)
    np.testing.assert_array_equal(sim.pref(), pref)
    assert ref.unsent == n * k and ref.applied == 0 and ref.lost == 0 and sim.round == 1
    # down peers and a loss draw lose nothing where nothing was sent
    ref.set_responding(list(range(n)), 0)
    assert not CR.lost_table(SEED, ref.lists, k, 1, 2**32 - 1, ref.down).any()


def test_mixed_topology_shape():
    lists = CR.mixed_lists(97, 8)
    assert [len(c) for c in lists[:7]] == [0, 1, 3, 8, 9, 20, 96]
    assert all(c == sorted(set(c)) and i not in c for i, c in enumerate(lists))
    assert CR.mixed_lists(97, 8) == lists  # seeded
    g = CR.group_lists(96, 2)
    assert g[0] == list(range(1, 48)) and g[95] == list(range(48, 95))
