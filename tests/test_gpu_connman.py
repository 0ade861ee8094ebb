"""Batched rounds over per-node peer lists (rule R6: av_set_peer_lists, av_unsent_polls, the listed
av_sample_peers / av_sample_lost; csrc/round_listed.hip) against the restated round of
tests/connman_ref.py over the oracle, round by round. Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import avhip
import connman_ref as CR
import lossy_ref as L

pytestmark = pytest.mark.gpu

SEED = 0xA7A1A9C4
P80 = int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)
AV_ERR_INVALID_ARG = -1
AV_ERR_UNSUPPORTED = -6


def rows(u):
    return [tuple(int(v) for v in r) for r in np.asarray(u).tolist()]


def make(oracle, n, m, k, byz=0, lists=None, **kw):
    eng = avhip.Engine(n, m, k=k, seed=SEED, byz_threshold=byz, **kw)
    eng.init_records(avhip.INIT_BERNOULLI, P80)
    sim = oracle.Sim(n, m, k, seed=SEED, byz_threshold=byz, init_mode=3, init_param=P80)
    ref = CR.ConnmanRef(sim, SEED)
    if lists is not None:
        set_lists(eng, ref, lists)
    return eng, ref


def set_lists(eng, ref, lists):
    eng.set_peer_lists(lists)
    ref.lists = lists


def down_nodes(count):
    return list(range(1, 1 + 2 * count, 2))


def same_pref(eng, ref):
    got, exp = eng.read_pref(), ref.sim.pref()
    np.testing.assert_array_equal(got[~ref.byz], exp[~ref.byz])
    flip = (1 - ((np.arange(ref.sim.m) ^ eng.round) & 1)).astype(np.uint8)
    np.testing.assert_array_equal(got[ref.byz], np.broadcast_to(flip, (int(ref.byz.sum()), ref.sim.m)))


def same_all(eng, ref, exp_updates, what):
    assert rows(eng.fetch_updates()) == rows(exp_updates), what
    np.testing.assert_array_equal(eng.read_records(), ref.sim.dump(), err_msg=what)
    same_pref(eng, ref)
    assert eng.applied_votes() == ref.applied, what
    assert eng.lost_responses() == ref.lost, what
    assert eng.unsent_polls() == ref.unsent, what


def plain_rounds(eng, ref, rounds, what):
    """Rounds of a perfect, fully connected network on both sides (the oracle's own round)."""
    for r in range(rounds):
        eng.run_rounds(1)
        same_all(eng, ref, ref.plain_round(), f"{what}, plain round {r}")


def listed_rounds(eng, ref, rounds, what, thr=0, mode=L.SKIP):
    for r in range(rounds):
        eng.run_rounds(1)
        same_all(eng, ref, ref.round(thr, mode), f"{what}, listed round {r}")


# ---- the draw ----

@pytest.mark.parametrize("k", [3, 8, 12])
def test_draw_parity(k):
    n = 97
    lists = CR.mixed_lists(n, k)
    eng = avhip.Engine(n, 40, k=k, seed=SEED)
    shard = avhip.Engine(n, 40, k=k, seed=SEED, node_range=(32, 64))
    eng.set_peer_lists(lists)
    shard.set_peer_lists(lists[32:64])  # its own nodes' lists, with global ids
    for rnd in (0, 1, 2**32 - 1):
        exp = CR.peer_table(SEED, lists, k, rnd)
        got = eng.sample_peers(rnd)
        np.testing.assert_array_equal(got, exp, err_msg=f"round {rnd}")
        assert (exp == CR.NO_PEER).any() and (exp[0] == CR.NO_PEER).all() and not (exp[6] == CR.NO_PEER).any()
        np.testing.assert_array_equal(eng.sample_peers(rnd, 40, 71), exp[40:71])
        np.testing.assert_array_equal(shard.sample_peers(rnd, 32, 64), got[32:64])
        assert not eng.sample_lost(rnd).any()  # nothing is lost without R5
    eng.close()
    shard.close()


@pytest.mark.parametrize("n,m", [(96, 40), (37, 33)])
def test_complete_lists_are_r1(oracle, n, m):
    """A list of every other node draws what AV_PEERS_RANDOM draws, and the listed kernel then computes
    what the oracle's own round computes."""
    eng, ref = make(oracle, n, m, 8)
    twin = avhip.Engine(n, m, k=8, seed=SEED)
    eng.set_peer_lists(CR.complete_lists(n))
    for rnd in (0, 1, 7, 2**32 - 1):
        np.testing.assert_array_equal(eng.sample_peers(rnd), twin.sample_peers(rnd))
    plain_rounds(eng, ref, 12, "complete lists")
    assert eng.unsent_polls() == 0 and eng.lost_responses() == 0
    eng.close()
    twin.close()


# ---- lives ----

LIFE = [
    # n, m, k, byz, rounds
    (96, 40, 8, 0, 40),
    (97, 40, 3, 0, 60),
    (70, 72, 12, 0, 40),
    (64, 2100, 8, 0, 30),  # BL 66: a node's lanes straddle two waves
    (96, 40, 8, BYZ20, 40),
]


@pytest.mark.parametrize("n,m,k,byz,rounds", LIFE, ids=[f"{c[0]}x{c[1]}k{c[2]}{'byz' if c[3] else ''}" for c in LIFE])
def test_life_parity(oracle, n, m, k, byz, rounds):
    """A network's life on the mixed topology, compared after every round. It ends with finalized
    records, with live ones (the isolated nodes never move) and with polls that were never sent."""
    eng, ref = make(oracle, n, m, k, byz, CR.mixed_lists(n, k))
    listed_rounds(eng, ref, rounds, "life")
    assert ref.finalized() > 0 and eng.finalized_count() > 0 and ref.live() > 0 and ref.unsent > 0
    w = ref.sim.dump()
    assert ((w[0::7] >> 17) < 128).all()  # nodes of degree 0
    eng.close()


def test_partition(oracle):
    """Two halves that cannot see each other: each finalizes every target on its own value."""
    n, m, k = 96, 40, 8
    eng = avhip.Engine(n, m, k=k, seed=SEED)
    sim = oracle.Sim(n, m, k, seed=SEED, init_mode=0, init_param=0)
    eng.admit_targets(list(range(m)), avhip.INIT_ACCEPTED, n0=0, n1=48, count=False)
    eng.admit_targets(list(range(m)), avhip.INIT_REJECTED, n0=48, n1=96, count=False)
    for j in range(n):
        for t in range(m):
            sim.add(j, t, 1 if j < 48 else 0)
    ref = CR.ConnmanRef(sim, SEED)
    set_lists(eng, ref, CR.group_lists(n, 2))
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    listed_rounds(eng, ref, 17, "partition")
    assert ref.live() == 0 and eng.live_records() == 0 and eng.unsent_polls() == 0
    cls = eng.census(nodes=False, hist=False, count_sum=False)["target_classes"]
    assert (cls[:, avhip.CENSUS_ABSENT_ACCEPTED] == 48).all() and (cls[:, avhip.CENSUS_ABSENT_REJECTED] == 48).all()
    eng.close()


@pytest.mark.parametrize("n,m", [(200, 1000), (96, 40)])
def test_partition_heal_partition(oracle, n, m):
    """Plain rounds (which leave stale vote planes and pending count steps behind), two groups, the
    whole network again, the mixed topology; a drop-in batch, an invalid target and admitted targets in
    between."""
    eng, ref = make(oracle, n, m, 8)
    sim = ref.sim
    plain_rounds(eng, ref, 12, "start")
    set_lists(eng, ref, CR.group_lists(n, 2))
    listed_rounds(eng, ref, 6, "two groups")
    # drop-in Responses between the stretches, one of them neutral
    nodes, targets = [2, 7, 2], [[0, 5, 33], [1, 2, 3, m - 1], [5, 6]]
    errs = [[0, 1, 0], [1, 0x80000000, 0, 1], [0, 0]]
    offs = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    got = eng.register_votes_batch(nodes, offs, np.concatenate(targets), np.concatenate(errs))
    exp = []
    for j, t, e in zip(nodes, targets, errs):
        st = dict(sim.register_votes(j, t, e))
        exp += [st.get(x, -1) for x in t]
    assert got.tolist() == exp
    ref.applied = eng.applied_votes()  # drop-in votes are counted by their own kernels: re-based
    eng.set_peer_lists(None)
    plain_rounds(eng, ref, 8, "healed")
    eng.set_valid(3, 0)
    ref.set_valid(3, 0)
    again = [0, 1, 34, m - 1]
    eng.admit_targets(again, avhip.INIT_ACCEPTED, count=False)
    for t in again:
        for j in range(n):
            sim.add(j, t, 1)
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    set_lists(eng, ref, CR.mixed_lists(n, 8))
    listed_rounds(eng, ref, 4, "mixed")
    assert ref.unsent > 0
    eng.close()


# ---- with R5 ----

@pytest.mark.parametrize("mode,loss,down", [(L.SKIP, 0.25, 8), (L.NEUTRAL, 0.08, 3)], ids=["skip", "neutral"])
@pytest.mark.parametrize("n,m,k", [(96, 40, 8), (70, 72, 12)])
def test_life_with_lost_responses(oracle, n, m, k, mode, loss, down):
    """R6 with R5: a slot that is not empty is lost by R5's rule; an empty slot registers nothing in
    either mode and is not a lost Response."""
    eng, ref = make(oracle, n, m, k, 0, CR.mixed_lists(n, k))
    thr = L.threshold(loss)
    eng.set_loss(thr, mode)
    eng.set_responding(down_nodes(down), 0)
    ref.set_responding(down_nodes(down), 0)
    both = 0
    for r in range(40):
        peers, lost = ref.tables(thr)
        assert not (lost & (peers == CR.NO_PEER)).any()
        both += int(((peers == CR.NO_PEER).any(axis=1) & lost.any(axis=1)).sum())
        if r in (0, 1, 20):
            np.testing.assert_array_equal(eng.sample_lost(r), lost.astype(np.uint8), err_msg=f"round {r}")
            np.testing.assert_array_equal(eng.sample_peers(r), peers, err_msg=f"round {r}")
        eng.run_rounds(1)
        same_all(eng, ref, ref.round(thr, mode), f"round {r}")
    assert both > 0  # some node had an empty and a lost slot in one round
    assert ref.lost > 0 and ref.unsent > 0 and ref.finalized() > 0
    eng.close()


def test_nonpolling_nodes_and_literal_responder(oracle):
    """Nodes whose run loop has returned send nothing (no unsent poll either) and still answer;
    responder 1 answers false for a record it deleted. Node 0 is idle and isolated."""
    n, m, k = 96, 40, 8
    eng, ref = make(oracle, n, m, k, 0, CR.mixed_lists(n, k))
    idle = [0, 11, 40, 95]
    eng.set_option("responder", 1)
    ref.set_responder(1)
    for j in idle:
        eng.set_polling(j, 0)
        ref.set_polling(j, 0)
    listed_rounds(eng, ref, 30, "idle nodes, responder 1")
    w = ref.sim.dump()
    assert ((w[idle] >> 17) < 128).all() and ((w >> 17) >= 128).any()
    per_round = sum(max(0, k - len(c)) for j, c in enumerate(ref.lists) if j not in idle)
    assert ref.unsent == 30 * per_round > 0
    eng.close()


def test_listed_round_right_after_init(oracle):
    """av_init_records leaves the consider planes preset for the fresh sweep round; a listed round
    comes instead and has them stored first."""
    n, m = 96, 1000
    lists = CR.mixed_lists(n, 8)
    eng, ref = make(oracle, n, m, 8)
    set_lists(eng, ref, lists)  # (after the init: the planes were preset for a plain round)
    listed_rounds(eng, ref, 3, "after init")
    eng.init_records(avhip.INIT_BERNOULLI, P80)  # and once more, at round 3, with the lists standing
    sim = oracle.Sim(n, m, 8, seed=SEED, init_mode=3, init_param=P80)
    sim.set_round_index(3)
    ref2 = CR.ConnmanRef(sim, SEED, lists)
    ref2.applied, ref2.unsent = ref.applied, ref.unsent
    listed_rounds(eng, ref2, 2, "after the second init")
    eng.close()


def test_all_lists_empty(oracle):
    n, m, k = 70, 100, 8
    eng, ref = make(oracle, n, m, k)
    plain_rounds(eng, ref, 3, "start")
    rec, pref, applied = eng.read_records(), eng.read_pref(), eng.applied_votes()
    eng.set_peer_lists([[] for _ in range(n)])
    assert (eng.sample_peers(eng.round) == avhip.NO_PEER).all()
    eng.run_rounds(1)
    assert eng.updates_count() == 0 and len(eng.fetch_updates()) == 0
    np.testing.assert_array_equal(eng.read_records(), rec)
    np.testing.assert_array_equal(eng.read_pref(), pref)
    assert eng.unsent_polls() == n * k and eng.lost_responses() == 0 and eng.applied_votes() == applied
    assert eng.round == 4
    # cleared: the network goes on where the reference does, one round index later
    eng.set_peer_lists(None)
    ref.sim.set_round_index(4)
    ref.unsent += n * k
    plain_rounds(eng, ref, 3, "cleared")
    eng.close()


def test_set_then_clear_is_a_no_op(oracle):
    """set_peer_lists(lists) then set_peer_lists(None) before the first round: the same updates,
    records, launches, network-quiet rounds, applied votes and model bytes as an untouched twin."""
    n, m = 64, 1000
    out = []
    for touched in (False, True):
        eng = avhip.Engine(n, m, k=8, seed=SEED)
        eng.init_records(avhip.INIT_BERNOULLI, P80)
        eng.set_timing(True)
        if touched:
            eng.set_peer_lists(CR.mixed_lists(n, 8))
            eng.set_peer_lists(None)
        ups = []
        for _ in range(30):
            eng.run_rounds(1)
            ups.append(eng.fetch_updates(decode=False))
        _, launches = eng.kernel_stats()
        out.append((np.concatenate(ups), eng.read_records(), launches, eng.net_quiet_rounds, eng.applied_votes(),
                    eng.alg_bytes(), eng.unsent_polls(), eng.lost_responses()))
        eng.close()
    a, b = out
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2:] == b[2:] and a[6] == 0 and a[7] == 0


def test_target_shards_agree(oracle):
    n, m, k = 64, 96, 8
    thr = L.threshold(0.25)
    lists = CR.mixed_lists(n, k)
    whole = avhip.Engine(n, m, k=k, seed=SEED)
    parts = [avhip.Engine(n, m, k=k, seed=SEED, target_range=r) for r in ((0, 64), (64, 96))]
    for e in [whole] + parts:
        e.init_records(avhip.INIT_BERNOULLI, P80)
        e.set_peer_lists(lists)
        e.set_loss(thr, L.SKIP)
        e.set_responding(down_nodes(4), 0)
    for r in range(40):
        for e in [whole] + parts:
            e.run_rounds(1)
        np.testing.assert_array_equal(np.concatenate([e.read_records() for e in parts], axis=1), whole.read_records(),
                                      err_msg=f"round {r}")
        np.testing.assert_array_equal(np.concatenate([e.read_pref() for e in parts], axis=1), whole.read_pref())
        got = np.concatenate([e.fetch_updates() for e in parts])
        exp = whole.fetch_updates()
        assert sorted(rows(got)) == sorted(rows(exp)), f"round {r}"
        assert all(e.lost_responses() == whole.lost_responses() for e in parts)
        assert all(e.unsent_polls() == whole.unsent_polls() for e in parts)
    assert sum(e.applied_votes() for e in parts) == whole.applied_votes()
    assert whole.finalized_count() > 0 and whole.unsent_polls() > 0 and whole.lost_responses() > 0
    for e in [whole] + parts:
        e.close()


# ---- errors ----

def refused(call, code):
    with pytest.raises(avhip.AvError) as ei:
        call()
    assert ei.value.code == code


def raw_set(eng, offsets, peers):
    """av_set_peer_lists with the caller's arrays as they are."""
    o = np.ascontiguousarray(offsets, np.int64)
    p = np.ascontiguousarray(peers, np.int64)
    rc = avhip.lib().av_set_peer_lists(eng._h, o.ctypes.data, p.ctypes.data if p.size else None)
    return rc


def test_invalid_lists_change_nothing():
    n, k = 10, 3
    eng = avhip.Engine(n, 40, k=k, seed=SEED)
    good = CR.mixed_lists(n, k)
    eng.set_peer_lists(good)
    before = eng.sample_peers(5)
    offs = [0] + [2 * (i + 1) for i in range(n)]
    flat = [q for i in range(n) for q in sorted(((i + 1) % n, (i + 2) % n))]
    assert raw_set(eng, offs, flat) == 0  # the base every bad case below departs from
    np.testing.assert_array_equal(eng.sample_peers(5)[:, :2], np.array(flat).reshape(n, 2))
    eng.set_peer_lists(good)

    def bad(offsets, peers):
        assert raw_set(eng, offsets, peers) == AV_ERR_INVALID_ARG
        np.testing.assert_array_equal(eng.sample_peers(5), before)

    bad([1] + offs[1:], flat)  # offsets[0] != 0
    bad(offs[:4] + [offs[4] - 3] + offs[5:], flat)  # offsets decrease
    bad(offs, flat[:7] + [n] + flat[8:])  # out of range
    bad(offs, flat[:7] + [-1] + flat[8:])
    bad(offs, [0, 1] + flat[2:])  # node 0 lists itself
    bad(offs, [2, 1] + flat[2:])  # descending
    bad(offs, [2, 2] + flat[2:])  # a duplicate
    bad([0] + [2**31] * n, flat)  # 2^31 entries: refused before any is read
    with pytest.raises(ValueError):
        eng.set_peer_lists(good[:-1])  # one list per local node
    eng.close()


def test_unsupported_combinations():
    def unchanged_after(eng, call):
        rec, rnd = eng.read_records(), eng.round
        refused(call, AV_ERR_UNSUPPORTED)
        np.testing.assert_array_equal(eng.read_records(), rec)
        assert eng.round == rnd

    capped = avhip.Engine(64, 4200, k=8, seed=SEED)
    capped.init_records(avhip.INIT_BERNOULLI, P80)
    capped.run_rounds(2)
    capped.set_peer_lists(CR.mixed_lists(64, 8))
    unchanged_after(capped, lambda: capped.run_rounds(1))
    assert "4096" in str(avhip.lib().av_last_error())
    capped.set_peer_lists(None)
    capped.run_rounds(1)  # and the engine goes on once the lists are cleared
    assert capped.round == 3
    capped.close()

    readd = avhip.Engine(32, 40, k=8, seed=SEED)
    readd.init_records(avhip.INIT_BERNOULLI, P80)
    readd.set_option("responder", 2)
    readd.set_peer_lists(CR.mixed_lists(32, 8))
    unchanged_after(readd, lambda: readd.run_rounds(1))
    assert "responder" in str(avhip.lib().av_last_error())
    readd.set_option("responder", 1)  # IsAccepted literally runs
    readd.run_rounds(1)
    assert readd.round == 1 and readd.unsent_polls() > 0
    readd.close()

    group = [avhip.Engine(64, 40, k=8, seed=SEED, node_range=r) for r in ((0, 32), (32, 64))]
    for e in group:
        e.init_records(avhip.INIT_BERNOULLI, P80)
    group[1].set_peer_lists(CR.mixed_lists(64, 8)[32:])
    refused(lambda: avhip.peer_group_serial(group), AV_ERR_UNSUPPORTED)  # a listed engine cannot join
    group[1].set_peer_lists(None)
    avhip.peer_group_serial(group)
    unchanged_after(group[0], lambda: group[0].set_peer_lists(CR.mixed_lists(64, 8)[:32]))
    group[0].set_peer_lists(None)  # nothing set: allowed
    avhip.run_group_rounds(group, 2)
    assert group[0].round == 2 and group[1].round == 2
    for e in group:  # (closing one member closes the whole group; the others' close is then a no-op)
        e.close()

    robin = avhip.Engine(32, 40, k=8, seed=SEED, peer_mode=avhip.PEERS_ROUND_ROBIN)
    refused(lambda: robin.set_peer_lists(CR.mixed_lists(32, 8)), AV_ERR_UNSUPPORTED)
    robin.close()


def test_cpp_mirror_connman():
    """Engine::SetConnmans / ClearConnmans / UnsentPolls of the C++ mirror (host/avalanche_connman_tests.cpp)."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-avalanche_amd", "bin",
                       "avalanche_connman_tests")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS Connman" in r.stdout, r.stdout + r.stderr
