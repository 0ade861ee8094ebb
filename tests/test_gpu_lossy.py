"""Batched rounds with lost Responses and unresponsive nodes (rule R5: av_set_loss,
av_set_responding, av_sample_lost, av_lost_responses; csrc/round_lossy.hip) against the restated
round of tests/lossy_ref.py over the oracle. Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import avhip
import lossy_ref as L

pytestmark = pytest.mark.gpu

SEED = 0xA7A1A9C4
P80 = int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)
AV_ERR_UNSUPPORTED = -6


def rows(u):
    return [tuple(int(v) for v in r) for r in np.asarray(u).tolist()]


def make(oracle, n, m, k, byz=0, **kw):
    eng = avhip.Engine(n, m, k=k, seed=SEED, byz_threshold=byz, **kw)
    eng.init_records(avhip.INIT_BERNOULLI, P80)
    sim = oracle.Sim(n, m, k, seed=SEED, byz_threshold=byz, init_mode=3, init_param=P80)
    return eng, L.LossyRef(sim, SEED)


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


def plain_rounds(eng, ref, rounds, what):
    """Rounds of a perfect network on both sides (the oracle's own round)."""
    for r in range(rounds):
        eng.run_rounds(1)
        exp, ap = ref.sim.run_round()
        ref.applied += ap
        same_all(eng, ref, exp, f"{what}, plain round {r}")


def lossy_rounds(eng, ref, rounds, thr, mode, what):
    for r in range(rounds):
        eng.run_rounds(1)
        same_all(eng, ref, ref.round(thr, mode), f"{what}, lossy round {r}")


@pytest.mark.parametrize("k", [3, 8, 12])
def test_sample_lost_matches_the_draw(k):
    n, thr = 97, L.threshold(0.25)
    down = [0, 13, 50, 64, 96]
    eng = avhip.Engine(n, 40, k=k, seed=SEED)
    assert not eng.sample_lost(0).any()
    eng.set_loss(thr)
    eng.set_responding(down, 0)
    for rnd in (0, 1, 2**32 - 1):
        got = eng.sample_lost(rnd)
        exp = L.lost_table(SEED, n, k, rnd, thr, down)
        np.testing.assert_array_equal(got, exp.astype(np.uint8), err_msg=f"round {rnd}")
        assert exp.any() and not exp.all()
        np.testing.assert_array_equal(eng.sample_lost(rnd, 40, 71), exp[40:71].astype(np.uint8))
    # the down nodes alone, then nobody
    eng.set_loss(0)
    np.testing.assert_array_equal(eng.sample_lost(1), L.lost_table(SEED, n, k, 1, 0, down).astype(np.uint8))
    eng.set_responding(down, 1)
    assert not eng.sample_lost(1).any()
    eng.close()


LIFE = [
    # n, m, k, mode, loss, down, byz, rounds, must end with no live record
    (96, 40, 8, L.SKIP, 0.25, 8, 0, 80, True),
    (96, 40, 8, L.NEUTRAL, 0.08, 3, 0, 60, True),
    (97, 40, 3, L.SKIP, 0.25, 8, 0, 120, True),
    (70, 72, 12, L.NEUTRAL, 0.08, 3, 0, 60, True),
    (96, 40, 8, L.SKIP, 0.25, 8, BYZ20, 80, True),
    (37, 33, 8, L.SKIP, 0.25, 4, 0, 40, False),
    # BL 66; 30 rounds leave 4523 live records under the Philox draw, 37 rounds none
    (64, 2100, 8, L.NEUTRAL, 0.08, 3, 0, 40, True),
]


@pytest.mark.parametrize("n,m,k,mode,loss,down,byz,rounds,ends", LIFE,
                         ids=[f"{c[0]}x{c[1]}k{c[2]}{'neutral' if c[3] else 'skip'}{'byz' if c[6] else ''}" for c in LIFE])
def test_life_parity(oracle, n, m, k, mode, loss, down, byz, rounds, ends):
    """A network's whole life under loss, compared after every round: updates, records, published rows,
    applied votes, lost Responses; through finalization and deletion."""
    eng, ref = make(oracle, n, m, k, byz)
    thr = L.threshold(loss)
    eng.set_loss(thr, mode)
    eng.set_responding(down_nodes(down), 0)
    ref.set_responding(down_nodes(down), 0)
    lossy_rounds(eng, ref, rounds, thr, mode, "life")
    assert ref.lost > 0 and eng.finalized_count() > 0
    if ends:
        assert ref.live() == 0
    eng.close()


@pytest.mark.parametrize("mode", [L.SKIP, L.NEUTRAL], ids=["skip", "neutral"])
def test_life_nonpolling_nodes_and_literal_responder(oracle, mode):
    """Nodes whose run loop has returned (av_set_polling 0: they poll nothing, lose nothing and still
    answer) and responder 1 (a node answers false for a record it deleted) under loss, compared after
    every round like the other lives; two of the idle nodes are also down."""
    n, m, k = 96, 40, 8
    eng, ref = make(oracle, n, m, k)
    thr = L.threshold(0.25 if mode == L.SKIP else 0.08)
    idle, down = [2, 11, 40, 95], [11, 33, 40, 64]
    eng.set_option("responder", 1)
    ref.set_responder(1)
    for j in idle:
        eng.set_polling(j, 0)
        ref.set_polling(j, 0)
    eng.set_loss(thr, mode)
    eng.set_responding(down, 0)
    ref.set_responding(down, 0)
    lossy_rounds(eng, ref, 60, thr, mode, "idle nodes, responder 1")
    w = ref.sim.dump()
    assert ((w[idle] >> 17) < 128).all() and ((w >> 17) >= 128).any()  # the idle nodes' records never moved
    assert 0 < ref.lost <= 60 * (n - len(idle)) * k
    # an idle node polls again: it loses Responses like the others from then on
    eng.set_polling(2, 1)
    ref.set_polling(2, 1)
    lossy_rounds(eng, ref, 4, thr, mode, "node 2 polls again")
    eng.close()


@pytest.mark.parametrize("n,m", [(200, 1000), (96, 40)])
def test_transitions_on_one_engine(oracle, n, m):
    """Plain rounds (which leave stale vote planes and pending count steps behind), skip rounds, plain,
    neutral, plain again, with drop-in votes, an invalid target and admitted targets in between."""
    eng, ref = make(oracle, n, m, 8)
    sim = ref.sim
    thr = L.threshold(0.25)
    down = down_nodes(5)
    plain_rounds(eng, ref, 12, "start")
    eng.set_loss(thr, L.SKIP)
    eng.set_responding(down, 0)
    ref.set_responding(down, 0)
    lossy_rounds(eng, ref, 6, thr, L.SKIP, "skip")
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
    eng.set_loss(0)
    eng.set_responding(down, 1)
    ref.set_responding(down, 1)
    plain_rounds(eng, ref, 6, "plain again")
    eng.set_valid(3, 0)
    ref.set_valid(3, 0)
    eng.set_loss(L.threshold(0.08), L.NEUTRAL)
    eng.set_responding(down[:2], 0)
    ref.set_responding(down[:2], 0)
    lossy_rounds(eng, ref, 6, L.threshold(0.08), L.NEUTRAL, "neutral")
    # every node adds four targets again (re-adds of finalized ones included), as accepted
    again = [0, 1, 34, m - 1]
    eng.admit_targets(again, avhip.INIT_ACCEPTED, count=False)
    for t in again:
        for j in range(n):
            sim.add(j, t, 1)
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    eng.set_loss(0)
    eng.set_responding(down, 1)
    ref.set_responding(down, 1)
    plain_rounds(eng, ref, 10, "end")
    eng.close()


@pytest.mark.parametrize("how", ["neutral_rounds", "neutral_dropin"])
@pytest.mark.parametrize("n,m", [(96, 40), (70, 1000)])
def test_skip_rounds_after_a_neutral_vote(oracle, n, m, how):
    """Skip rounds on live records whose consider windows hold a zero below an all-ones oldest bit (left
    by neutral rounds, or by one neutral drop-in vote): the oldest plane no longer says that the
    younger ones are all-ones, so the warm form, which neither reads nor stores them, must not be
    taken."""
    eng, ref = make(oracle, n, m, 8)
    sim = ref.sim
    thr = L.threshold(0.25)
    plain_rounds(eng, ref, 2, "start")
    if how == "neutral_rounds":
        eng.set_loss(L.threshold(0.08), L.NEUTRAL)
        lossy_rounds(eng, ref, 3, L.threshold(0.08), L.NEUTRAL, "neutral")
    else:
        got = eng.register_votes(2, [5, 33], [0x80000000, 0x80000000])
        assert got.tolist() == [-1, -1] and sim.register_votes(2, [5, 33], [0x80000000, 0x80000000]) == []
        ref.applied = eng.applied_votes()  # (drop-in votes are counted by their own kernels: re-based)
    w = sim.dump()
    cons = ((w >> 8) & 0xFF)[(w >> 17) < 128]
    assert (((cons & 0x80) != 0) & (cons != 0xFF)).any()
    eng.set_loss(thr, L.SKIP)
    eng.set_responding(down_nodes(4), 0)
    ref.set_responding(down_nodes(4), 0)
    lossy_rounds(eng, ref, 6, thr, L.SKIP, "skip after a neutral vote")
    eng.set_loss(0)
    eng.set_responding(down_nodes(4), 1)
    ref.set_responding(down_nodes(4), 1)
    plain_rounds(eng, ref, 3, "end")
    eng.close()


@pytest.mark.parametrize("mode", [L.SKIP, L.NEUTRAL], ids=["skip", "neutral"])
def test_lossy_round_right_after_init(oracle, mode):
    """av_init_records leaves the consider planes preset for the fresh sweep round; a lossy round
    comes instead and has them stored first."""
    eng, ref = make(oracle, 96, 1000, 8)
    thr = L.threshold(0.25)
    eng.set_loss(thr, mode)
    lossy_rounds(eng, ref, 3, thr, mode, "after init")
    eng.init_records(avhip.INIT_BERNOULLI, P80)  # and once more, at round 3
    sim = oracle.Sim(96, 1000, 8, seed=SEED, init_mode=3, init_param=P80)
    sim.set_round_index(3)
    ref2 = L.LossyRef(sim, SEED)
    ref2.applied, ref2.lost = ref.applied, ref.lost
    lossy_rounds(eng, ref2, 2, thr, mode, "after the second init")
    eng.close()


def test_loss_zero_is_a_no_op(oracle):
    """set_loss(0) and set_responding(x, 1) change nothing: the same records, updates, launches and
    network-quiet rounds as an untouched twin."""
    n, m = 64, 1000
    out = []
    for touched in (False, True):
        eng = avhip.Engine(n, m, k=8, seed=SEED)
        eng.init_records(avhip.INIT_BERNOULLI, P80)
        eng.set_timing(True)
        if touched:
            eng.set_loss(0)
            eng.set_loss(0, L.NEUTRAL)
            eng.set_responding([3, 9], 1)
            eng.set_responding([], 0)
        ups = []
        for _ in range(30):
            eng.run_rounds(1)
            ups.append(eng.fetch_updates(decode=False))
        _, launches = eng.kernel_stats()
        out.append((np.concatenate(ups), eng.read_records(), launches, eng.net_quiet_rounds, eng.applied_votes(),
                    eng.lost_responses(), eng.alg_bytes()))
        eng.close()
    a, b = out
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2:] == b[2:] and a[5] == 0


def test_all_peers_down_skip(oracle):
    n, m, k = 70, 100, 8
    eng, ref = make(oracle, n, m, k)
    plain_rounds(eng, ref, 3, "start")
    rec, pref, applied = eng.read_records(), eng.read_pref(), eng.applied_votes()
    eng.set_responding(list(range(n)), 0)
    assert eng.sample_lost(eng.round).all()
    eng.run_rounds(1)
    assert eng.updates_count() == 0 and len(eng.fetch_updates()) == 0
    np.testing.assert_array_equal(eng.read_records(), rec)
    np.testing.assert_array_equal(eng.read_pref(), pref)
    assert eng.lost_responses() == n * k and eng.applied_votes() == applied and eng.round == 4
    # back up: the network goes on where the reference does, one round index later
    eng.set_responding(list(range(n)), 1)
    ref.sim.set_round_index(4)
    ref.lost += n * k
    plain_rounds(eng, ref, 3, "up again")
    eng.close()


def test_all_peers_down_neutral(oracle):
    n, m, k = 70, 100, 8
    eng, ref = make(oracle, n, m, k)
    plain_rounds(eng, ref, 3, "start")
    live = (eng.read_records() >> 17) < 128
    eng.set_loss(0, L.NEUTRAL)
    eng.set_responding(list(range(n)), 0)
    ref.set_responding(list(range(n)), 0)
    lossy_rounds(eng, ref, 1, 0, L.NEUTRAL, "all down")
    w = eng.read_records()
    still = (w >> 17) < 128
    assert still.any() and np.array_equal(still, live)  # eight unconsidered votes conclude nothing
    assert not ((w[still] >> 8) & 0xFF).any()  # every live record's consider byte is 0
    assert not (w[still] & 0xFF).any()
    assert eng.lost_responses() == n * k
    eng.close()


def test_target_shards_agree(oracle):
    n, m, k = 64, 96, 8
    thr = L.threshold(0.25)
    whole = avhip.Engine(n, m, k=k, seed=SEED)
    parts = [avhip.Engine(n, m, k=k, seed=SEED, target_range=r) for r in ((0, 64), (64, 96))]
    for e in [whole] + parts:
        e.init_records(avhip.INIT_BERNOULLI, P80)
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
    assert sum(e.applied_votes() for e in parts) == whole.applied_votes()
    assert whole.finalized_count() > 0
    for e in [whole] + parts:
        e.close()


def unchanged_after(eng, call):
    rec, rnd = eng.read_records(), eng.round
    with pytest.raises(avhip.AvError) as ei:
        call()
    assert ei.value.code == AV_ERR_UNSUPPORTED
    np.testing.assert_array_equal(eng.read_records(), rec)
    assert eng.round == rnd


def test_unsupported_combinations():
    capped = avhip.Engine(64, 4200, k=8, seed=SEED)
    capped.init_records(avhip.INIT_BERNOULLI, P80)
    capped.run_rounds(2)
    capped.set_loss(L.threshold(0.1))
    unchanged_after(capped, lambda: capped.run_rounds(1))
    assert "4096" in str(avhip.lib().av_last_error())
    capped.set_loss(0)
    capped.run_rounds(1)  # and the engine goes on once loss is off
    assert capped.round == 3
    capped.close()

    readd = avhip.Engine(32, 40, k=8, seed=SEED)
    readd.init_records(avhip.INIT_BERNOULLI, P80)
    readd.set_option("responder", 2)
    readd.set_responding([5], 0)
    unchanged_after(readd, lambda: readd.run_rounds(1))
    assert "responder" in str(avhip.lib().av_last_error())
    readd.set_option("responder", 1)  # IsAccepted literally runs
    readd.run_rounds(1)
    assert readd.round == 1 and readd.lost_responses() > 0
    readd.close()

    group = [avhip.Engine(64, 40, k=8, seed=SEED, node_range=r) for r in ((0, 32), (32, 64))]
    for e in group:
        e.init_records(avhip.INIT_BERNOULLI, P80)
    group[1].set_loss(L.threshold(0.1))
    with pytest.raises(avhip.AvError) as ei:  # a lossy engine cannot join
        avhip.peer_group_serial(group)
    assert ei.value.code == AV_ERR_UNSUPPORTED
    group[1].set_loss(0)
    avhip.peer_group_serial(group)
    unchanged_after(group[0], lambda: group[0].set_loss(L.threshold(0.1)))
    unchanged_after(group[0], lambda: group[0].set_responding([40], 0))
    group[0].set_loss(0, L.NEUTRAL)  # nothing lost: allowed
    group[0].set_responding([40], 1)
    avhip.run_group_rounds(group, 2)
    assert group[0].round == 2 and group[1].round == 2
    for e in group:  # (closing one member closes the whole group; the others' close is then a no-op)
        e.close()


def test_cpp_mirror_lossy():
    """Engine::SetLoss / SetResponding of the C++ mirror (host/avalanche_lossy_tests.cpp)."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-avalanche_amd", "bin",
                       "avalanche_lossy_tests")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS Lossy" in r.stdout, r.stdout + r.stderr
