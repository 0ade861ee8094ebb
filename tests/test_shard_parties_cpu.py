"""shard_parties.py and the sharded lives' geometry, checked on the CPU: every merge against a
direct numpy computation on small random data, the refusals the parties rely on (an unordered
part, a vote claimed twice), the shard shapes the 32 seeds give, and the peer-group schedules
(life_schedule.restrict) replayed on the oracle alone: they still end at the schedule's round, and
every round flagged taken still sits in a settled stretch."""
import numpy as np
import pytest

import life_schedule as ls
import shard_parties as sp
from avhip import sharding
from census_ref import census_from_words
from test_life_schedule_cpu import replay

RANGES = [(0, 32), (32, 96), (96, 128), (128, 129)]  # the last shard holds one target


def random_rows(rng, n, targets):
    """n distinct update rows in canonical order with targets from `targets`."""
    keys = set()
    while len(keys) < n:
        keys.add((int(rng.integers(0, 5)), int(rng.integers(0, 40)), int(rng.integers(0, 8)), int(rng.choice(targets))))
    rows = np.array(sorted(keys), np.int64).reshape(-1, 4)
    return np.concatenate([rows, rng.integers(0, 4, size=(len(rows), 1))], axis=1)


def by_target(rows, ranges):
    return [rows[(rows[:, 3] >= a) & (rows[:, 3] < b)] for a, b in ranges]


# ---- the merges
def test_merge_updates_is_lexsort_of_the_concatenation():
    rng = np.random.default_rng(1)
    rows = random_rows(rng, 300, np.arange(129))
    parts = by_target(rows, RANGES)
    assert all(len(p) for p in parts)
    cat = np.concatenate(parts)
    exp = cat[np.lexsort((cat[:, 3], cat[:, 2], cat[:, 1], cat[:, 0]))]
    assert np.array_equal(sp.merge_updates(parts), exp) and np.array_equal(exp, rows)
    assert np.array_equal(sp.merge_words([ls.pack_updates(p, 0) for p in parts]), ls.pack_updates(rows, 0))
    assert sp.merge_updates([rows[:0], rows[:0]]).shape == (0, 5) and sp.merge_words([]).size == 0


def test_merge_updates_refuses_an_unordered_part():
    rng = np.random.default_rng(2)
    rows = random_rows(rng, 60, np.arange(129))
    parts = by_target(rows, RANGES)
    swapped = parts[1].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(AssertionError, match="not strictly ascending"):
        sp.merge_updates([parts[0], swapped] + parts[2:])
    with pytest.raises(AssertionError, match="not strictly ascending"):
        sp.merge_words([ls.pack_updates(swapped, 0)])
    with pytest.raises(AssertionError, match="not strictly ascending"):  # an update twice in one part
        sp.merge_updates([np.concatenate([parts[0][:1], parts[0]])])
    with pytest.raises(AssertionError, match="two parts"):  # one (round, node, slot, target) on two shards
        sp.merge_updates([parts[0], parts[0][:1]])


def test_merge_statuses_and_added():
    rng = np.random.default_rng(3)
    owner = rng.integers(-1, 3, size=50)  # -1: no shard gives the vote a status
    value = rng.integers(0, 4, size=50)
    parts = [np.where(owner == g, value, -1).astype(np.int32) for g in range(3)]
    assert np.array_equal(sp.merge_statuses(parts), np.where(owner >= 0, value, -1))
    assert np.array_equal(sp.merge_added([owner == g for g in range(3)]), owner >= 0)
    twice = [p.copy() for p in parts]
    twice[0][7] = twice[2][7] = 0
    with pytest.raises(AssertionError, match="two shards"):
        sp.merge_statuses(twice)
    with pytest.raises(AssertionError, match="two shards"):
        sp.merge_added([owner >= 0, owner == 0])
    with pytest.raises(AssertionError):
        sp.merge_statuses([np.array([-2], np.int32)])


def test_merge_digests_is_the_digest_of_the_union(oracle):
    rng = np.random.default_rng(4)
    rows = random_rows(rng, 500, np.arange(129))
    words = ls.pack_updates(rows, 0)
    parts = [oracle.update_digest(ls.pack_updates(p, 0)) for p in by_target(rows, RANGES)]
    assert sp.merge_digests(parts) == oracle.update_digest(words)
    assert sp.merge_digests([((1 << 64) - 1, (1 << 64) - 1, 5), (2, 3, 5)]) == (1, 2, 0)  # mod 2^64
    assert sp.merge_digests([]) == (0, 0, 0) == oracle.update_digest(words[:0])


@pytest.mark.parametrize("start,width", [(0, 129), (0, 32), (5, 20), (32, 64), (31, 2), (90, 39), (128, 1), (100, 10)])
def test_split_reassembles(start, width):
    """Rectangles that start, end or lie wholly inside one shard, or outside all but one."""
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, size=(7, width), dtype=np.uint64).astype(np.uint32)
    pieces = sp.split_columns(start, words, RANGES)
    assert all(p.shape[1] > 0 and RANGES[g][0] <= t < t + p.shape[1] <= RANGES[g][1] for g, t, p in pieces)
    assert [t for _, t, _ in pieces] == sorted(t for _, t, _ in pieces) and pieces[0][1] == start
    assert np.array_equal(np.concatenate([p for _, _, p in pieces], axis=1), words)
    assert [g for g, _, _ in pieces] == [g for g, (a, b) in enumerate(RANGES) if a < start + width and b > start]
    errs = rng.integers(0, 4, size=(3, 8, width)).astype(np.uint32)  # the last axis of any array
    assert np.array_equal(np.concatenate([p for _, _, p in sp.split_columns(start, errs, RANGES)], axis=2), errs)
    rows = sp.split_rows(start, words.T, RANGES)
    assert [(g, t) for g, t, _ in rows] == [(g, t) for g, t, _ in pieces]
    assert np.array_equal(np.concatenate([p for _, _, p in rows]), words.T)


def test_split_outside_every_range():
    assert sp.split_columns(40, np.zeros((2, 5), np.uint32), [(0, 32)]) == []
    assert sp.split_rows(0, np.zeros((0, 5), np.uint32), RANGES) == []


def random_words(rng, n, m):
    count = rng.integers(0, 160, size=(n, m)).astype(np.uint32)  # >= 128: no record
    return (rng.integers(0, 1 << 16, size=(n, m)).astype(np.uint32) | (rng.integers(0, 2, size=(n, m)).astype(np.uint32) << 16) |
            (count << 17)).astype(np.uint32)


@pytest.mark.parametrize("honest", [False, True])
def test_census_merges(honest):
    rng = np.random.default_rng(6)
    words = random_words(rng, 24, 129)
    mask = rng.random(24) < 0.7 if honest else None
    whole = census_from_words(words, mask)
    cols = sp.merge_census_targets([census_from_words(words[:, a:b], mask) for a, b in RANGES])
    cuts = [(0, 6), (6, 7), (7, 24)]
    rows = sp.merge_census_nodes([census_from_words(words[a:b], None if mask is None else mask[a:b]) for a, b in cuts])
    for key in sp.CENSUS_KEYS:
        assert np.array_equal(cols[key], whole[key]), key
        assert np.array_equal(rows[key], whole[key]), key


def test_invs_merges():
    rng = np.random.default_rng(7)
    live = rng.random((9, 129)) < 0.4
    live[3] = False

    def csr(block, t0):
        rows = [np.flatnonzero(r) + t0 for r in block]
        return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32)

    whole = csr(live, 0)
    got = sp.merge_invs([csr(live[:, a:b], a) for a, b in RANGES])
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    got = sp.concat_invs([csr(live[a:b], 0) for a, b in [(0, 3), (3, 4), (4, 9)]])
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


# ---- geometry of the sharded lives
def test_target_shard_geometry():
    bls, counts, one_target = set(), {}, []
    for seed in range(ls.N_SEEDS):
        n, m = ls.seed_config(seed)[:2]
        ranges = ls.target_shards(seed)
        g = len(ranges)
        assert g == min((2, 3, 4, 8)[seed % 4], (m + 31) // 32)
        assert ranges == [sharding.target_shard(m, g, r) for r in range(g)]
        assert ranges[0][0] == 0 and ranges[-1][1] == m and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        assert all(a % 32 == 0 and a < b for a, b in ranges)
        bls.update((b - a + 31) // 32 for a, b in ranges)
        counts.setdefault((n, m), set()).add(g)
        if ranges[-1][1] - ranges[-1][0] == 1:
            one_target.append(seed)
    assert bls >= {1, 4, 16, 17, 18} and max(bls) == 18, bls
    assert one_target and all(ls.seed_config(s)[1] == 33 for s in one_target)
    for seed in (19, 23):  # the 8-GPU C4 decomposition
        shard_bls = [(b - a + 31) // 32 for a, b in ls.target_shards(seed)]
        assert len(shard_bls) == 8 and set(shard_bls) <= {4, 5} and 4 in shard_bls, (seed, shard_bls)
    assert [(b - a + 31) // 32 for a, b in ls.target_shards(23)] == [4] * 8
    assert [(b - a + 31) // 32 for a, b in ls.target_shards(8)] == [16, 16]  # the vv_min_bl boundary
    for seed in (4, 28):
        assert [(b - a + 31) // 32 for a, b in ls.target_shards(seed)] == [17, 18]
    assert all(len(gs) >= 3 for shape, gs in counts.items() if shape != (64, 33)), counts


def test_peer_world_geometry():
    none = [seed for seed in range(ls.N_SEEDS) if ls.peer_world(seed) is None]
    assert none == [seed for seed in range(ls.N_SEEDS) if ls.seed_config(seed)[0] == 67] and len(none) == 5
    worlds = set()
    for seed in range(ls.N_SEEDS):
        w = ls.peer_world(seed)
        if w is not None:
            assert w in (2, 4, 8) and ls.seed_config(seed)[0] % w == 0
            worlds.add(w)
    assert worlds == {2, 4, 8}


# ---- the peer-group schedules
def test_restrict_drops_only_the_named_steps():
    sched = ls.make_schedule(6)
    cut = ls.restrict(sched, ls.PEER_REFUSED)
    kept = [s for s in sched["steps"] if s["op"] not in ls.PEER_REFUSED]
    assert [ls.describe(s) for s in cut["steps"]] == [ls.describe(s) for s in kept]
    assert len(cut["steps"]) < len(sched["steps"]) and {k: v for k, v in cut.items() if k != "steps"} == \
        {k: v for k, v in sched.items() if k != "steps"}
    assert [ls.describe(s) for s in ls.make_schedule(6)["steps"]] == [ls.describe(s) for s in sched["steps"]]
    assert ls.restrict(sched, ())["steps"] == sched["steps"]


def test_restricted_schedules_replay_and_stay_settled(oracle):
    checked = dropped = lives = 0
    for seed in range(ls.N_SEEDS):
        if ls.peer_world(seed) is None:
            continue
        full = ls.make_schedule(seed)
        sched = ls.restrict(full, ls.PEER_REFUSED)
        assert not [s for s in sched["steps"] if s["op"] in ls.PEER_REFUSED]
        dropped += len(full["steps"]) - len(sched["steps"])
        state, life = replay(sched, oracle)
        assert life.sim.round == sched["rounds"], seed
        for step in sched["steps"]:
            if step["op"] == "rounds" and step["taken"]:
                assert step["c"] == 1 and sched["taken_seed"]
                for rr in (step["first"] - 2, step["first"] - 1, step["first"]):
                    same_rows, all_valid = state[rr]
                    assert same_rows and all_valid, f"seed {seed}: taken round {step['first']}, round {rr}: rows " \
                                                    f"identical {same_rows}, all valid {all_valid}"
                checked += 1
        lives += 1
    assert lives == 27 and dropped == 125 and checked >= 59, (lives, dropped, checked)
