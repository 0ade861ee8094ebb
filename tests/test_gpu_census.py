"""Network census on the device (av_census, census.hip): per-target class and
count sums, per-node class counts and the count histogram in one pass over the
A and K planes. Every comparison is exact equality with the numpy reference
(census_ref.py) applied to the engine's own read_records() and, where a network
runs, to the oracle's dump."""
import numpy as np
import pytest

import avhip
from census_ref import census_from_words, check_identities

pytestmark = pytest.mark.gpu

P97 = int(0.97 * 2**32)
BYZ20 = int(0.2 * 2**32)
KEYS = ("target_classes", "target_count_sum", "node_classes", "count_hist")
# census.hip kCensusFlush: tiles a lane accumulates in its register counters (7 tiles per 3-plane
# level-1 counter x 36 spills into the 8-plane level-2 counter) before it flushes them to LDS
FLUSH_TILES = 252


def same(got, exp, where):
    assert sorted(got) == sorted(exp), where
    for k in exp:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (where, k)
        if not np.array_equal(got[k], exp[k]):
            bad = np.argwhere(got[k] != exp[k])[:5].tolist()
            raise AssertionError(f"{where}: {k} differs at {bad}: "
                                 f"{[(int(got[k][tuple(i)]), int(exp[k][tuple(i)])) for i in bad]}")


def check(eng, where, sim=None, honest_only=False, mask=None, **kw):
    got = eng.census(honest_only=honest_only, **kw)
    words = eng.read_records()
    same(got, census_from_words(words, mask), f"{where} (read_records)")
    if sim is not None:
        same(got, census_from_words(sim.dump(), mask), f"{where} (oracle)")
    n = words.shape[0] if mask is None else int(mask.sum())
    check_identities(got, n, words.shape[1], mask)
    return got


def random_words(rng, n, m):
    """Canonical words in every form: both absent forms; live records with every count 0..127,
    both accepted bits, arbitrary vote and consider registers."""
    count = rng.integers(0, 128, size=(n, m)).astype(np.uint32)
    a = rng.integers(0, 2, size=(n, m)).astype(np.uint32)
    vc = rng.integers(0, 1 << 16, size=(n, m)).astype(np.uint32)
    live = vc | (((count << np.uint32(1)) | a) << np.uint32(16))
    absent = np.uint32(0xFFFE0000) | (a << np.uint32(16))
    w = np.where(rng.random((n, m)) < 0.3, absent, live).astype(np.uint32)
    # every (accepted, count) pair at least once, at scattered places
    at = rng.choice(n * m, size=256, replace=False)
    w.reshape(-1)[at] = np.uint32(0x5AA5) | (np.arange(256, dtype=np.uint32) << np.uint32(16))
    return w


LIFE_ROUNDS = (0, 1, 2, 5, 10, 15, 20, 25, 30)
SHAPES = [
    (200, 1000),  # BL 32, ragged last block
    (500, 256),   # BL 8
    (37, 33),     # BL 2, one target in the last block, 74 lanes: not a tile multiple
    (64, 20),     # BL 1
    (70, 2100),   # BL 66: does not divide 64 and is larger
    (64, 4200),   # capped engine
]


@pytest.mark.parametrize("n,m", SHAPES, ids=lambda v: str(v))
def test_census_through_a_networks_life(oracle, n, m):
    """Fresh round (virtual K4..K7), the deferred stretch, finalization."""
    eng = avhip.Engine(n, m, k=8, seed=11, log_capacity=1 << 23)
    eng.init_records(3, P97)
    sim = oracle.Sim(n, m, 8, seed=11, init_mode=3, init_param=P97)
    done = 0
    for r in LIFE_ROUNDS:
        eng.run_rounds(r - done)
        for _ in range(r - done):
            sim.run_round()
        done = r
        eng.discard_updates()
        c = check(eng, f"after {r} rounds", sim)
    assert c["target_classes"][:, 2:].sum() > 0, "no record finalized: the run does not reach finalization"
    eng.close()


def test_census_validity_flip_in_deferred_stretch(oracle):
    """Pending count steps apply to the valid records only; validity itself changes no class."""
    n, m = 200, 1000
    eng = avhip.Engine(n, m, k=8, seed=3, log_capacity=1 << 23)
    eng.init_records(3, P97)
    sim = oracle.Sim(n, m, 8, seed=3, init_mode=3, init_param=P97)
    for r in range(14):
        if r == 9:
            eng.set_valid(m - 1, False)
            sim.set_valid(m - 1, False)
        if r == 12:
            eng.set_valid(m - 1, True)
            sim.set_valid(m - 1, True)
        if r >= 8:
            check(eng, f"before round {r}", sim)
        eng.run_rounds(1)
        sim.run_round()
        eng.discard_updates()
        if r >= 8:
            check(eng, f"after round {r}", sim)
    eng.close()


@pytest.mark.parametrize("n,m", [(130, 100), (37, 33)], ids=lambda v: str(v))
def test_census_arbitrary_state(n, m):
    rng = np.random.default_rng(n * 1000 + m)
    words = random_words(rng, n, m)
    ref = census_from_words(words)
    assert (ref["count_hist"] > 0).all(), "the written state does not hit every histogram bin"
    assert (ref["target_classes"].sum(axis=0) > 0).all(), "the written state misses a class"
    eng = avhip.Engine(n, m, k=8, seed=1)
    eng.write_records(words)
    assert np.array_equal(eng.read_records(), words)
    same(check(eng, "written words"), ref, "written words (as written)")
    eng.close()


def test_census_subranges_and_shards(oracle):
    n, m = 130, 100
    rng = np.random.default_rng(5)
    words = random_words(rng, n, m)
    eng = avhip.Engine(n, m, k=8, seed=1)
    eng.write_records(words)
    full = eng.census()
    for n0, n1 in ((3, 67), (64, 65), (5, 5)):
        got = eng.census(n0, n1)
        same(got, census_from_words(words[n0:n1]), f"nodes [{n0}, {n1})")
        same(got, census_from_words(eng.read_records(n0, n1)), f"nodes [{n0}, {n1}) (read_records)")
    eng.close()

    # a node shard: its counts add to the other shard's
    parts = []
    for rng_ in ((0, 40), (40, 130)):
        e = avhip.Engine(n, m, k=8, seed=1, node_range=rng_)
        e.write_records(words[rng_[0]:rng_[1]])
        got = e.census()
        same(got, census_from_words(words[rng_[0]:rng_[1]]), f"node shard {rng_}")
        same(got, census_from_words(e.read_records()), f"node shard {rng_} (read_records)")
        parts.append(got)
        e.close()
    for k in ("target_classes", "target_count_sum", "count_hist"):
        assert np.array_equal(parts[0][k] + parts[1][k], full[k]), k
    assert np.array_equal(np.concatenate([p["node_classes"] for p in parts]), full["node_classes"])

    # a target shard of a running network: its rows are the full network's rows of those targets
    t0, t1 = 32, 96
    e = avhip.Engine(n, m, k=8, seed=9, target_range=(t0, t1), log_capacity=1 << 22)
    e.init_records(3, P97)
    sim = oracle.Sim(n, m, 8, seed=9, init_mode=3, init_param=P97)
    for r in (0, 6, 22):
        while sim.round < r:
            sim.run_round()
            e.run_rounds(1)
        e.discard_updates()
        got = e.census()
        same(got, census_from_words(e.read_records()), f"target shard, round {r} (read_records)")
        same(got, census_from_words(sim.dump()[:, t0:t1]), f"target shard, round {r} (oracle)")
        check_identities(got, n, t1 - t0)
    e.close()


def test_census_byzantine(oracle):
    n, m = 300, 200
    eng = avhip.Engine(n, m, k=8, seed=17, byz_threshold=BYZ20, log_capacity=1 << 23)
    eng.init_records(3, P97)
    sim = oracle.Sim(n, m, 8, seed=17, byz_threshold=BYZ20, init_mode=3, init_param=P97)
    honest = np.array([not sim.is_byzantine(j) for j in range(n)])
    assert 0 < honest.sum() < n
    done = 0
    for r in (0, 5, 12):
        eng.run_rounds(r - done)
        for _ in range(r - done):
            sim.run_round()
        done = r
        eng.discard_updates()
        check(eng, f"round {r}, all nodes", sim)
        got = check(eng, f"round {r}, honest only", sim, honest_only=True, mask=honest)
        assert not got["node_classes"][~honest].any()
    eng.close()


def test_census_flush_period():
    """One workgroup walks the whole network: each of its four waves accumulates more than three
    flush periods per lane (m = 64: two blocks per node, a lane's block never changes)."""
    m = 64
    tiles = 4 * (3 * FLUSH_TILES + 25)  # per wave: three full periods and a partial one
    n = tiles * 64 // 2 - 7             # the last tile is ragged
    rng = np.random.default_rng(252)
    words = random_words(rng, n, m)
    ref = census_from_words(words)
    eng = avhip.Engine(n, m, k=8, seed=1)
    eng.write_records(words)
    dflt = eng.census()
    eng.set_option("census_blocks", 1)
    one = eng.census()
    eng.set_option("census_blocks", 3)
    three = eng.census()
    eng.set_option("census_blocks", 0)
    same(one, ref, "one workgroup")
    same(three, ref, "three workgroups")
    same(dflt, ref, "default grid")
    eng.close()


def test_census_leaves_fast_paths_on():
    """A census after every round changes nothing a run without it produces, and leaves the
    deferred forms in place: the bytes the rounds move are the same."""
    n, m = 20_000, 1000
    out = []
    for census in (True, False):
        e = avhip.Engine(n, m, k=8, seed=0xA7A1A9C4, log_capacity=1 << 24)
        e.init_records(3, P97)
        for _ in range(24):
            e.run_rounds(1)
            if census:
                c = e.census()
        out.append((e.alg_bytes(), e.fetch_updates(), e.read_records()))
        e.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])
    check_identities(c, n, m)


def test_census_null_combinations_and_errors():
    n, m = 130, 100
    rng = np.random.default_rng(8)
    eng = avhip.Engine(n, m, k=8, seed=1)
    eng.write_records(random_words(rng, n, m))
    full = eng.census()
    flags = ("targets", "count_sum", "nodes", "hist")
    for flag, key in zip(flags, KEYS):
        got = eng.census(**{f: f == flag for f in flags})
        assert list(got) == [key]
        assert np.array_equal(got[key], full[key]), key
    pair = eng.census(targets=False, nodes=False)
    assert sorted(pair) == ["count_hist", "target_count_sum"]
    for k in pair:
        assert np.array_equal(pair[k], full[k]), k

    L = avhip.lib()
    with pytest.raises(avhip.AvError) as err:  # all four pointers NULL
        eng.census(targets=False, count_sum=False, nodes=False, hist=False)
    assert err.value.code == avhip.AV_ERR_INVALID_ARG
    assert L.av_census(eng._h, 0, n, 0, None) == avhip.AV_ERR_INVALID_ARG  # out NULL
    for n0, n1 in ((-1, 5), (0, n + 1), (7, 3)):
        with pytest.raises(avhip.AvError) as err:
            eng.census(n0, n1)
        assert err.value.code == avhip.AV_ERR_INVALID_ARG
    empty = eng.census(5, 5)  # n0 == n1: zeros
    assert empty["node_classes"].shape == (0, 4)
    assert not any(empty[k].any() for k in KEYS)
    eng.close()
    shard = avhip.Engine(n, m, k=8, seed=1, node_range=(40, 130))
    with pytest.raises(avhip.AvError):
        shard.census(39, 50)
    shard.close()
