"""AddTargetToReconcile for many Processors at once (processor.go:45-58):
av_admit_targets (every node of a range adds a list of targets, as every node
does when a transaction appears, main.go:97-103) and av_add_targets_batch (many
Processors' lists in one call). Checked against the oracle's Sim.add looped
over nodes and targets: the created records, the published rows, the rounds
that follow and the counters."""
import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)
AV_ERR_INVALID_ARG, AV_ERR_UNSUPPORTED = -1, -6
ABSENT = avhip.ABSENT_WORD


def rows(u):
    return [tuple(int(v) for v in r) for r in np.asarray(u).tolist()]


def checkerboard(n, m, seed):
    """Live words, absent records with decision 0 and absent records with decision 1."""
    rng = np.random.default_rng(seed)
    votes = rng.integers(0, 256, (n, m)).astype(np.uint32)
    cons = rng.integers(0, 256, (n, m)).astype(np.uint32)
    conf = rng.integers(0, 2 * 100, (n, m)).astype(np.uint32)
    live = votes | (cons << np.uint32(8)) | (conf << np.uint32(16))
    kind = (np.arange(n)[:, None] + np.arange(m)[None, :]) % 3
    return np.where(kind == 0, live, np.where(kind == 1, np.uint32(ABSENT), np.uint32(ABSENT | (1 << 16)))).astype(np.uint32)


def init_bits(oracle, n, m, seed, byz, mode, param):
    """The acceptance av_init_records gives every (node, target): bit 16 of a fresh oracle network."""
    fresh = oracle.Sim(n, m, 8, seed=seed, byz_threshold=byz, init_mode=mode, init_param=param)
    bits = (fresh.dump() >> 16) & 1
    fresh.close()
    return bits


def oracle_admit(sim, targets, nodes, acc_of):
    """Sim.add for every node and target, in list order; the column sums of its returns."""
    added = np.zeros(len(targets), np.int64)
    for i, t in enumerate(targets):
        if not 0 <= t < sim.m:
            continue  # an unknown hash: skipped
        for j in nodes:
            added[i] += sim.add(j, t, acc_of(j, t, i))
    return added


def byz_rows(sim):
    return np.array([sim.is_byzantine(j) for j in range(sim.n)], bool)


def same_pref(eng, sim, byz):
    """Honest rows are the oracle's; a Byzantine node publishes its flip-flop row whatever it holds."""
    got, exp = eng.read_pref(), sim.pref()
    np.testing.assert_array_equal(got[~byz], exp[~byz])
    flip = (1 - ((np.arange(sim.m) ^ eng.round) & 1)).astype(np.uint8)
    np.testing.assert_array_equal(got[byz], np.broadcast_to(flip, (int(byz.sum()), sim.m)))


RAGGED_LIST = [0, 37, -1, 75, 10, 33, 10, 64, 69, 5, 40, 31, 32]
RAGGED_ACC = [1, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0]  # target 10 twice, accepted then rejected


@pytest.mark.parametrize("amap", [1, 2], ids=["block_major", "lane_major"])
@pytest.mark.parametrize("rng_", [(3, 97), (0, 0)], ids=["sub_range", "whole_shard"])
@pytest.mark.parametrize("mode", [avhip.INIT_GIVEN, avhip.INIT_BERNOULLI, avhip.INIT_PAIRS],
                         ids=["given", "bernoulli", "pairs"])
def test_admit_parity_ragged(oracle, mode, rng_, amap):
    """130 x 70 (lanes straddle a 64-lane tile, three blocks with a partial last one, a lane count that
    is no multiple of 64) over a checkerboard of live and absent records, one invalid target, Byzantine
    nodes; the list holds live, invalid, unknown and repeated targets in all three blocks. Both thread
    mappings."""
    n, m, seed = 130, 70, 11
    param = P80 if mode == avhip.INIT_BERNOULLI else 0
    eng = avhip.Engine(n, m, k=8, seed=seed, byz_threshold=BYZ20)
    eng.set_option("admit_map", amap)
    sim = oracle.Sim(n, m, 8, seed=seed, byz_threshold=BYZ20, init_mode=avhip.INIT_NONE)
    byz = byz_rows(sim)
    assert byz.any() and not byz.all()
    words = checkerboard(n, m, 5)
    eng.write_records(words)
    sim.write_records(words)
    eng.set_valid(37, False)
    sim.set_valid(37, False)
    assert m + 5 == RAGGED_LIST[3]
    if mode == avhip.INIT_GIVEN:
        acc_of = lambda j, t, i: RAGGED_ACC[i]
    else:
        bits = init_bits(oracle, n, m, seed, BYZ20, mode, param)
        acc_of = lambda j, t, i: int(bits[j, t])
    nodes = range(*rng_) if rng_ != (0, 0) else range(n)
    got = eng.admit_targets(RAGGED_LIST, mode, param, RAGGED_ACC if mode == avhip.INIT_GIVEN else None, *rng_)
    exp = oracle_admit(sim, RAGGED_LIST, nodes, acc_of)
    print("added_nodes", got.tolist())
    assert got.tolist() == exp.tolist()
    assert exp[1] == 0 and exp[2] == 0 and exp[3] == 0 and exp[6] == 0 and exp[4] > 0
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    same_pref(eng, sim, byz)
    for r in range(4):
        eng.run_rounds(1)
        e_exp, _ = sim.run_round()
        assert rows(eng.fetch_updates()) == rows(e_exp), f"round {r}"
        np.testing.assert_array_equal(eng.read_records(), sim.dump(), err_msg=f"round {r}")
    eng.close()


@pytest.mark.parametrize("c_preset", [0, 1])
@pytest.mark.parametrize("mode", [avhip.INIT_BERNOULLI, avhip.INIT_PAIRS], ids=["bernoulli", "pairs"])
def test_admit_equals_init(mode, c_preset):
    """Admitting every target to an empty engine leaves what av_init_records leaves: records, published
    words and the rounds after (the twin's consider planes preset or stored)."""
    n, m, seed = 200, 1000, 3
    param = P80 if mode == avhip.INIT_BERNOULLI else 0
    eng = avhip.Engine(n, m, k=8, seed=seed, byz_threshold=BYZ20, log_capacity=1 << 22)
    twin = avhip.Engine(n, m, k=8, seed=seed, byz_threshold=BYZ20, log_capacity=1 << 22)
    twin.set_option("c_preset", c_preset)
    twin.init_records(mode, param)
    got = eng.admit_targets(np.arange(m), mode, param)
    assert got.tolist() == [n] * m
    np.testing.assert_array_equal(eng.read_records(), twin.read_records())
    np.testing.assert_array_equal(eng.read_pref_words(), twin.read_pref_words())
    for r in range(3):
        eng.run_rounds(1)
        twin.run_rounds(1)
        np.testing.assert_array_equal(eng.fetch_updates(), twin.fetch_updates(), err_msg=f"round {r}")
    np.testing.assert_array_equal(eng.read_records(), twin.read_records())
    np.testing.assert_array_equal(eng.read_pref_words(), twin.read_pref_words())
    eng.close()
    twin.close()


@pytest.mark.parametrize("whole", [False, True], ids=["node_11", "every_node"])
def test_admit_inside_deferred_stretch(oracle, whole):
    """The shape and schedule of test_quiet_tiles_add_targets_midrun and
    test_uniform_rows_add_targets_midrun: dead records re-admitted as rejected at round 20, inside the
    quiescent stretch (the write-back before the admission and the plan facts after it)."""
    n, m = 1200, 256
    eng = avhip.Engine(n, m, k=8, seed=7, log_capacity=1 << 24)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    sim = oracle.Sim(n, m, 8, seed=7, init_mode=avhip.INIT_ACCEPTED, init_param=0, threads=4)
    for r in range(24):
        if r == 20:  # every record finalized by now
            nodes = range(n) if whole else range(11, 12)
            got = eng.admit_targets([4, 5, 200], avhip.INIT_REJECTED, 0, None, *((0, 0) if whole else (11, 12)))
            exp = oracle_admit(sim, [4, 5, 200], nodes, lambda j, t, i: 0)
            assert got.tolist() == exp.tolist() == [len(nodes)] * 3
        eng.run_rounds(1)
        e_exp, _ = sim.run_round(threads=4)
        assert rows(eng.fetch_updates()) == rows(e_exp), f"round {r}"
    np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=4))
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


def test_admit_slot_reuse(oracle):
    """The streaming life: every record finalizes and is deleted (processor.go:114-116), then every
    node adds every target again (:50-53 tests only the map) and the network runs on."""
    n, m, seed = 200, 64, 13
    eng = avhip.Engine(n, m, k=1, seed=seed, log_capacity=1 << 22)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    sim = oracle.Sim(n, m, 1, seed=seed, init_mode=avhip.INIT_ACCEPTED, init_param=0)
    for r in range(160):
        if eng.finalized_count() == n * m:
            break
        eng.run_rounds(1)
        eng.discard_updates()
        sim.run_round(collect=False)
    else:
        pytest.fail(f"not every record finalized in 160 rounds ({eng.finalized_count()} of {n * m})")
    print("rounds to finalization:", r)
    assert eng.live_records() == 0
    bits = init_bits(oracle, n, m, seed, 0, avhip.INIT_BERNOULLI, P80)
    got = eng.admit_targets(np.arange(m), avhip.INIT_BERNOULLI, P80)
    exp = oracle_admit(sim, list(range(m)), range(n), lambda j, t, i: int(bits[j, t]))
    assert got.tolist() == exp.tolist() == [n] * m
    assert eng.live_records() == n * m
    for r in range(30):
        eng.run_rounds(1)
        e_exp, _ = sim.run_round()
        assert rows(eng.fetch_updates()) == rows(e_exp), f"round {r}"
        dump = sim.dump()
        np.testing.assert_array_equal(eng.read_records(), dump, err_msg=f"round {r}")
        live = (dump >> 17) < avhip.FINALIZATION_SCORE
        assert eng.live_records() == int(live.sum())
        cls = eng.census(count_sum=False, nodes=False, hist=False)["target_classes"]
        assert (cls.sum(axis=1) == n).all()
        acc = ((dump >> 16) & 1).astype(bool)
        np.testing.assert_array_equal(cls[:, avhip.CENSUS_LIVE_ACCEPTED], (live & acc).sum(axis=0))
        np.testing.assert_array_equal(cls[:, avhip.CENSUS_LIVE_REJECTED], (live & ~acc).sum(axis=0))
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


def random_csr(rng, n, m, n_req):
    """Repeated nodes, unsorted targets, repeats within and across a node's requests with differing
    accepted bits, foreign targets, empty requests."""
    nodes = rng.integers(0, max(2, n // 4), n_req) * 3 % n
    lens = rng.integers(0, 12, n_req)
    lens[rng.integers(0, n_req, 3)] = 0
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    targets = rng.integers(-2, m + 3, offsets[-1])
    accepted = rng.integers(0, 2, offsets[-1]).astype(np.uint8)
    return nodes.astype(np.int64), offsets, targets.astype(np.int64), accepted


def ascending_csr(rng, n, m, n_req):
    nodes = rng.permutation(n)[:n_req].astype(np.int64)
    reqs = [np.sort(rng.choice(m, rng.integers(1, 20), replace=False)) for _ in range(n_req)]
    offsets = np.concatenate([[0], np.cumsum([len(q) for q in reqs])]).astype(np.int64)
    targets = np.concatenate(reqs).astype(np.int64)
    return nodes, offsets, targets, rng.integers(0, 2, targets.size).astype(np.uint8)


@pytest.mark.parametrize("case", ["random", "ascending", "empty"])
def test_add_targets_batch(oracle, case):
    """The batch against a twin engine fed one av_add_targets per request, and against the oracle."""
    n, m, seed = 50, 70, 21
    rng = np.random.default_rng(17)
    if case == "random":
        nodes, offsets, targets, accepted = random_csr(rng, n, m, 60)
        assert len(set(nodes.tolist())) < len(nodes) and (np.diff(offsets) == 0).any()
        assert ((targets < 0) | (targets >= m)).any()
    elif case == "ascending":
        nodes, offsets, targets, accepted = ascending_csr(rng, n, m, 30)
    else:
        nodes, offsets, targets, accepted = (np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64),
                                             np.zeros(0, np.uint8))
    eng = avhip.Engine(n, m, k=8, seed=seed)
    twin = avhip.Engine(n, m, k=8, seed=seed)
    sim = oracle.Sim(n, m, 8, seed=seed, init_mode=avhip.INIT_NONE)
    words = checkerboard(n, m, 9)
    for x in (eng, twin, sim):
        x.write_records(words)
        x.set_valid(41, False)
    got = eng.add_targets_batch(nodes, offsets, targets, accepted)
    seq, exp = [], []
    for r, node in enumerate(nodes.tolist()):
        lo, hi = offsets[r], offsets[r + 1]
        seq += twin.add_targets(node, targets[lo:hi], accepted[lo:hi]).tolist()
        exp += [0 <= t < m and sim.add(node, t, a) for t, a in zip(targets[lo:hi].tolist(), accepted[lo:hi].tolist())]
    assert got.dtype == np.bool_ and got.tolist() == seq == exp
    if case != "empty":
        assert any(exp) and not all(exp)
    np.testing.assert_array_equal(eng.read_records(), twin.read_records())
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    np.testing.assert_array_equal(eng.read_pref(), twin.read_pref())
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()
    twin.close()


def test_admit_shards():
    """Target shards split at 32 of 70: per position exactly one shard reports, and together they are
    the unsharded engine. Node shards without an exchange: the counts add, the records concatenate."""
    n, m, seed = 130, 70, 11
    words = checkerboard(n, m, 5)
    lst = [0, 37, -1, 75, 10, 33, 10, 64, 69, 5, 40, 31, 32]
    full = avhip.Engine(n, m, k=8, seed=seed)
    full.write_records(words)
    full.set_valid(37, False)
    exp = full.admit_targets(lst, avhip.INIT_BERNOULLI, P80)
    exp_rec, exp_pref = full.read_records(), full.read_pref()
    full.close()
    assert (exp > 0).sum() >= 8

    parts = [avhip.Engine(n, m, k=8, seed=seed, target_range=r) for r in ((0, 32), (32, 70))]
    got = []
    for e in parts:
        e.write_records(words[:, e.target_range[0]:e.target_range[1]])
        e.set_valid(37, False)
        got.append(e.admit_targets(lst, avhip.INIT_BERNOULLI, P80))
    assert not ((got[0] != 0) & (got[1] != 0)).any()
    assert (got[0] + got[1]).tolist() == exp.tolist()
    np.testing.assert_array_equal(np.concatenate([e.read_records() for e in parts], axis=1), exp_rec)
    np.testing.assert_array_equal(np.concatenate([e.read_pref() for e in parts], axis=1), exp_pref)
    for e in parts:
        e.close()

    parts = [avhip.Engine(n, m, k=8, seed=seed, node_range=r) for r in ((0, 60), (60, 130))]
    got = []
    for e in parts:
        e.write_records(words[e.node_range[0]:e.node_range[1]])
        e.set_valid(37, False)
        got.append(e.admit_targets(lst, avhip.INIT_BERNOULLI, P80))
    assert (got[0] + got[1]).tolist() == exp.tolist()
    np.testing.assert_array_equal(np.concatenate([e.read_records() for e in parts]), exp_rec)
    np.testing.assert_array_equal(np.concatenate([e.read_pref(*e.node_range) for e in parts]), exp_pref)
    for e in parts:
        e.close()


def code_of(fn):
    with pytest.raises(avhip.AvError) as ei:
        fn()
    return ei.value.code


def test_admit_refusals():
    n, m = 64, 70
    engs = [avhip.Engine(n, m, k=8, seed=11, node_range=(r * 32, (r + 1) * 32)) for r in range(2)]
    for e in engs:
        e.init_records(avhip.INIT_ACCEPTED, 0)
    avhip.peer_group_serial(engs)
    for e in engs:
        lo = e.node_range[0]
        assert code_of(lambda: e.admit_targets([1, 2], avhip.INIT_ACCEPTED)) == AV_ERR_UNSUPPORTED
        assert code_of(lambda: e.add_targets_batch([lo], [0, 1], [3], [1])) == AV_ERR_UNSUPPORTED
    engs[0].close()

    e = avhip.Engine(n, m, k=8, seed=11, node_range=(8, 40))
    before = e.read_records()
    bad = AV_ERR_INVALID_ARG
    assert code_of(lambda: e.admit_targets([1], avhip.INIT_ACCEPTED, n0=20, n1=12)) == bad       # n0 > n1
    assert code_of(lambda: e.admit_targets([1], avhip.INIT_ACCEPTED, n0=4, n1=12)) == bad        # outside the shard
    assert code_of(lambda: e.admit_targets([1], avhip.INIT_ACCEPTED, n0=12, n1=41)) == bad
    assert code_of(lambda: e.admit_targets([1], avhip.INIT_NONE)) == bad
    assert code_of(lambda: e.admit_targets([1], 6)) == bad
    assert code_of(lambda: e.admit_targets([1], avhip.INIT_GIVEN, accepted=None)) == bad
    assert code_of(lambda: e.add_targets_batch([9, 10], [1, 1, 2], [3, 4], [1, 1])) == bad      # offsets[0] != 0
    assert code_of(lambda: e.add_targets_batch([9, 10], [0, 2, 1], [3, 4], [1, 1])) == bad      # a decreasing offset
    assert code_of(lambda: e.add_targets_batch([9, 40], [0, 1, 2], [3, 4], [1, 1])) == bad      # a foreign node
    assert code_of(lambda: e.init_records(avhip.INIT_GIVEN, 0)) == bad
    np.testing.assert_array_equal(e.read_records(), before)
    # and the calls still work on this engine
    assert e.admit_targets([1, 1], avhip.INIT_GIVEN, accepted=[1, 0], n0=8, n1=10).tolist() == [2, 0]
    assert e.add_targets_batch([9, 10], [0, 1, 2], [1, 1], [1, 1]).tolist() == [False, True]
    e.close()


def test_cpp_mirror_admit_all():
    """Engine::AddTargetToReconcileAll of the C++ mirror (host/avalanche_admit_tests.cpp)."""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-avalanche_amd", "bin",
                       "avalanche_admit_tests")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS AdmitAll" in r.stdout, r.stdout + r.stderr
