"""The randomised engine lives of test_gpu_life_fuzz.py on sharded networks.

test_life_target_shards: every seed's schedule on 2, 3, 4 or 8 target shards
(life_schedule.target_shards: 1 to 18 blocks of 32 targets per shard, a last shard of one
target, 16 | 16, 17 | 18, eight shards of 4), presented to life_schedule.Life as one engine by
shard_parties.TargetShards. Every call takes global ids, so an engine that is off by its
target_begin anywhere (drop-in votes, add_targets, validity, cells, poll sets, rectangles,
replay slices, the compact header) differs from the oracle at that step.

test_life_target_shards_lossy: the lossy lives (life_schedule.make_lossy_schedule) on their target
shards; set_loss and set_responding go to every shard, and every shard must count the same lost
Responses.

test_life_peer_group: the schedules without the record writes a peer-push engine refuses, on
serial peer groups of 2, 4 or 8 ranks (shard_parties.PeerGroup) in the masked, full and direct
exchange modes: validity flips, materialize, option and kernel switches, re-inits and a replay
round between need-masked sweep rounds, observed in mid-life.

Both run the oracle, the party under test with the schedule's options and, in seeds with taken
rounds, a plain twin; in every taken round the tested party's shards together must move fewer
bytes than the twin's. No option of life_schedule.option_values is refused by a target shard or a
peer rank: a refusal (AvError from set_option) fails the life.

The directed cases pin what a shard does with targets that are not its own, what a peer rank
does with the calls it refuses, the full push that ends a non-sweep round of a masked group
whose rows are changing, and the device-generated replay stream on shards."""
import numpy as np
import pytest

import avhip
import life_schedule as ls
import shard_parties as sp

pytestmark = pytest.mark.gpu

# the exchange of a peer group, set on every rank of both parties before the group is made
EXCHANGE_MODES = [(), (("peer_mask", 0),), (), (("peer_mask", 0), ("push_defer", 0))]


def new_engine(sched, **shard):
    return avhip.Engine(sched["n"], sched["m"], k=sched["k"], seed=sched["engine_seed"], byz_threshold=sched["byz"],
                        log_capacity=ls.LOG_CAPACITY, **shard)


def run_life(oracle, sched, make_party, kind, first_options=()):
    """test_life_fuzz's loop over parties made by make_party()."""
    seed = sched["seed"]
    parties = {"test": make_party()}
    if sched["taken_seed"]:
        parties["twin"] = make_party()
    life = ls.Life(sched, oracle, parties, av=sp.PartyAv(avhip))
    life.post_init = {"twin": [("fresh", 0)]}  # av_init_records sets the fact again
    life.set_options("test", list(first_options) + list(sched["options"]))
    if "twin" in parties:
        life.set_options("twin", list(first_options) + ls.PLAIN_OPTIONS)
    for name, p in parties.items():
        p.init_records(sched["init_mode"], sched["init_param"])
        life.set_options(name, life.post_init.get(name, ()))
        if kind == "peer":
            p.group()
    checks = []
    for i, step in enumerate(sched["steps"]):
        life.apply(i, step)
        if step["op"] == "rounds" and step["taken"]:
            got, plain = life.deltas["test"], life.deltas["twin"]
            checks.append((step["first"], "".join(d[0] for d in step["deferrals"]), got, plain))
            assert got < plain, (f"{life.where}: no deferred form taken in round {step['first']}: {got} bytes, plain twin "
                                 f"{plain}; options {life.options['test']}")
    shape = [len(p.engines) for p in parties.values()]
    print(f"seed {seed} {kind} x{shape[0]} {sched['n']}x{sched['m']} k={sched['k']} taken (round, deferrals on, bytes, "
          f"twin bytes): {checks}")
    for name, p in parties.items():
        assert p.applied_votes() == life.applied, (seed, name, "applied_votes")
        assert p.finalized_count() == life.finalized, (seed, name, "finalized_count")
        assert p.round == sched["rounds"]
        assert p.lost_responses() == life.ref.lost, (seed, name, "lost_responses")
        p.close()


@pytest.mark.parametrize("seed", range(ls.N_SEEDS))
def test_life_target_shards(oracle, seed):
    sched = ls.make_schedule(seed)
    ranges = ls.target_shards(seed)
    run_life(oracle, sched, lambda: sp.TargetShards([new_engine(sched, target_range=r) for r in ranges], ranges, avhip),
             "target")


@pytest.mark.parametrize("seed", range(ls.N_LOSSY_SEEDS))
def test_life_target_shards_lossy(oracle, seed):
    """The lossy lives on target shards: every shard runs the whole network's loss (the draw depends on
    node, round and slot, and on the peer alone), so the shards' lost_responses must be equal."""
    sched = ls.make_lossy_schedule(seed)
    ranges = ls.target_shards(seed, sched["m"])
    run_life(oracle, sched, lambda: sp.TargetShards([new_engine(sched, target_range=r) for r in ranges], ranges, avhip),
             "lossy target")


@pytest.mark.parametrize("seed", [s for s in range(ls.N_SEEDS) if ls.peer_world(s) is not None])
def test_life_peer_group(oracle, seed):
    sched = ls.restrict(ls.make_schedule(seed), ls.PEER_REFUSED)
    world = ls.peer_world(seed)
    per = sched["n"] // world
    run_life(oracle, sched,
             lambda: sp.PeerGroup([new_engine(sched, node_range=(r * per, (r + 1) * per)) for r in range(world)], avhip),
             "peer", first_options=EXCHANGE_MODES[seed % 4])


# ---- directed cases
N, M, K, SEED = 40, 130, 8, 77


def test_foreign_targets_on_a_shard(oracle):
    t0, t1 = 32, 96
    e = avhip.Engine(N, M, k=K, seed=SEED, target_range=(t0, t1), log_capacity=ls.LOG_CAPACITY)
    e.init_records(avhip.INIT_BERNOULLI, ls.P80)
    sim = oracle.Sim(N, M, K, seed=SEED, init_mode=avhip.INIT_BERNOULLI, init_param=ls.P80)
    e.run_rounds(2)
    for _ in range(2):
        sim.run_round()
    gone = np.full((2, 3), avhip.ABSENT_WORD, np.uint32)  # some variety in the poll sets
    e.write_records(gone, n0=3, t0=50)
    sim.write_records(gone, 3, 50)
    e.set_valid(40, False)
    sim.set_valid(40, False)

    def state():
        return e.read_records(), e.applied_votes(), e.updates_count(), e.live_records(), e.get_invs_batch()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[:3] + a[4], b[:3] + b[4])) and a[3] == b[3]

    before = state()
    assert np.array_equal(before[0], sim.dump()[:, t0:t1])
    foreign = np.array([0, 31, 96, 129, -1, -7, 130, 1000, 31, 96], np.int64)  # below, above, negative, >= M
    assert e.register_votes(5, foreign, np.zeros(foreign.size, np.uint32)).tolist() == [-1] * foreign.size
    nodes, offs = np.array([5, 39, 5], np.int64), np.array([0, 4, 4, foreign.size], np.int64)
    assert e.register_votes_batch(nodes, offs, foreign, np.zeros(foreign.size, np.uint32)).tolist() == [-1] * foreign.size
    assert same(state(), before), "foreign votes changed the shard"
    assert e.add_targets(3, foreign, np.ones(foreign.size, np.uint8)).tolist() == [False] * foreign.size
    assert same(state(), before), "foreign add_targets changed the shard"
    for t in (0, 31, 96, 129, 8):  # 8 = the local index of the invalid target 40
        e.set_valid(t, False)
        assert same(state(), before), f"set_valid({t}) of a foreign target changed the shard"
        e.set_valid(t, True)
        assert same(state(), before)
    for rect in ((0, N, 31, 96), (0, N, 32, 97), (0, N, 0, 32), (0, N, 96, 130), (0, N + 1, 32, 96)):
        with pytest.raises(avhip.AvError):
            e.read_records(*rect)
    for w, start in ((np.zeros((2, 2), np.uint32), 31), (np.zeros((2, 2), np.uint32), 95), (np.zeros((1, 65), np.uint32), 32)):
        with pytest.raises(avhip.AvError):
            e.write_records(w, n0=0, t0=start)
    assert same(state(), before), "a refused rectangle changed the shard"
    offs, tg = before[4]
    live = (sim.dump() >> 17) < 128
    live[:, 40] = False
    for node in (0, 3, 4, 39):
        row = tg[offs[node]:offs[node + 1]].tolist()
        assert e.get_invs(node).tolist() == row == [t for t in np.flatnonzero(live[node]).tolist() if t0 <= t < t1]
    assert len(tg[offs[3]:offs[4]]) == 64 - 4 and len(tg[offs[0]:offs[1]]) == 63
    e.close()


def test_refused_writes_leave_no_trace_on_a_peer_group(oracle):
    sim = oracle.Sim(N, M, K, seed=SEED, init_mode=avhip.INIT_BERNOULLI, init_param=ls.P80)
    ranks = [avhip.Engine(N, M, k=K, seed=SEED, node_range=(r * 20, r * 20 + 20), log_capacity=ls.LOG_CAPACITY)
             for r in range(2)]
    group = sp.PeerGroup(ranks, avhip)
    group.init_records(avhip.INIT_BERNOULLI, ls.P80)
    group.group()
    group.run_rounds(2)
    exp = [sim.run_round()[0] for _ in range(2)]
    for e in ranks:
        node = e.node_range[0] + 1
        with pytest.raises(avhip.AvError):
            e.add_targets(node, np.array([3, 70]), np.array([1, 0], np.uint8))
        with pytest.raises(avhip.AvError):
            e.register_votes(node, np.array([3, 70]), np.zeros(2, np.uint32))
        with pytest.raises(avhip.AvError):
            e.write_records(np.zeros((2, 2), np.uint32), n0=node, t0=5)
        with pytest.raises(avhip.AvError):
            e.set_polling(node, False)
    assert np.array_equal(group.read_records(), sim.dump())
    assert group.updates_count() == sum(len(u) for u in exp)
    group.run_rounds(3)
    exp += [sim.run_round()[0] for _ in range(3)]
    assert np.array_equal(group.fetch_updates(), np.concatenate(exp))
    assert np.array_equal(group.read_records(), sim.dump())
    group.close()


@pytest.mark.parametrize("world", [2, 8])
def test_full_push_after_a_non_sweep_round_under_masked_pushes(oracle, world):
    """A first-generation round and a replay round between need-masked sweep rounds of a network whose
    rows keep changing (conflicting pairs, a Byzantine share): each ends in a full push of the rank's
    rows, without which the peers' next round reads rows three rounds old. (The lives flip the kernel
    of masked groups only in settled stretches, where such a row equals the current one.)"""
    n, m, byz = 64, 100, ls.BYZ20  # BL = 4: a layout with need-masked pushes
    per = n // world
    sim = oracle.Sim(n, m, K, seed=SEED, byz_threshold=byz, init_mode=avhip.INIT_PAIRS, init_param=0)

    def new_group(mask):
        ranks = [avhip.Engine(n, m, k=K, seed=SEED, byz_threshold=byz, node_range=(r * per, (r + 1) * per),
                              log_capacity=ls.LOG_CAPACITY) for r in range(world)]
        group = sp.PeerGroup(ranks, avhip)
        group.set_option("peer_mask", mask)
        group.init_records(avhip.INIT_PAIRS, 0)
        group.group()
        return group

    group, full = new_group(1), new_group(0)
    for what, v in [("rounds", 3), ("kernel", 1), ("rounds", 1), ("kernel", 2), ("rounds", 3), ("replay", 1), ("rounds", 3)]:
        if what == "kernel":
            group.set_option("kernel", v)
            continue
        first, rows = sim.round, sim.pref()
        if what == "replay":
            errs = oracle.gen_replay_errs(SEED, sim.round, 0, n, m, K)
            exp = [sim.run_round(errs)[0]]
            group.replay_round_errs(errs)
        else:
            exp = [sim.run_round()[0] for _ in range(v)]
            group.run_rounds(v)
        if v == 1:  # the two rounds that end in a full push
            assert (sim.pref() != rows).any(), f"round {first} must change published rows"
        assert np.array_equal(group.fetch_updates(), np.concatenate(exp)), f"updates of the rounds from {first}"
        assert np.array_equal(group.read_records(), sim.dump()), f"records after the rounds from {first}"
        if first == 0:  # the masks are in use: three sweep rounds push no more words than full pushes do
            full.run_rounds(v)
            pushed = [sum(e.pushed_words() for e in g.engines) for g in (group, full)]
            assert 0 < pushed[0] <= pushed[1] and (world == 2 or pushed[0] < pushed[1]), pushed
            full.close()
    honest = np.array([not sim.is_byzantine(j) for j in range(n)])
    assert np.array_equal(group.read_pref()[honest], sim.pref()[honest])
    group.close()


def test_generated_replay_on_shards(oracle):
    """av_replay_prepare / av_replay_rounds (the vote stream generated on the device from global node and
    target ids) on a target shard whose first target is not 0 and on a two-rank group: the oracle's
    stream of the whole network, cut to the shard."""
    t0, t1 = 32, 96
    shard = avhip.Engine(N, M, k=K, seed=SEED, target_range=(t0, t1), log_capacity=ls.LOG_CAPACITY)
    shard.init_records(avhip.INIT_BERNOULLI, ls.P80)
    group = sp.PeerGroup([avhip.Engine(N, M, k=K, seed=SEED, node_range=(r * 20, r * 20 + 20),
                                       log_capacity=ls.LOG_CAPACITY) for r in range(2)], avhip)
    group.init_records(avhip.INIT_BERNOULLI, ls.P80)
    group.group()
    sim = oracle.Sim(N, M, K, seed=SEED, init_mode=avhip.INIT_BERNOULLI, init_param=ls.P80)
    for e in [shard] + group.engines:
        e.replay_prepare(2)
    exp = []
    for _ in range(2):
        exp.append(sim.run_round(oracle.gen_replay_errs(SEED, sim.round, 0, N, M, K))[0])
        shard.replay_rounds(1)
        for e in group.engines:
            e.replay_rounds(1)
    exp = np.concatenate(exp)
    assert len(exp) > 0
    assert np.array_equal(shard.fetch_updates(), exp[(exp[:, 3] >= t0) & (exp[:, 3] < t1)])
    assert np.array_equal(shard.read_records(), sim.dump()[:, t0:t1])
    assert np.array_equal(group.fetch_updates(), exp)
    assert np.array_equal(group.read_records(), sim.dump())
    shard.close()
    group.close()
