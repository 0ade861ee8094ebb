"""The life-fuzz schedule generator (life_schedule.py) checked on the CPU, with the
oracle alone: every seed replays, phase 1 keeps c_monotone, the Byzantine share
is bounded, and every taken seed really holds the settled stretches the GPU test's
taken check relies on — at each taken round (the round before a phase-1
disturbance, and one more after round 6) every row of the oracle's published
preferences is identical at the start of that round and of the two before it,
and every target is valid. Without that the GPU test could pass with no deferred
form ever in use."""
import numpy as np
import pytest

import life_schedule as ls


def phase1_steps(sched):
    out, r = [], 0
    for step in sched["steps"]:
        if r >= sched["phase1"]:
            break
        if step["op"] in ("rounds", "replay"):
            r = step["first"] + step.get("c", 1)
        out.append(step)
    return out


def replay(sched, oracle):
    """A schedule replayed on the oracle alone: the per-round (rows identical, all valid) and the Life."""
    life = ls.Life(sched, oracle)
    state = {}

    def hook(r, sim, valid):
        pref = sim.pref()
        state[r] = (bool((pref == pref[0]).all()), bool(valid.all()))

    life.round_hook = hook
    for i, step in enumerate(sched["steps"]):
        life.apply(i, step)
    assert sorted(state) == list(range(sched["rounds"])), sched["seed"]
    return state, life


@pytest.fixture(scope="module")
def replays(oracle):
    """Every seed's schedule replayed once on the oracle: per seed, the per-round (rows identical, all valid)."""
    out = {}
    for seed in range(ls.N_SEEDS):
        sched = ls.make_schedule(seed)
        state, life = replay(sched, oracle)
        out[seed] = (sched, state, life)
    return out


def test_every_seed_replays(replays):
    shapes, inits, ks, ops, opts = set(), set(), set(), set(), set()
    for sched, _, life in replays.values():
        assert 36 <= sched["rounds"] <= 48
        assert life.sim.round == sched["rounds"]
        assert sum(s["c"] if s["op"] == "rounds" else 1 for s in sched["steps"] if s["op"] in ("rounds", "replay")) == \
            sched["rounds"]
        assert sum(s["op"] == "replay" for s in sched["steps"]) == 1
        shapes.add((sched["n"], sched["m"]))
        inits.add((sched["init_mode"], sched["init_param"]))
        ks.add(sched["k"])
        ops.update(s["what"] if s["op"] == "observe" else s["op"] for s in sched["steps"])
        opts.update(tuple(x) for x in sched["options"])
        for s in sched["steps"]:
            if s["op"] == "options":
                opts.update(tuple(x) for x in s["set"])
    assert shapes == set(ls.SHAPES) and inits == set(ls.INITS) and 8 in ks and ks & {3, 5}
    assert ops >= set(ls.OBSERVATIONS) | (set(ls.PHASE1_KINDS) - {"kernel_flip"}) | {"write", "replay", "rounds"}
    # every listed option value is drawn by some seed
    missing = {(nm, v) for nm, vs in ls.option_values(8).items() for v in vs} - opts
    assert not missing, missing


def test_same_schedule_twice():
    a, b = ls.make_schedule(5), ls.make_schedule(5)
    assert [ls.describe(s) for s in a["steps"]] == [ls.describe(s) for s in b["steps"]] and a["options"] == b["options"]


def test_phase1_keeps_c_monotone():
    broke_later = 0
    for seed in range(ls.N_SEEDS):
        sched = ls.make_schedule(seed)
        assert ("warm_skip", 0) not in [tuple(x) for x in sched["options"]]
        first = phase1_steps(sched)
        for step in first:
            assert not ls.breaks_c_monotone(step), (seed, ls.describe(step))
        broke_later += any(ls.breaks_c_monotone(s) for s in sched["steps"][len(first):])
    assert broke_later == ls.N_SEEDS  # phase 2 always holds the replay round


def test_kernel_switched_in_mid_life():
    """kernel 2 -> 1 -> 2 inside phase 1 of taken seeds (deferred state to write back) and elsewhere."""
    in_taken = anywhere = 0
    for seed in range(ls.N_SEEDS):
        sched = ls.make_schedule(seed)
        flips = [s for s in sched["steps"] if s["op"] == "options" and s.get("tail")]
        anywhere += bool(flips)
        in_taken += bool(sched["taken_seed"] and any(s.get("tail") and s["op"] == "options" for s in phase1_steps(sched)))
    assert anywhere >= 8 and in_taken >= 4, (anywhere, in_taken)


def test_honest_seeds_space_their_phase1_disturbances():
    for seed in range(ls.N_SEEDS):
        sched = ls.make_schedule(seed)
        if sched["byz"]:
            continue
        r, last = 0, None
        for step in phase1_steps(sched):
            if step["op"] in ("rounds", "replay"):
                r = step["first"] + step.get("c", 1)
            elif step["op"] != "observe":
                if not step.get("tail"):
                    assert r >= 6 and (last is None or r == last or r - last >= 5), (seed, r, last)
                last = r


def test_byzantine_share():
    byz = [seed for seed in range(ls.N_SEEDS) if ls.make_schedule(seed)["byz"]]
    assert 0 < len(byz) <= ls.N_SEEDS // 4
    small_k = [seed for seed in range(ls.N_SEEDS) if ls.make_schedule(seed)["k"] != 8]
    assert len(small_k) == ls.N_SEEDS // 8


def test_taken_rounds_sit_in_settled_stretches(replays):
    checked, quiet_seeds = 0, []
    for seed, (sched, state, _) in replays.items():
        taken = [s["first"] for s in sched["steps"] if s["op"] == "rounds" and s.get("taken")]
        if not sched["taken_seed"]:
            assert not taken, seed
            continue
        assert all(s["c"] == 1 for s in sched["steps"] if s["op"] == "rounds" and s.get("taken")), seed
        if not taken:  # kernel 1, or all four deferrals off, at every phase-1 disturbance (checked below)
            quiet_seeds.append(seed)
        assert not taken or (max(taken) > 6 and min(taken) >= 6), (seed, taken)
        # disturbances of phase 1: none before round 6, >= 5 rounds apart; each is preceded by a taken
        # round whenever the options in force leave a deferral on with kernel 2
        cur = dict(ls.DEFAULTS)
        cur.update({nm: v for nm, v in sched["options"] if nm in cur})
        r, last, pending = 0, None, set()
        bound, bound_r, deferrable = -6, 0, {}  # count_bound as round_plan.h keeps it
        for step in phase1_steps(sched):
            if step["op"] in ("rounds", "replay"):
                r = step["first"] + (step["c"] if step["op"] == "rounds" else 1)
                continue
            if step["op"] == "observe":
                continue
            if step.get("tail"):  # the second half of a validity flip or of a kernel 2 -> 1 -> 2 switch
                assert r - last <= 3, (seed, r)
                if step["op"] == "set_valid":
                    assert step["valid"] and step["t"] in pending
                    pending.discard(step["t"])
                else:
                    assert step["set"] == [("kernel", 2)] and cur["kernel"] == 1
                    cur["kernel"] = 2
                last = r
                continue
            assert r >= 6 and (last is None or r == last or r - last >= 5), (seed, r, last)
            if cur["kernel"] == 2 and any(cur[d] for d in ls.DEFERRALS):
                assert r - 1 in taken, (seed, r)
            for x in (r - 2, r - 1):
                # what plan_round can defer in round x: stale vote planes in any warm round, count steps
                # (and with them quiescent tiles) only while count_bound < 120
                deferrable.setdefault(x, bool(cur["virtual_votes"]) or
                                      (bool(cur["count_lazy"]) and min(127, bound + 8 * (x - bound_r)) < 120))
            if step["op"] == "reinit":
                bound, bound_r = -6, r
            if step["op"] in ("register", "register_batch"):
                bound, bound_r = min(127, bound + 8 * (r - bound_r) + ls.max_node_votes(step)), r
            if step["op"] == "set_valid":
                pending.add(step["t"])
            if step["op"] == "options":
                cur.update({nm: v for nm, v in step["set"] if nm in cur})
            last = r
        for x in taken:
            assert deferrable[x], f"seed {seed}: nothing can be deferred in taken round {x}"
            for rr in (x - 2, x - 1, x):
                same_rows, all_valid = state[rr]
                assert same_rows and all_valid, f"seed {seed}: taken round {x}, round {rr}: rows identical " \
                                                f"{same_rows}, all valid {all_valid}"
            checked += 1
    assert len(quiet_seeds) <= 2, quiet_seeds
    assert checked >= 2 * (sum(s[0]["taken_seed"] for s in replays.values()) - len(quiet_seeds))
