"""The life-fuzz schedule generator (life_schedule.py) checked on the CPU, with the
oracle alone: every seed replays, phase 1 keeps c_monotone, the Byzantine share
is bounded, and every taken seed really holds the settled stretches the GPU test's
taken check relies on — at each taken round (the round before a phase-1
disturbance, and one more after round 6) every row of the oracle's published
preferences is identical at the start of that round and of the two before it,
and every target is valid. Without that the GPU test could pass with no deferred
form ever in use.

The 32 schedules are pinned by a hash. The lossy lives (make_lossy_schedule) are
replayed on the oracle too: what their stretches must contain (updates and
finalizations emitted by lossy rounds, both modes, every kind of down set, every
disturbance inside some stretch, the three update routes) and that every regain
round follows a SKIP stretch into a settled, still c_monotone network."""
import hashlib

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


# ---- the 32 schedules are pinned; the lossy lives (make_lossy_schedule) on the oracle alone
SCHEDULES_SHA256 = "38b2d039371cff13fd7b214232db0080c4fa7e6d6f04b8de4aecfc480ff94906"
STRETCH_KINDS = ("register", "register_batch", "add", "set_valid", "materialize", "options", "kernel_flip", "write",
                 "neutral")


def test_the_32_schedules_are_pinned():
    """make_schedule(0..31) is what it was before the lossy lives came: SHA-256 over every seed's
    initial options and the one-line description of every step."""
    h = hashlib.sha256()
    for seed in range(ls.N_SEEDS):
        sched = ls.make_schedule(seed)
        h.update(repr(sched["options"]).encode())
        for step in sched["steps"]:
            h.update(ls.describe(step).encode() + b"\n")
    assert h.hexdigest() == SCHEDULES_SHA256


def disturbance_kind(step):
    if step["op"] == "register":
        return "neutral" if ls.breaks_c_monotone(step) else "register"
    if step["op"] == "options":
        return "kernel_flip" if step.get("tail") or step["set"] == [("kernel", 1)] else "options"
    return step["op"]


def walk(sched):
    """The steps with the round about to run and the loss state (threshold, mode, down set) at each."""
    r, thr, mode, down = 0, 0, ls.LOSS_SKIP, set()
    for step in sched["steps"]:
        yield step, r, thr, mode, frozenset(down)
        if step["op"] in ("rounds", "replay"):
            assert step["first"] == r
            r += step.get("c", 1)
        elif step["op"] == "set_loss":
            thr, mode = step["thr"], step["mode"]
        elif step["op"] == "set_responding":
            (down.difference_update if step["responds"] else down.update)(step["nodes"].tolist())


@pytest.fixture(scope="module")
def lossy_replays(oracle):
    out = {}
    for seed in range(ls.N_LOSSY_SEEDS):
        sched = ls.make_lossy_schedule(seed)
        state, life = replay(sched, oracle)
        out[seed] = (sched, state, life)
    return out


def test_lossy_schedule_twice():
    for seed in (3, 8):
        a, b = ls.make_lossy_schedule(seed), ls.make_lossy_schedule(seed)
        assert [ls.describe(s) for s in a["steps"]] == [ls.describe(s) for s in b["steps"]] and a["options"] == b["options"]
        assert a["stretches"] == b["stretches"] and a["regain"] == b["regain"]


def test_lossy_seeds_replay_and_emit_updates(lossy_replays):
    with_updates = with_final = 0
    for seed, (sched, _, life) in lossy_replays.items():
        assert 36 <= sched["rounds"] <= 48 and life.sim.round == sched["rounds"]
        assert sum(s.get("c", 1) for s in sched["steps"] if s["op"] in ("rounds", "replay")) == sched["rounds"]
        assert sum(s["op"] == "replay" for s in sched["steps"]) == 1
        assert life.thr == 0 and not life.ref.down, f"seed {seed}: a stretch is left open"
        assert life.ref.lost > 0 and life.lossy_rows, seed
        rows = np.concatenate(life.lossy_rows)
        with_updates += len(rows) > 0
        with_final += bool(np.isin(rows[:, 4], (0, 3)).any())
    assert with_updates >= 8 and with_final >= 4, (with_updates, with_final)


def test_lossy_seed_mix():
    modes, downs, thrs, ks, byz, shapes = set(), set(), set(), [], 0, set()
    all_down_rounds = 0
    for seed in range(ls.N_LOSSY_SEEDS):
        sched = ls.make_lossy_schedule(seed)
        n = sched["n"]
        ks.append(sched["k"])
        byz += bool(sched["byz"])
        shapes.add((n, sched["m"]))
        assert 1 <= len(sched["stretches"]) <= 3 and all(2 <= b - a <= 8 for a, b in sched["stretches"]), seed
        for step, r, thr, mode, down in walk(sched):
            if step["op"] != "rounds" or not (thr or down):
                continue
            assert any(a <= r and r + step["c"] <= b for a, b in sched["stretches"]), (seed, r)
            modes.add(mode)
            thrs.add(thr)
            all_down_rounds += step["c"] * (len(down) == n)
            word = len(down) >= 32 and any(set(range(32 * w, 32 * w + 32)) <= down for w in range(n // 32))
            downs.add("none" if not down else "all" if len(down) == n else "word" if word else
                      "ends" if down == {0, n - 1} else "few")
        # outside the stretches nothing is lost
        for step, r, thr, mode, down in walk(sched):
            if step["op"] == "rounds" and not any(a <= r < b for a, b in sched["stretches"]):
                assert not thr and not down, (seed, r)
    assert modes == {ls.LOSS_SKIP, ls.LOSS_NEUTRAL} and downs == {"none", "few", "ends", "word", "all"}, (modes, downs)
    assert 0 in thrs and ls.THR_MAX in thrs and all_down_rounds == 1, (sorted(thrs), all_down_rounds)
    assert {int(p * 2**32) for p in ls.SKIP_P + ls.NEUTRAL_P} <= thrs
    assert ks.count(12) >= 1 and sum(k in (1, 3, 5) for k in ks) >= 2 and byz >= 3
    assert all(k in (1, 3, 5, 8, 12) for k in ks) and shapes == set(ls.SHAPES)
    honest8 = [s for s in range(ls.N_LOSSY_SEEDS) if ls.lossy_config(s)[2:] == (0, 8)]
    assert len(honest8) == ls.N_LOSSY_SEEDS - byz - sum(k != 8 for k in ks)


def test_lossy_stretch_contents():
    multi = mode_changes = down_changes = 0
    inside = {kd: 0 for kd in STRETCH_KINDS + ("reinit", "replay")}
    routes = {0: set(), 1: set(), 2: set()}
    for seed in range(ls.N_LOSSY_SEEDS):
        sched = ls.make_lossy_schedule(seed)
        seen, multi_here, prev = set(), False, None
        for step, r, thr, mode, down in walk(sched):
            lossy = bool(thr or down)
            if step["op"] == "rounds" and lossy:
                multi_here |= step["c"] >= 2
                routes[step["route"]].add(seed)
            elif lossy and step["op"] not in ("observe", "set_loss", "set_responding", "rounds"):
                seen.add(disturbance_kind(step))
            elif lossy and step["op"] == "set_loss" and step["thr"] and step["mode"] != mode:
                mode_changes += 1
            elif lossy and step["op"] == "set_responding" and any(a < r < b for a, b in sched["stretches"]):
                down_changes += len(step["nodes"]) == 1
            prev = step
        multi += multi_here
        for kd in seen:
            inside[kd] += 1
    assert multi >= 6 and mode_changes >= 2 and down_changes >= 2, (multi, mode_changes, down_changes)
    assert all(inside[kd] >= 1 for kd in STRETCH_KINDS) and inside["reinit"] >= 2 and inside["replay"] >= 2, sorted(inside.items())
    assert all(len(v) >= 4 for v in routes.values()), routes


def test_lossy_phase1_keeps_c_monotone():
    for seed in range(ls.N_LOSSY_SEEDS):
        sched = ls.make_lossy_schedule(seed)
        for step in phase1_steps(sched):
            assert not ls.breaks_c_monotone(step), (seed, ls.describe(step))
            assert step["op"] != "set_loss" or step["mode"] == ls.LOSS_SKIP
        assert any(ls.breaks_c_monotone(s) for s in sched["steps"])


def test_regain_rounds_follow_settled_skip_stretches(lossy_replays):
    """A regain round is b + 2 for a phase-1 SKIP stretch [a, b) of an honest k = 8 seed: rounds b, b + 1
    and b + 2 start with identical published rows and every target valid, no step but observations lies
    between them, c_monotone still holds, and the options in force let plan_round defer."""
    found = 0
    for seed, (sched, state, _) in lossy_replays.items():
        flagged = [s["first"] for s in sched["steps"] if s["op"] == "rounds" and s.get("regain")]
        assert flagged == sched["regain"], seed
        if not sched["taken_seed"]:
            assert not flagged and not any(s.get("taken") for s in sched["steps"]), seed
            continue
        cur = dict(ls.DEFAULTS)
        cur.update({nm: v for nm, v in sched["options"] if nm in cur})
        bound, monotone, quiet_since, skip_only = -6, True, 0, {}
        for step, r, thr, mode, down in walk(sched):
            if step["op"] == "rounds":
                for x in range(r, r + step["c"]):
                    for a, b in sched["stretches"]:
                        if a <= x < b:
                            skip_only[b] = skip_only.get(b, True) and mode == ls.LOSS_SKIP
                if step.get("taken"):
                    assert step["c"] == 1 and not (thr or down), (seed, r)
                    assert not any(a <= r < b + 2 for a, b in sched["stretches"]), (seed, r)
                if step.get("regain"):
                    b = r - 2
                    assert step["taken"] and b in [y for _, y in sched["stretches"]] and skip_only[b], (seed, r)
                    assert monotone and quiet_since <= b <= sched["phase1"], (seed, r, quiet_since)
                    lazy = cur["count_lazy"] and bound < 120
                    assert cur["kernel"] == 2 and (cur["virtual_votes"] or lazy), (seed, r, cur, bound)
                    for x in (b, b + 1, b + 2):
                        assert state[x] == (True, True), f"seed {seed}: regain round {r}, round {x}: {state[x]}"
                    found += 1
                bound = min(127, bound + 8 * step["c"])
                continue
            if step["op"] == "observe":
                continue
            monotone = monotone and not ls.breaks_c_monotone(step)
            if step["op"] in ("set_loss", "set_responding") and not (step["op"] == "set_loss" and step["thr"]) and \
                    not (step["op"] == "set_responding" and not step["responds"]):
                continue  # a stretch's closing steps
            quiet_since = r + 1
            if step["op"] == "replay":
                bound = min(127, bound + 8)
            elif step["op"] == "reinit":
                bound = -6
            elif step["op"] == "write":
                bound = 127
            elif step["op"] in ("register", "register_batch"):
                bound = min(127, bound + ls.max_node_votes(step))
            elif step["op"] == "options":
                cur.update({nm: v for nm, v in step["set"] if nm in cur})
    assert found >= 4, found
