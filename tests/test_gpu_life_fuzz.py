"""Randomised engine lives across the deferred record forms and the option paths.

test_life_fuzz: a schedule of life_schedule.make_schedule(seed) — rounds, API calls
at random positions inside deferred stretches, option switches, observations —
runs on three parties: the oracle, the engine under test with the schedule's
options, and a plain twin (same arguments, kernel 2, every deferral and shortcut
option off, never changed). After every step both engines' outputs equal the
oracle's bit for bit; a mismatch of the tested engine alone points at the options,
one of both at the engine. In the rounds the schedule flags taken (honest k = 8
seeds: the round before each phase-1 disturbance and one more after round 6,
whenever virtual_votes, count_lazy, uniform_rows or quiet_tiles is on with kernel
2) the tested engine's alg_bytes() delta must be strictly below the twin's: the
deferred form was really in use when the disturbance hit it
(tests/test_life_schedule_cpu.py shows on the oracle that those rounds sit in
settled stretches).

test_life_fuzz_lossy: the same loop over life_schedule.make_lossy_schedule(seed),
lives with stretches of lost Responses and unresponsive nodes (rule R5) laid over
them; the oracle's rounds inside a stretch are lossy_ref.LossyRef's. A regain
round, two rounds after a phase-1 SKIP stretch, is a taken round: the engine must
be deferring again by then.

test_option_paths_identical: every listed option value alone, on three fixed lives
(the third runs into and out of a SKIP and a NEUTRAL stretch), against the oracle."""
import numpy as np
import pytest

import avhip
import life_schedule as ls
import lossy_ref as L

pytestmark = pytest.mark.gpu


def new_engine(sched):
    return avhip.Engine(sched["n"], sched["m"], k=sched["k"], seed=sched["engine_seed"], byz_threshold=sched["byz"],
                        log_capacity=ls.LOG_CAPACITY)


def run_life(oracle, sched):
    """The three-party loop: the oracle, the engine under test and the plain twin over one schedule."""
    seed = sched["seed"]
    engines = {"test": new_engine(sched), "twin": new_engine(sched)}
    life = ls.Life(sched, oracle, engines, av=avhip)
    life.post_init = {"twin": [("fresh", 0)]}  # av_init_records sets the fact again
    life.set_options("test", sched["options"])
    life.set_options("twin", ls.PLAIN_OPTIONS)
    for name, e in engines.items():
        e.init_records(sched["init_mode"], sched["init_param"])
        life.set_options(name, life.post_init.get(name, ()))
    checks = []
    for i, step in enumerate(sched["steps"]):
        life.apply(i, step)
        if step["op"] == "rounds" and step["taken"]:
            got, plain = life.deltas["test"], life.deltas["twin"]
            checks.append((step["first"], "".join(d[0] for d in step["deferrals"]), got, plain))
            assert got < plain, (f"{life.where}: no deferred form taken in round {step['first']}: {got} bytes, plain twin "
                                 f"{plain}; options {life.options['test']}")
    kind = "lossy seed" if sched.get("lossy") else "seed"
    print(f"{kind} {seed} {sched['n']}x{sched['m']} k={sched['k']} taken (round, deferrals on, bytes, twin bytes): {checks}")
    for name, e in engines.items():
        assert e.applied_votes() == life.applied, (seed, name, "applied_votes")
        assert e.finalized_count() == life.finalized, (seed, name, "finalized_count")
        assert e.round == sched["rounds"]
        assert e.lost_responses() == life.ref.lost, (seed, name, "lost_responses")
        e.close()


@pytest.mark.parametrize("seed", range(ls.N_SEEDS))
def test_life_fuzz(oracle, seed):
    run_life(oracle, ls.make_schedule(seed))


@pytest.mark.parametrize("seed", range(ls.N_LOSSY_SEEDS))
def test_life_fuzz_lossy(oracle, seed):
    """The same loop on a lossy life: loss stretches (SKIP and NEUTRAL, nodes down) laid over the
    rounds, disturbances and observations of a full life; the regain rounds are among the taken ones."""
    run_life(oracle, ls.make_lossy_schedule(seed))


# ---- every option value alone
LIVES = [dict(n=200, m=256, byz=0, init_mode=avhip.INIT_BERNOULLI, init_param=ls.P80, rounds=24, seed=41),
         dict(n=67, m=640, byz=ls.BYZ20, init_mode=avhip.INIT_PAIRS, init_param=0, rounds=12, seed=42),
         dict(n=96, m=100, byz=0, init_mode=avhip.INIT_BERNOULLI, init_param=ls.P80, rounds=20, seed=43)]
# the third life's loss: (first round, threshold, mode, nodes down); nothing is lost before the first entry
LOSS = [(6, L.threshold(0.25), L.SKIP, [1, 3, 5]), (11, 0, L.SKIP, []), (14, L.threshold(0.08), L.NEUTRAL, []),
        (18, 0, L.SKIP, [])]
OPTION_CASES = [(nm, v) for nm, vs in ls.option_values(8).items() for v in vs]
THREE_ROUTES = ("dense_min", "wave_dense")


@pytest.fixture(scope="module")
def life_reference(oracle):
    """The three lives on the oracle, once: per-round update rows, final records and honest rows."""
    out = []
    for lf in LIVES:
        sim = oracle.Sim(lf["n"], lf["m"], 8, seed=lf["seed"], byz_threshold=lf["byz"], init_mode=lf["init_mode"],
                         init_param=lf["init_param"])
        if lf is LIVES[2]:  # 6 plain rounds, 5 SKIP, 3 plain, 4 NEUTRAL, 2 plain
            ref = L.LossyRef(sim, lf["seed"])
            ups, thr, mode = [], 0, L.SKIP
            for r in range(lf["rounds"]):
                for _, thr, mode, down in [x for x in LOSS if x[0] == r]:
                    ref.set_responding(sorted(ref.down), 1)
                    ref.set_responding(down, 0)
                ups.append(ref.round(thr, mode) if thr or ref.down else sim.run_round()[0])
            assert ref.lost > 0 and sum(len(ups[r]) for r in (6, 7, 8, 9, 10, 14, 15, 16, 17)) > 0
        else:
            ups = [sim.run_round()[0] for _ in range(lf["rounds"])]
        honest = np.array([not sim.is_byzantine(j) for j in range(lf["n"])])
        for a in ups:
            a.setflags(write=False)
        out.append((ups, sim.dump(), sim.pref()[honest], honest))
        sim.close()
    assert sum(len(u) for u in out[0][0]) > 0 and (out[0][1] >> 17 >= 128).any(), "the honest life must finalize"
    return out


@pytest.mark.parametrize("name,value", OPTION_CASES, ids=[f"{nm}={v}" for nm, v in OPTION_CASES])
def test_option_paths_identical(oracle, life_reference, name, value):
    for lf, (ups, dump, pref, honest) in zip(LIVES, life_reference):
        eng = avhip.Engine(lf["n"], lf["m"], k=8, seed=lf["seed"], byz_threshold=lf["byz"], log_capacity=ls.LOG_CAPACITY)
        eng.set_option(name, value)
        eng.init_records(lf["init_mode"], lf["init_param"])
        if name in ("fresh", "warm_skip"):  # switch-offs of a fact: av_init_records sets "fresh" again
            eng.set_option(name, value)
        for r, exp in enumerate(ups):
            where = f"{name}={value} {lf['n']}x{lf['m']} round {r}"
            for _, thr, mode, down in [x for x in LOSS if x[0] == r and lf is LIVES[2]]:
                eng.set_loss(thr, mode)
                eng.set_responding(list(range(lf["n"])), 1)
                eng.set_responding(down, 0)
            eng.run_rounds(1)
            route = r % 3 if name in THREE_ROUTES else 0
            base = eng.log_base_round()
            if route == 0:
                assert np.array_equal(eng.fetch_updates(), exp), where
            elif route == 1:
                assert np.array_equal(avhip.compact_expand(eng.fetch_compact()), ls.pack_updates(exp, base)), where
            else:
                assert eng.updates_digest() == oracle.update_digest(ls.pack_updates(exp, base)), where
                eng.discard_updates()
        assert np.array_equal(eng.read_records(), dump), f"{name}={value} {lf['n']}x{lf['m']} records"
        assert np.array_equal(eng.read_pref()[honest], pref), f"{name}={value} {lf['n']}x{lf['m']} published rows"
        eng.close()
