"""Behavioural trace of the round planner against a recorded run.

Every scenario below drives an engine through the transitions the host tracks as record facts
(csrc/round_plan.h: fresh -> klazy -> kconsume, quiet tiles, the A/B switches, the lean loop off,
k = 4, the capped node kernel and fused replay, adds / drop-in votes / record writes between
rounds, the first-generation kernel). After every round it reads the counters that any change of
the plan would move (algorithmic bytes and their re-read part, applied votes, finalized records,
the digest of the pending StatusUpdates), at the end the records, and compares all of it with
tests/golden/round_trace.json, recorded with this script from the commit before the planner became
one module:

    python tests/test_gpu_round_trace.py OUT.json     # AVHIP_LIB selects the library recorded

Every counter was identical in two recordings of that commit.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "round_trace.json")
SEED = 0xA7A1A9C4
BYZ = int(0.2 * 2**32)
P80 = int(0.8 * 2**32)


class Trace:
    def __init__(self, eng):
        self.eng, self.rounds, self.events = eng, [], {}

    def snap(self):
        e = self.eng
        self.rounds.append([e.alg_bytes(), e.alg_bytes_reread(), e.applied_votes(), e.finalized_count(),
                            *e.updates_digest()])

    def run(self, rounds):
        for _ in range(rounds):
            self.eng.run_rounds(1)
            self.snap()

    def result(self):
        rec = self.eng.read_records()
        self.eng.close()
        return {"rounds": self.rounds, "events": self.events, "records_shape": list(rec.shape),
                "records_sha256": hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest()}


def _engine(avhip, n=64, m=1024, k=8, byz=BYZ, mode=None, options=()):
    eng = avhip.Engine(n, m, k=k, seed=SEED, byz_threshold=byz, device=0)
    for name, value in options:
        eng.set_option(name, value)
    eng.init_records(avhip.INIT_BERNOULLI if mode is None else mode, P80)
    return Trace(eng)


def _plain(rounds, **kw):
    def scenario(avhip):
        t = _engine(avhip, **kw)
        t.run(rounds)
        return t.result()
    return scenario


def _all_accept(avhip):
    t = _engine(avhip, byz=0, mode=avhip.INIT_ACCEPTED)
    t.run(20)
    return t.result()


def _capped_replay(fuse):
    def scenario(avhip):
        t = _engine(avhip, n=16, m=5000, options=() if fuse is None else (("replay_fuse", fuse),))
        assert t.eng.layout_info()["capped"]
        t.run(6)
        t.eng.replay_prepare(20)
        if fuse is None:  # the default: fused launches, one call
            t.eng.replay_rounds(20)
            t.snap()
        else:
            for _ in range(20):
                t.eng.replay_rounds(1)
                t.snap()
        return t.result()
    return scenario


def _writes_between_rounds(avhip):
    t = _engine(avhip)
    t.run(5)
    t.events["added"] = t.eng.add_targets(3, [0, 5, 1023], [1, 0, 1]).astype(int).tolist()
    t.run(3)
    st = t.eng.register_votes_batch([2], [0, 3], [1, 2, 3], [0, 1, 0x80000000])  # yes, no, neutral
    t.events["vote_status"] = st.astype(int).tolist()
    t.run(3)
    t.eng.write_records(t.eng.read_records(n0=5, n1=6), n0=6)  # node 5's row over node 6's
    t.run(3)
    return t.result()


SCENARIOS = {
    "a_bernoulli_byz": _plain(20),  # BL = 32: fresh -> klazy -> kconsume at round 16
    "b_all_accept": _all_accept,  # the quiet-tile and uniform-row path
    "c_count_lazy_0": _plain(20, options=(("count_lazy", 0),)),
    "c_virtual_votes_0": _plain(20, options=(("virtual_votes", 0),)),
    "d_m200": _plain(10, m=200),  # BL = 7: lean loop off
    "e_k4": _plain(10, k=4),
    "f_capped_replay_fused": _capped_replay(None),
    "f_capped_replay_unfused": _capped_replay(1),
    "g_writes_between_rounds": _writes_between_rounds,
    "h_responder_1": _plain(5, options=(("responder", 1),)),  # the first-generation kernel
}


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_round_trace(name, fixture):
    import avhip

    got = json.loads(json.dumps(SCENARIOS[name](avhip)))
    exp = fixture[name]
    assert len(got["rounds"]) == len(exp["rounds"])
    for r, (g, x) in enumerate(zip(got["rounds"], exp["rounds"])):
        assert g == x, f"{name}: counters after step {r} (bytes, reread, applied, finalized, digest x3)"
    assert got == exp


def test_fixture_covers_every_scenario(fixture):
    assert sorted(fixture) == sorted(SCENARIOS)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "go-avalanche_amd", "python")]
    import avhip

    out = {name: fn(avhip) for name, fn in sorted(SCENARIOS.items())}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} scenarios with {avhip.LIB_PATH}")
