"""Network-quiet rounds (sweep_settled.h, option net_quiet, default on): when every
run of the network was quiescent in round r - 1 and nothing was written since, round
r adds the deferred count step to the tile words alone: a leader wave takes
net_quiet_group runs, the others end at once. Bytes, applied votes, records,
rows and the log are those of the per-run quiescent path, so the tests tell the
path by its counter (Engine.net_quiet_rounds).

A round is fully quiescent exactly when it moves 8 B per tile (its kpend word read
and written) and nothing else: the tests derive from that, not from the counter,
which rounds must take the path: round r takes it iff rounds r - 1 and r both move
8 B per tile and no writer was called between them."""
import os

import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
BYZ20 = int(0.2 * 2**32)
T = max(1, min(8, os.cpu_count() or 1))


def rows(u):
    return [tuple(int(v) for v in r) for r in np.asarray(u).tolist()]


class Watch:
    """Runs rounds one at a time and holds the counter against the byte counter."""

    def __init__(self, eng, enabled=True):
        self.eng = eng
        self.enabled = enabled  # option net_quiet
        self.tiles = (eng.layout_info()["lanes"] + 63) // 64
        self.prev_quiet = False
        self.taken = eng.net_quiet_rounds
        self.log = []

    def wrote(self):
        """A writer was called: the next round may not take the path."""
        self.prev_quiet = False

    def round(self, expect=None):
        b0 = self.eng.alg_bytes()
        self.eng.run_rounds(1)
        quiet = self.eng.alg_bytes() - b0 == 8 * self.tiles
        got = self.eng.net_quiet_rounds - self.taken
        want = int(self.prev_quiet and quiet and self.enabled)
        self.log.append((quiet, got))
        assert got == want, (self.log, "round took the path" if got else "round did not take the path")
        if expect is not None:
            assert got == expect, self.log
        self.taken += got
        self.prev_quiet = quiet
        return got


def make(n, m, init=avhip.INIT_ACCEPTED, param=0, opts=(), seed=3, byz=0, k=8, log=1 << 22):
    eng = avhip.Engine(n, m, k=k, seed=seed, byz_threshold=byz, log_capacity=log)
    for name, v in opts:
        eng.set_option(name, v)
    eng.init_records(init, param)
    return eng


@pytest.mark.parametrize("n", [64, 1000])
@pytest.mark.parametrize("m", [1024, 256, 128])
def test_path_taken(n, m):
    """All-accepted honest network: round 0 is the fresh round, round 1 and 2 defer, round 3 is
    the first fully quiescent one; rounds 4..15 take the path, round 16 (kconsume) and later do
    not. Reads between the rounds do not break the stretch."""
    eng = make(n, m, log=1 << 21)
    w = Watch(eng)
    for r in range(20):
        w.round(expect=1 if 4 <= r <= 15 else 0)
        assert eng.net_quiet_rounds == max(0, min(r, 15) - 3), r
        if r in (5, 6, 9):
            eng.read_records(0, 2)
            eng.read_pref(0, 2)
            eng.census()
    assert eng.finalized_count() == n * m
    eng.close()


def life(n, m, on, chunked, opts, rounds=20, init=avhip.INIT_BERNOULLI, param=P80, seed=5):
    eng = make(n, m, init, param, opts=tuple(opts) + (("net_quiet", on),), seed=seed, log=1 << 23)
    out = []
    for _ in range(rounds if chunked else 1):
        eng.run_rounds(1 if chunked else rounds)
        out.append(dict(rec=eng.read_records(), pref=eng.read_pref(), bytes=eng.alg_bytes(),
                        reread=eng.alg_bytes_reread(), applied=eng.applied_votes(), fin=eng.finalized_count(),
                        dig=eng.updates_digest(), dig_lo=eng.updates_digest(0, n // 2)))
    taken = eng.net_quiet_rounds
    eng.close()
    return out, taken


def same(a, b):
    assert len(a) == len(b)
    for r, (x, y) in enumerate(zip(a, b)):
        for key in ("bytes", "reread", "applied", "fin", "dig", "dig_lo"):
            assert x[key] == y[key], (r, key, x[key], y[key])
        np.testing.assert_array_equal(x["rec"], y["rec"], err_msg=f"records after round {r}")
        np.testing.assert_array_equal(x["pref"], y["pref"], err_msg=f"rows after round {r}")


def identity(n, m, tpw, group, merge=1, front=1):
    opts = (("tiles_per_wave", tpw), ("net_quiet_group", group), ("uni_merge", merge), ("net_quiet_front", front))
    on, taken = life(n, m, 1, True, opts)
    off, none = life(n, m, 0, True, opts)
    same(on, off)
    assert none == 0 and taken > 0, (taken, none)
    on20, taken20 = life(n, m, 1, False, opts)
    off20, _ = life(n, m, 0, False, opts)
    same(on20, off20)
    same(on20, on[-1:])
    assert taken20 == taken


@pytest.mark.parametrize("m", [1024, 256, 128])
@pytest.mark.parametrize("tpw,group,merge,front", [
    (1, 1, 1, 1), (1, 16, 1, 1), (2, 4, 1, 1), (3, 4, 1, 1), (4, 4, 1, 1), (5, 16, 1, 1), (8, 4, 2, 1), (16, 1, 1, 1),
    (16, 4, 1, 1), (16, 16, 1, 1), (4, 16, 4, 1), (1, 16, 1, 0), (4, 4, 1, 0), (7, 4, 1, 0), (16, 16, 1, 0)])
def test_option_identity(m, tpw, group, merge, front):
    """net_quiet 0 and 1 are identical after every one of 20 rounds, run one by one and as
    run_rounds(20): Bernoulli(0.8) through convergence, the quiet stretch and the finalization
    storm. 700 nodes: 350 / 88 / 44 tiles, no multiple of most run and group lengths. front: the
    leaders are the grid's first waves (default) or every group-th wave."""
    identity(700, m, tpw, group, merge, front)


@pytest.mark.parametrize("n", [37, 65, 513, 4097])
@pytest.mark.parametrize("m", [1024, 256, 128])
def test_edge_geometry(n, m):
    """Half-full last tiles (BL 32: every odd N; BL 8 / 4: N no multiple of 8 / 16), tile counts
    that are no multiple of group x run, wave counts that are no multiple of the group."""
    lanes = n * (m // 32)
    tiles = (lanes + 63) // 64
    assert lanes % 64 == 32 if m == 1024 else lanes % 64 != 0
    for tpw, group, front in ((4, 4, 1), (16, 16, 1), (3, 5, 1), (3, 5, 0), (16, 16, 0)):
        waves = (tiles + tpw - 1) // tpw
        if tiles > group * tpw:
            assert tiles % (group * tpw) != 0
        if waves > group and (tpw, group) == (3, 5):
            assert waves % group != 0, (tiles, waves)
        opts = (("tiles_per_wave", tpw), ("net_quiet_group", group), ("net_quiet_front", front))
        on, taken = life(n, m, 1, False, opts, rounds=14)
        off, _ = life(n, m, 0, False, opts, rounds=14)
        same(on, off)
        assert taken > 0
        # all-accepted: rounds 4..15 take the path, whatever the geometry
        on, taken = life(n, m, 1, False, opts, rounds=16, init=avhip.INIT_ACCEPTED, param=0)
        off, _ = life(n, m, 0, False, opts, rounds=16, init=avhip.INIT_ACCEPTED, param=0)
        same(on, off)
        assert taken == 12


WRITERS = ["set_valid", "register_votes_batch", "add_targets", "write_records", "materialize", "set_option",
           "init_records"]


@pytest.mark.parametrize("writer", WRITERS)
def test_writers_break_it(oracle, writer):
    """A writer inside the quiet stretch: the counter stays flat until two deferred rounds and
    one fully quiescent round have passed (Watch holds every round to the byte counter), at
    least three rounds; state and StatusUpdates equal the oracle's throughout."""
    n, m = 300, 1024
    eng = make(n, m, seed=93)
    sim = oracle.Sim(n, m, 8, seed=93, init_mode=avhip.INIT_ACCEPTED, init_param=0, threads=T)
    w = Watch(eng)

    def step(expect=None):
        got = w.round(expect)
        exp, _ = sim.run_round(threads=T)
        assert rows(eng.fetch_updates()) == rows(exp)
        return got

    for r in range(6):
        step(expect=1 if r >= 4 else 0)
    if writer == "set_valid":  # one round without target 3, then with it again
        eng.set_valid(3, False)
        sim.set_valid(3, False)
        w.wrote()
        step(expect=0)
        eng.set_valid(3, True)
        sim.set_valid(3, True)
    elif writer == "register_votes_batch":
        eng.register_votes_batch([5], [0, 2], [0, 1], [0, 0])
        sim.register_votes(5, [0, 1], np.array([0, 0], np.uint32))
        eng.discard_updates()
    elif writer == "add_targets":
        got = eng.add_targets(11, [4, 5], [True, True])
        assert list(map(bool, got)) == [sim.add(11, t, True) for t in (4, 5)]
    elif writer == "write_records":
        words = eng.read_records(0, 3)
        eng.write_records(words, 0, 0)
        sim.write_records(words, 0, 0)
    elif writer == "materialize":
        eng.materialize()
    elif writer == "set_option":
        eng.set_option("uni_votes", 1)
    elif writer == "init_records":
        eng.discard_updates()
        eng.init_records(avhip.INIT_ACCEPTED, 0)
        sim.close()
        sim = oracle.Sim(n, m, 8, seed=93, init_mode=avhip.INIT_ACCEPTED, init_param=0, threads=T)
        sim.set_round_index(6)
    w.wrote()
    np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T))
    taken = [step() for _ in range(9)]
    print(writer, "(quiescent, taken) per round:", w.log)
    assert taken[:3] == [0, 0, 0], taken
    if writer in ("set_valid", "register_votes_batch", "materialize", "set_option"):
        assert taken[3:] == [1] * 6, taken  # two deferred and one quiescent round behind them
    elif writer in ("init_records", "add_targets"):
        # the fresh round (init) / a round that checks the consider planes again (add) comes first
        assert taken[3] == 0 and taken[4:] == [1] * 5, taken
    else:  # written consider planes are no longer known all-ones: no deferred rounds at all
        assert taken == [0] * 9, taken
    np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T))
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


@pytest.mark.parametrize("case", ["byzantine", "k4", "quiet_tiles_off", "kernel1", "net_quiet_off"])
def test_never_taken(case):
    n, m = 500, 1024
    kw = dict(byzantine=dict(byz=BYZ20, init=avhip.INIT_BERNOULLI, param=P80), k4=dict(k=4),
              quiet_tiles_off=dict(opts=(("quiet_tiles", 0),)), kernel1=dict(opts=(("kernel", 1),)),
              net_quiet_off=dict(opts=(("net_quiet", 0),)))[case]
    eng = make(n, m, **kw)
    for _ in range(18):
        eng.run_rounds(1)
        assert eng.net_quiet_rounds == 0
    eng.close()


def test_pairs_not_before_settling(oracle):
    """INIT_PAIRS: no round takes the path before the network has settled and a whole round was
    quiescent (Watch); results equal the oracle's."""
    n, m = 400, 517
    eng = make(n, m, avhip.INIT_PAIRS, P80, seed=17)
    sim = oracle.Sim(n, m, 8, seed=17, init_mode=avhip.INIT_PAIRS, init_param=P80, threads=T)
    w = Watch(eng)
    for r in range(18):
        w.round(expect=0 if r < 4 else None)
        exp, _ = sim.run_round(threads=T)
        assert rows(eng.fetch_updates()) == rows(exp), r
    print("pairs: (quiescent, taken) per round", w.log)
    np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T))
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


def epoch_protocol(on, mat_at):
    """The benchmark's epoch protocol: 16 rounds, the log dropped and the records re-initialised,
    16 more rounds with a write-back inside the stretch, the final write-back, a read."""
    n, m = 2048, 1024
    eng = make(n, m, avhip.INIT_BERNOULLI, P80, opts=(("net_quiet", on),), seed=0xA7A1A9C4, log=1 << 24)
    w = Watch(eng, enabled=bool(on))
    seen, took = [], []
    for epoch in range(2):
        for r in range(16):
            took.append(w.round())
            if epoch == 1 and r == mat_at:
                eng.materialize()
                w.wrote()
        seen.append((eng.updates_digest(), eng.applied_votes(), eng.finalized_count(), eng.alg_bytes()))
        if epoch == 0:
            eng.discard_updates()
            eng.init_records(avhip.INIT_BERNOULLI, P80)
            w.wrote()
    eng.materialize()
    rec, pref = eng.read_records(), eng.read_pref()
    eng.close()
    return seen, rec, pref, took


def test_epoch_protocol():
    on = epoch_protocol(1, 11)
    off = epoch_protocol(0, 11)
    assert on[0] == off[0]
    np.testing.assert_array_equal(on[1], off[1])
    np.testing.assert_array_equal(on[2], off[2])
    took = on[3]
    print("epoch protocol, rounds that took the path:", took)
    assert sum(took[:16]) > 0 and sum(took[16:28]) > 0
    assert took[28:31] == [0, 0, 0] and took[31] == 1, took  # rounds 12-14 after the write-back, then 15
    assert sum(off[3]) == 0
