"""Quiescent tiles (sweep_settled.h, option quiet_tiles, default on): a settled
tile that deferred its count step in the two rounds before this one, in a round
whose input snapshot and the one before it are both uniform, and whose run holds
no Byzantine node, takes one more deferred +8 step with no A-plane read and no
republished row: its A plane is what it published three rounds ago into the
buffer this round writes, and equals the reference word every vote would be.

Checked against the oracle with API calls placed inside the quiescent stretch
(drop-in votes, validity flips, reads, adds, re-initialisation, write-backs),
against the same engine with the option off through a network's whole life at
several run shapes, and by the byte counter: a quiescent tile moves its kpend
word (read and written, 8 B) and nothing per lane."""
import os

import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
P97 = int(0.97 * 2**32)
BYZ20 = int(0.2 * 2**32)
T = max(1, min(8, os.cpu_count() or 1))


def rows(u):
    return [tuple(int(v) for v in r) for r in np.asarray(u).tolist()]


def test_quiet_tiles_bytes():
    """All-accepted 4000 x 1000 (BL 32, 2000 whole tiles). Round 2 is settled with one
    deferred round behind it (incoming pend 1): 8 B per lane (the A read, the
    published word) + the kpend word. From round 3 every tile is quiescent: the
    kpend word alone. Option off: round 2's bytes in every round."""
    n, m = 4000, 1000
    for on in (1, 0):
        e = avhip.Engine(n, m, k=8, seed=1, log_capacity=1 << 22)
        e.set_option("quiet_tiles", on)
        e.init_records(avhip.INIT_ACCEPTED, 0)
        lanes = e.layout_info()["lanes"]
        tiles = (lanes + 63) // 64
        e.run_rounds(2)
        moved = []
        for r in (2, 3, 4, 5):
            b = e.alg_bytes()
            a = e.applied_votes()
            e.run_rounds(1)
            moved.append(e.alg_bytes() - b)
            assert e.applied_votes() - a == n * m * 8, (on, r)
            assert e.updates_count() == 0
        print("quiet_tiles", on, "bytes per round 2..5:", moved, "lanes", lanes, "tiles", tiles)
        assert moved[0] == lanes * 8 + tiles * 8, on
        for r, got in zip((3, 4, 5), moved[1:]):
            assert got == (tiles * 8 if on else lanes * 8 + tiles * 8), (on, r)
        e.close()


def life(n, m, rounds, seed, byz=0, opts=()):
    """One network's life with quiet_tiles on and off: per-round digests, byte and
    applied-vote counters, the final records, rows and finalizations."""
    out = []
    for on in (1, 0):
        eng = avhip.Engine(n, m, k=8, seed=seed, byz_threshold=byz, log_capacity=1 << 26)
        for name, v in opts:
            eng.set_option(name, v)
        eng.set_option("quiet_tiles", on)
        eng.init_records(avhip.INIT_BERNOULLI, P80)
        digests, nbytes, applied = [], [], []
        for _ in range(rounds):
            b0 = eng.alg_bytes()
            eng.run_rounds(1)
            nbytes.append(eng.alg_bytes() - b0)
            applied.append(eng.applied_votes())
            digests.append(eng.updates_digest())
            eng.discard_updates()
        out.append(dict(digests=digests, bytes=nbytes, applied=applied, rec=eng.read_records(), pref=eng.read_pref(),
                        fin=eng.finalized_count()))
        eng.close()
    return out


def same_life(on, off):
    assert on["digests"] == off["digests"]
    assert on["applied"] == off["applied"]
    np.testing.assert_array_equal(on["rec"], off["rec"])
    np.testing.assert_array_equal(on["pref"], off["pref"])
    assert on["fin"] == off["fin"]


def test_quiet_tiles_on_off_identical_and_taken():
    """20k x 1000 (C4's row shape), Bernoulli(0.8), honest, through convergence, the
    settled rounds and the finalization storm."""
    on, off = life(20_000, 1000, 22, seed=5)
    same_life(on, off)
    assert on["fin"] > 0
    print("bytes on ", on["bytes"])
    print("bytes off", off["bytes"])
    for r in range(8, 14):
        assert on["bytes"][r] < off["bytes"][r], r


@pytest.mark.parametrize("n,m,init", [(3000, 1000, avhip.INIT_BERNOULLI), (4000, 256, avhip.INIT_BERNOULLI),
                                      (1500, 64, avhip.INIT_ACCEPTED), (2000, 517, avhip.INIT_PAIRS),
                                      (3001, 1000, avhip.INIT_BERNOULLI)],
                         ids=["bl32", "bl8", "bl2_accepted", "ragged_pairs", "half_tile"])
def test_quiet_tiles_vs_oracle(oracle, n, m, init):
    """Disturbances inside the quiescent stretch; (3001, 1000): the last tile is half
    full and the tile count no multiple of the run length."""
    eng = avhip.Engine(n, m, k=8, seed=93, log_capacity=1 << 24)
    eng.init_records(init, P80)
    sim = oracle.Sim(n, m, 8, seed=93, init_mode=init, init_param=P80, threads=T)
    for r in range(26):
        if r == 10:  # a drop-in Response rewrites node 5's records and published row
            eng.register_votes(5, [0, 1, 2, 40 % m], [1, 1, 1, 1])
            sim.register_votes(5, [0, 1, 2, 40 % m], np.array([1, 1, 1, 1], np.uint32))
            eng.discard_updates()
        if r == 12:
            eng.set_valid(3, False)
            sim.set_valid(3, False)
        if r == 14:
            eng.set_valid(3, True)
            sim.set_valid(3, True)
        eng.run_rounds(1)
        exp, _ = sim.run_round(threads=T)
        assert rows(eng.fetch_updates()) == rows(exp), f"round {r}"
        if r in (9, 11, 15, 17, 23, 25):
            np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T), err_msg=f"round {r}")
        if r in (9, 10, 11):  # three rounds in a row: each of the three snapshot buffers
            np.testing.assert_array_equal(eng.read_pref(), sim.pref(), err_msg=f"rows after round {r}")
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


def test_quiet_tiles_add_targets_midrun(oracle):
    """An AddTargetToReconcile of dead records after finalization (records and a
    snapshot row rewritten outside the sweep); later rounds agree with the oracle."""
    n, m = 1200, 256
    eng = avhip.Engine(n, m, k=8, seed=7, log_capacity=1 << 24)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    sim = oracle.Sim(n, m, 8, seed=7, init_mode=avhip.INIT_ACCEPTED, init_param=0, threads=T)
    for r in range(24):
        if r == 20:  # every record finalized by now: re-add some as rejected
            got = eng.add_targets(11, [4, 5, 200], [False, False, False])
            exp = [sim.add(11, t, False) for t in (4, 5, 200)]
            assert list(map(bool, got)) == exp
        eng.run_rounds(1)
        e_exp, _ = sim.run_round(threads=T)
        assert rows(eng.fetch_updates()) == rows(e_exp), f"round {r}"
    np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T))
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


SHAPES = [(1, 1, 1000), (4, 1, 1000), (8, 1, 1000), (16, 1, 1000)] + [
    (tpw, merge, m) for tpw, merge in ((4, 4), (8, 2), (2, 8)) for m in (1000, 250, 125)]


@pytest.mark.parametrize("tpw,merge,m", SHAPES)
def test_quiet_tiles_run_shapes(tpw, merge, m):
    """Runs of 1, 4, 8 and 16 tiles, and merged runs (uni_merge) at C4's row shape and
    its target shards at 4 / 8 ranks (BL 8 / 4: up to 256 nodes per merged run)."""
    on, off = life(20_000, m, 20, seed=7, opts=(("tiles_per_wave", tpw), ("uni_merge", merge)))
    same_life(on, off)
    assert on["fin"] > 0
    assert sum(on["bytes"]) < sum(off["bytes"])


def test_quiet_tiles_byzantine_not_taken():
    """20 % Byzantine voters: their flip-flop rows keep every snapshot tagged, so no
    tile is quiescent: same results and the same bytes with the option on and off."""
    on, off = life(2500, 1000, 22, seed=11, byz=BYZ20)
    same_life(on, off)
    assert on["bytes"] == off["bytes"]


def test_quiet_tiles_call_boundaries(oracle):
    """Deferred and quiescent rounds carried over whole run_rounds calls."""
    n, m = 300, 640
    eng = avhip.Engine(n, m, k=8, seed=21, log_capacity=1 << 22)
    eng.init_records(3, P97)
    sim = oracle.Sim(n, m, 8, seed=21, init_mode=3, init_param=P97)
    exp = []
    for chunk in (3, 9, 4, 8):
        eng.run_rounds(chunk)
        exp += [sim.run_round()[0] for _ in range(chunk)]
    assert rows(eng.fetch_updates()) == rows(np.concatenate(exp))
    np.testing.assert_array_equal(eng.read_records(), sim.dump())
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


def epoch_protocol(on, mat_at=None):
    """The benchmark's epoch protocol: 12 rounds, the log dropped and the records
    re-initialised mid-flight, 12 more rounds, the write-back, a read."""
    n, m = 4000, 1000
    eng = avhip.Engine(n, m, k=8, seed=0xA7A1A9C4, log_capacity=1 << 26)
    eng.set_option("quiet_tiles", on)
    eng.init_records(avhip.INIT_BERNOULLI, P80)
    seen = []
    for epoch in range(2):
        for r in range(12):
            eng.run_rounds(1)
            if mat_at is not None and r == mat_at:
                eng.materialize()
        seen.append((eng.updates_digest(), eng.applied_votes(), eng.finalized_count()))
        if epoch == 0:
            b0 = eng.alg_bytes()
            eng.discard_updates()
            eng.init_records(avhip.INIT_BERNOULLI, P80)
    nbytes = eng.alg_bytes() - b0
    eng.materialize()
    rec, pref = eng.read_records(), eng.read_pref()
    eng.close()
    return seen, rec, pref, nbytes


def test_quiet_tiles_epoch_protocol():
    on = epoch_protocol(1)
    off = epoch_protocol(0)
    mat = epoch_protocol(1, mat_at=9)  # a write-back inside the quiescent stretch resets the streak
    for other in (off, mat):
        assert on[0] == other[0]
        np.testing.assert_array_equal(on[1], other[1])
        np.testing.assert_array_equal(on[2], other[2])
    assert on[3] < off[3], (on[3], off[3])  # the path was taken
    assert on[3] < mat[3], (on[3], mat[3])  # ... and left for the rounds after the write-back
