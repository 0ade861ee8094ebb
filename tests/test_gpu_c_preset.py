"""Preset consider planes (kernels.h c_preset) and the write-back's low count group (round_sweep.hip
materialize_tile), bit for bit against the oracle.

av_init_records stores the consider planes as all-ones where the next sim round is the fresh sweep
round; until that round has run they stand for consider = 0 on every record. Everything that reads
or writes records before it must see that: reads virtually (k_read_records_v), everything else after
the pass that stores the planes explicitly. Each case runs with option "c_preset" 1 and, for the old
path (kCAll), 0. Shapes: the smallest that reach every branch."""
import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
SEED = 0xC0FFEE
K = 8
M64 = 2**64 - 1

SHAPES = [
    (131, 1000),  # BL 32: stale vote planes; the last block holds 8 targets; lanes no multiple of 64
    (200, 512),   # BL 16: the vv_min_bl edge
    (64, 100),    # BL 4: uniform-only virtual votes
]
IDS = [f"n{n}m{m}" for n, m in SHAPES]


class Pair:
    """An engine and the oracle's network beside it."""

    def __init__(self, oracle, n, m, preset, init=True):
        self.oracle, self.n, self.m = oracle, n, m
        self.eng = avhip.Engine(n, m, k=K, seed=SEED, log_capacity=1 << 21)
        self.eng.set_option("c_preset", preset)
        self.sim = None
        if init:
            self.init()

    def init(self):
        self.eng.init_records(avhip.INIT_BERNOULLI, P80)
        if self.sim is not None:
            self.sim.close()
        self.sim = self.oracle.Sim(self.n, self.m, K, seed=SEED, init_mode=avhip.INIT_BERNOULLI, init_param=P80)
        self.sim.set_round_index(self.eng.round)

    def records(self):
        got = self.eng.read_records()
        assert np.array_equal(got, self.sim.dump())
        return got

    def rounds(self, r, replay=False):
        """r rounds on both sides: the pending StatusUpdates' digest, then the records."""
        eng, sim = self.eng, self.sim
        eng.fetch_updates()
        base = eng.log_base_round()
        first = eng.round
        if replay:
            eng.replay_prepare(r)
            eng.replay_rounds(r)
        else:
            eng.run_rounds(r)
        cnt = s = x = 0
        for i in range(r):
            errs = self.oracle.gen_replay_errs(SEED, first + i, 0, self.n, self.m, K) if replay else None
            (c, s_, x_), _ = sim.run_round(errs, collect=False, round_rel=first + i - base)
            cnt, s, x = cnt + c, (s + s_) & M64, x ^ x_
        assert eng.updates_digest() == (cnt, s, x)
        return self.records()

    def close(self):
        self.eng.close()
        self.sim.close()


@pytest.fixture(params=[1, 0], ids=["preset", "old"])
def preset(request):
    return request.param


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_read_after_init(oracle, shape, preset):
    p = Pair(oracle, *shape, preset)
    rec = p.records()
    assert not ((rec >> 8) & 0xFF).any()  # consider = 0 on every record
    assert np.array_equal(p.eng.read_records(), rec)  # a read leaves the form in place
    p.rounds(3)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_materialize_then_first_generation_rounds(oracle, shape, preset):
    """The first-generation kernel reads the stored consider planes: planes left all-ones would step
    the counts two votes early."""
    p = Pair(oracle, *shape, preset)
    p.eng.materialize()
    p.records()
    p.eng.set_option("kernel", 1)
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_first_generation_rounds_unmaterialized(oracle, shape, preset):
    """The same with no av_materialize: the round plan asks for the explicit planes."""
    p = Pair(oracle, *shape, preset)
    p.eng.set_option("kernel", 1)
    p.rounds(10)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_neutral_dropin_votes(oracle, shape, preset):
    n, m = shape
    p = Pair(oracle, n, m, preset)
    rng = np.random.default_rng(5)
    for node in (0, n // 2, n - 1):
        ts = np.sort(rng.choice(m, size=min(m, 48), replace=False))
        errs = rng.choice(np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32), ts.size)
        st = p.eng.register_votes(node, ts, errs)
        assert [(int(t), int(s)) for t, s in zip(ts, st) if s >= 0] == p.sim.register_votes(node, ts, errs)
    p.records()
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_add_targets(oracle, shape, preset):
    n, m = shape
    p = Pair(oracle, n, m, preset)
    assert not p.eng.add_targets(n - 1, [0, m - 1], [True, False]).any()  # live records: no-op
    assert not p.sim.add(n - 1, 0, True) and not p.sim.add(n - 1, m - 1, False)
    p.records()
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_write_records(oracle, shape, preset):
    n, m = shape
    p = Pair(oracle, n, m, preset)
    rng = np.random.default_rng(7)
    # arbitrary registers on a few rows (count < 100: live), the rest untouched
    w = rng.integers(0, 1 << 16, size=(5, m), dtype=np.uint32) | (rng.integers(0, 200, size=(5, m), dtype=np.uint32) << 16)
    p.eng.write_records(w, n0=3, t0=0)
    p.sim.write_records(w, n0=3, t0=0)
    p.records()
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_replay_rounds(oracle, shape, preset):
    p = Pair(oracle, *shape, preset)
    p.rounds(2, replay=True)
    p.rounds(6)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_invalid_targets_store_consider_in_the_fresh_round(oracle, shape, preset):
    n, m = shape
    p = Pair(oracle, n, m, preset)
    for t in (0, 33, m - 1):
        p.eng.set_valid(t, False)
        p.sim.set_valid(t, False)
    p.records()
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_option_fresh_off(oracle, shape, preset):
    p = Pair(oracle, *shape, preset)
    p.eng.set_option("fresh", 0)
    p.records()
    p.rounds(1)
    p.rounds(9)
    p.close()


@pytest.mark.parametrize("run", [1, 4], ids=["run1", "run4"])
@pytest.mark.parametrize("r", [1, 5, 9, 12])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rounds_then_materialize(oracle, shape, r, run, preset):
    """r sweep rounds, then the write-back: the records stay what a read saw before it (and the
    oracle's), and first-generation rounds, which read every stored plane, go on from them. The
    pending step counts the tiles hold after r rounds are even and odd: both forms of the write-back's
    count groups."""
    p = Pair(oracle, *shape, preset)
    p.eng.set_option("materialize_run", run)
    before = p.rounds(r)
    p.eng.materialize()
    assert np.array_equal(p.eng.read_records(), before)
    p.eng.set_option("kernel", 1)
    p.rounds(4)
    p.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_second_init(oracle, shape, preset):
    """A second av_init_records on an engine whose planes are still preset, and one after rounds."""
    p = Pair(oracle, *shape, preset)
    p.init()
    rec = p.records()
    assert not ((rec >> 8) & 0xFF).any()
    p.eng.materialize()
    p.eng.set_option("kernel", 1)
    p.rounds(3)
    p.eng.set_option("kernel", 2)
    p.init()
    p.rounds(6)
    p.init()
    p.rounds(2, replay=True)
    p.close()
