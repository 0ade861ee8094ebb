"""Calm tiles (sweep_tile.h process_tile, sweep_settled.h; option calm_tiles, default on): a general tile of a klazy
round that leaves its vote planes unstored and is not settled flags itself kVCalm when every
polled record has at most one of the round's slots 1..7 (next round's V6..V0) differing from
its final accepted bit. The next klazy round takes such a tile as a settled candidate: if its 8
new votes all equal A, every 8-vote window holds at most one disagreement, so every slot is a
conclusive agreeing vote (count + 8, no flip, no update) with no regather and no slot network.

Checked: option on against off after every round of a network's life (records, rows, digest,
applied votes, finalizations) with the byte counter showing the path; a directed all-accepted
network with one to three flip-flop voters against the oracle; API calls placed right after
the round that leaves calm tiles; the shapes and options that must not take the path; a serial
peer group of two ranks; the benchmark's epoch protocol."""
import hashlib
import os

import numpy as np
import pytest

import avhip
import shard_parties as sp

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
T = max(1, min(8, os.cpu_count() or 1))
LIFE_ROUNDS = 22  # through kconsume (round 16) and the finalization storm


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def same_updates(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if len(got):
        got = got[np.lexsort(got.T[::-1])]
        exp = exp[np.lexsort(exp.T[::-1])]
    np.testing.assert_array_equal(got, exp, err_msg=what)


def life(n, m, rounds, seed, calm, k=8, byz=0, opts=(), init=(avhip.INIT_BERNOULLI, P80), toggle=False):
    """One network's life; after every round: the bytes it moved and everything a caller can see."""
    eng = avhip.Engine(n, m, k=k, seed=seed, byz_threshold=byz, log_capacity=1 << 26)
    for name, v in opts:
        eng.set_option(name, v)
    if toggle:
        eng.set_option("calm_tiles", 1)
    eng.set_option("calm_tiles", calm)
    eng.init_records(*init)
    nbytes, seen = [], []
    for _ in range(rounds):
        b0 = eng.alg_bytes()
        eng.run_rounds(1)
        nbytes.append(eng.alg_bytes() - b0)
        seen.append((digest(eng.read_records()), digest(eng.read_pref()), eng.updates_digest(), eng.applied_votes(),
                     eng.finalized_count()))
        eng.discard_updates()
    eng.close()
    return nbytes, seen


def assert_same(on, off, what):
    for r, (a, b) in enumerate(zip(on[1], off[1])):
        assert a == b, f"{what}: round {r} differs (records, rows, digest, applied, finalized): {a} vs {b}"


def assert_taken(on, off, what):
    """No round moves more bytes with the option on (the 4 B of a newly settled tile's word are
    far below what its regather costs, so the plain inequality holds too), and one moves fewer."""
    print(what, "bytes on ", on[0])
    print(what, "bytes off", off[0])
    for r, (a, b) in enumerate(zip(on[0], off[0])):
        assert a <= b, f"{what}: round {r} moves {a} B with calm tiles, {b} B without"
    assert any(a < b for a, b in zip(on[0], off[0])), f"{what}: the path was never taken"


@pytest.mark.parametrize("tpw", [1, 4, 16])
@pytest.mark.parametrize("n,m", [(4096, 1000), (4097, 1000), (4096, 512), (4097, 512)],
                         ids=["bl32", "bl32_half_tile", "bl16", "bl16_half_tile"])
def test_calm_on_off_identical_and_taken(n, m, tpw):
    """Bernoulli(0.8) through convergence (the calm stretch is rounds 3-5), the settled rounds,
    kconsume and the finalization storm, at runs of 1, 4 and 16 tiles per wave."""
    opts = (("tiles_per_wave", tpw),)
    on = life(n, m, LIFE_ROUNDS, seed=5, calm=1, opts=opts)
    off = life(n, m, LIFE_ROUNDS, seed=5, calm=0, opts=opts)
    assert_same(on, off, f"{n}x{m} tpw {tpw}")
    assert on[1][-1][4] > 0  # finalizations were reached
    assert_taken(on, off, f"{n}x{m} tpw {tpw}")


def few_voters(oracle, n, seed0=1):
    """An engine seed and Byzantine threshold that give one to three flip-flop voters, by the
    draw the engine itself makes (avo_byz_words restates it)."""
    thr = int(2.0 / n * 2**32)
    for seed in range(seed0, seed0 + 8):
        cnt = int(sum(bin(int(w)).count("1") for w in oracle.byz_words(seed, n, thr)))
        if 1 <= cnt <= 3:
            return seed, thr, cnt
    return None


def test_calm_one_dissenter(oracle):
    """All-accepted honest network with one to three flip-flop voters. An honest node that drew a
    voter in one round (while its pattern disagreed) carries exactly one stray vote on every
    record: its tile is calm and settles in the next round through settled_run / settled_tile
    with no regather. A node that drew a voter in two rounds running carries two strays and
    takes the general path. Every round against the oracle, and option on against off."""
    n, m, rounds = 1024, 1000, 12
    found = few_voters(oracle, n)
    if found is None:
        pytest.skip("no seed in the range gives one to three Byzantine voters")
    seed, thr, cnt = found
    sim = oracle.Sim(n, m, 8, seed=seed, byz_threshold=thr, init_mode=avhip.INIT_ACCEPTED, init_param=0, threads=T)
    honest = [j for j in range(n) if not sim.is_byzantine(j)]  # a voter's row is its pattern, not its records
    exp = []
    for _ in range(rounds):
        u, _ = sim.run_round(threads=T)
        exp.append((u, sim.dump(threads=T), sim.pref()[honest]))
    out = {}
    for calm in (1, 0):
        eng = avhip.Engine(n, m, k=8, seed=seed, byz_threshold=thr, log_capacity=1 << 24)
        eng.set_option("calm_tiles", calm)
        eng.init_records(avhip.INIT_ACCEPTED, 0)
        nbytes = []
        for r in range(rounds):
            b0 = eng.alg_bytes()
            eng.run_rounds(1)
            nbytes.append(eng.alg_bytes() - b0)
            same_updates(eng.fetch_updates(), exp[r][0], f"calm {calm} round {r} updates")
            np.testing.assert_array_equal(eng.read_records(), exp[r][1], err_msg=f"calm {calm} round {r} records")
            np.testing.assert_array_equal(eng.read_pref()[honest], exp[r][2], err_msg=f"calm {calm} round {r} rows")
        out[calm] = nbytes
        eng.close()
    print(f"seed {seed}: {cnt} voters; bytes on {out[1]}; off {out[0]}")
    for r in range(rounds):
        assert out[1][r] <= out[0][r], r
    assert sum(out[1]) < sum(out[0]), "no tile with one stray vote settled without its regather"


def first_calm_round(n, m, seed):
    """The first round (0-based) that consumes calm tiles: the first that moves fewer bytes with
    the option on. The round before it left them."""
    on = life(n, m, 8, seed, calm=1)
    off = life(n, m, 8, seed, calm=0)
    assert_same(on, off, "scout")
    for r, (a, b) in enumerate(zip(on[0], off[0])):
        if a < b:
            return r
    raise AssertionError(f"no round takes calm tiles: {on[0]} / {off[0]}")


WRITERS = ["set_valid", "add_targets", "dropin_vote", "materialize", "read_records"]


@pytest.fixture(scope="module")
def stretch():
    """512 x 1000, Bernoulli(0.8): the round that first consumes calm tiles, found once."""
    n, m, seed = 512, 1000, 9
    return n, m, seed, first_calm_round(n, m, seed)


@pytest.mark.parametrize("writer", WRITERS)
def test_calm_writers_inside_the_stretch(oracle, stretch, writer):
    """An API call between the round that leaves calm tiles and the round that would take them:
    the write-back and the virtual read see a calm tile as a stale one. Four more rounds against
    the oracle."""
    n, m, seed, c = stretch
    eng = avhip.Engine(n, m, k=8, seed=seed, log_capacity=1 << 24)
    eng.init_records(avhip.INIT_BERNOULLI, P80)
    sim = oracle.Sim(n, m, 8, seed=seed, init_mode=avhip.INIT_BERNOULLI, init_param=P80, threads=T)
    eng.run_rounds(c)
    for _ in range(c):
        sim.run_round(threads=T, collect=False)
    eng.discard_updates()
    if writer == "set_valid":
        eng.set_valid(3, False)
        sim.set_valid(3, False)
    elif writer == "add_targets":
        got = eng.add_targets(11, [4, 5, 200], [False, True, False])
        assert list(map(bool, got)) == [sim.add(11, t, a) for t, a in ((4, False), (5, True), (200, False))]
    elif writer == "dropin_vote":
        eng.register_votes(5, [0, 1, 2, 40], [1, 0, 1, 1])
        sim.register_votes(5, [0, 1, 2, 40], np.array([1, 0, 1, 1], np.uint32))
        eng.discard_updates()
    elif writer == "materialize":
        eng.materialize()
    elif writer == "read_records":
        np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T), err_msg="virtual read of calm tiles")
    for r in range(c, c + 4):
        eng.run_rounds(1)
        exp, _ = sim.run_round(threads=T)
        same_updates(eng.fetch_updates(), exp, f"{writer}: round {r}")
        np.testing.assert_array_equal(eng.read_records(), sim.dump(threads=T), err_msg=f"{writer}: round {r}")
    np.testing.assert_array_equal(eng.read_pref(), sim.pref())
    eng.close()


@pytest.mark.parametrize("what,kw", [
    ("k5", dict(k=5)),
    ("kernel1", dict(opts=(("kernel", 1),))),
    ("bl8_below_vv_min_bl", dict(m=256)),
    ("calm_tiles_0", dict(toggle=True)),
])
def test_calm_not_taken(what, kw):
    """k < 8, the first-generation kernel, rows below vv_min_bl (uniform form only, no stale
    tile) and the option switched on and off again: the same bytes in every round as with the
    option off, and the same results."""
    kw = dict(kw)
    m = kw.pop("m", 1000)
    calm = 0 if what == "calm_tiles_0" else 1
    on = life(2048, m, 12, seed=5, calm=calm, **kw)
    off = life(2048, m, 12, seed=5, calm=0, **{k: v for k, v in kw.items() if k != "toggle"})
    assert_same(on, off, what)
    assert on[0] == off[0], (what, on[0], off[0])
    if what == "calm_tiles_0":  # ... where the option left on does take the path
        assert sum(life(2048, m, 12, seed=5, calm=1)[0]) < sum(off[0])


def group_life(n, m, rounds, seed, calm, mode, world=2, keep_updates=False):
    per = n // world
    g = sp.PeerGroup([avhip.Engine(n, m, k=8, seed=seed, node_range=(r * per, (r + 1) * per), log_capacity=1 << 26)
                      for r in range(world)], avhip)
    for name, v in mode:
        g.set_option(name, v)
    g.set_option("calm_tiles", calm)
    g.init_records(avhip.INIT_BERNOULLI, P80)
    g.group()
    nbytes, seen, ups = [], [], []
    for r in range(rounds):
        b0 = g.alg_bytes()
        g.run_rounds(1)
        nbytes.append(g.alg_bytes() - b0)
        rec, pref = g.read_records(), g.read_pref()
        seen.append((digest(rec), digest(pref), g.updates_digest(), g.applied_votes(), g.finalized_count()))
        if keep_updates:
            ups.append(g.fetch_updates())
        else:
            g.discard_updates()
    g.close()
    return nbytes, seen, ups, rec, pref


@pytest.fixture(scope="module")
def oracle_life(oracle):
    """The first 8 rounds of 4096 x 1000, Bernoulli(0.8), seed 5: computed once."""
    n, m = 4096, 1000
    sim = oracle.Sim(n, m, 8, seed=5, init_mode=avhip.INIT_BERNOULLI, init_param=P80, threads=T)
    ups = [sim.run_round(threads=T)[0] for _ in range(8)]
    return ups, sim.dump(threads=T), sim.pref()


@pytest.mark.parametrize("mode", [(), (("peer_mask", 0),)], ids=["masked", "full"])
def test_calm_peer_group(oracle_life, mode):
    """A serial peer group of two ranks (the counting / peer-push build of the sweep): on against
    off through the calm stretch and the settled rounds, and 8 rounds against the oracle."""
    n, m = 4096, 1000
    on = group_life(n, m, 12, 5, 1, mode)
    off = group_life(n, m, 12, 5, 0, mode)
    assert_same(on, off, f"peer group {mode}")
    assert_taken(on, off, f"peer group {mode}")
    ups, rec, pref = oracle_life
    par = group_life(n, m, 8, 5, 1, mode, keep_updates=True)
    for r in range(8):
        same_updates(par[2][r], ups[r], f"peer group {mode}: round {r}")
    np.testing.assert_array_equal(par[3], rec)
    np.testing.assert_array_equal(par[4], pref)


def epoch_protocol(calm, mat_at=None):
    """The benchmark's epoch protocol: 12 rounds, the log dropped and the records re-initialised
    mid-flight, 12 more rounds, the write-back, a read."""
    n, m = 4096, 1000
    eng = avhip.Engine(n, m, k=8, seed=0xA7A1A9C4, log_capacity=1 << 26)
    eng.set_option("calm_tiles", calm)
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


def test_calm_epoch_protocol():
    on = epoch_protocol(1)
    off = epoch_protocol(0)
    # a write-back right after the round that leaves calm tiles (found, not assumed): the flags go
    # with it, so the round after regathers as with the option off
    c = first_calm_round(4096, 1000, 0xA7A1A9C4)
    assert c >= 1
    mat = epoch_protocol(1, mat_at=c - 1)
    for other in (off, mat):
        assert on[0] == other[0]
        np.testing.assert_array_equal(on[1], other[1])
        np.testing.assert_array_equal(on[2], other[2])
    assert on[3] < off[3], (on[3], off[3])  # the path was taken
    assert on[3] < mat[3], (on[3], mat[3])  # ... and the write-back did fall inside the stretch
