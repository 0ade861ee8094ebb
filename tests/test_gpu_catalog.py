"""The engine's Hash catalog on the GPU: the caller's 64-bit hashes (avalanche.go:71) interned into
target slots by a deterministic rule (call order, lowest free slot) that a dict model reproduces, the
device table probed by the lookup kernel (catalog.hip) against the host map, slots recycled once no
node holds a record, and av_register_votes_hashed against the oracle and against a twin engine fed
the translated slots through av_register_votes_batch."""
import os
import subprocess

import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

ERRS = np.array([0, 0, 0, 0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
I64 = np.iinfo(np.int64)
EDGE = [0, -1, I64.min, I64.max, I64.min + 1, I64.max - 1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Model:
    """The slot rule: hashes interned in call order, a new one takes the lowest free slot."""

    def __init__(self, t0, t1):
        self.slot_of, self.free = {}, set(range(t0, t1))

    def intern(self, hashes):
        out = []
        for h in map(int, hashes):
            if h not in self.slot_of and self.free:
                s = min(self.free)
                self.free.remove(s)
                self.slot_of[h] = s
            out.append(self.slot_of.get(h, -1))
        return out

    def find(self, hashes):
        return [self.slot_of.get(int(h), -1) for h in hashes]

    def retire(self, h):
        self.free.add(self.slot_of.pop(int(h)))


def rand_hashes(rng, n):
    return rng.integers(I64.min, I64.max, size=n, dtype=np.int64, endpoint=True)


def code_of(fn):
    with pytest.raises(avhip.AvError) as ei:
        fn()
    return ei.value.code


def check_catalog(eng, model, queries, where=""):
    exp = model.find(queries)
    assert eng.catalog_find(queries).tolist() == exp, where
    assert eng.catalog_find_device(queries).tolist() == exp, where


@pytest.mark.parametrize("m,opts", [(64, {}), (33, {}), (64, {"catalog_lds": 0}), (1100, {})],
                         ids=["m64", "m33", "m64_global", "m1100_global"])
def test_lookup_parity(m, opts):
    """find_device == find == the model for queries of every size class (more than one pass of the
    grid included), with the table in LDS (M <= 1024) and in global memory."""
    rng = np.random.default_rng(m)
    eng = avhip.Engine(8, m, k=8, seed=3)
    for k, v in opts.items():
        eng.set_option(k, v)
    model = Model(0, m)
    assert eng.catalog_find(EDGE).tolist() == eng.catalog_find_device(EDGE).tolist() == [-1] * len(EDGE)
    h0, u0 = eng.catalog_hashes()
    assert h0.shape == u0.shape == (m,) and not u0.any()
    # edge keys, keys equal to slot numbers (not their own slots), random keys, until full and past it
    keys = np.concatenate([np.array(EDGE + [5, 3, m - 1, m, 32, 31], np.int64), rand_hashes(rng, m + 40)])
    seen = []
    for a in range(0, keys.size, 17):
        part = np.concatenate([keys[a:a + 17], keys[a:a + 3], keys[:2]])  # duplicates inside one call
        assert eng.catalog_intern(part).tolist() == model.intern(part), a
        seen += part.tolist()
    assert not model.free and -1 in model.find(keys)
    assert eng.catalog_intern(keys[-5:]).tolist() == [-1] * 5 == model.intern(keys[-5:])
    hs, used = eng.catalog_hashes()
    assert used.all() and {int(h): s for s, h in enumerate(hs)} == model.slot_of
    pool = np.concatenate([np.array(seen, np.int64), rand_hashes(rng, 200), np.arange(-4, m + 4)])
    for size in (0, 1, 63, 64, 65, 100_000):
        q = rng.choice(pool, size) if size else np.zeros(0, np.int64)
        check_catalog(eng, model, q, size)
    eng.set_option("catalog_blocks", 3)  # 1536 hashes per pass of the grid: 100 000 takes 66
    q = rng.choice(pool, 100_000)
    q[::2] = np.roll(q, 1)[::2]  # runs of repeated hashes
    check_catalog(eng, model, q, "small grid")
    check_catalog(eng, model, q[:1537], "one pass and one hash")
    eng.close()


@pytest.mark.parametrize("m", [64, 33])
def test_churn(m):
    """2000 interleaved retire / intern operations on slots written absent: the device table follows
    the host map through patches, tombstones and rebuilds."""
    rng = np.random.default_rng(100 + m)
    n = 8
    eng = avhip.Engine(n, m, k=8, seed=4)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    eng.write_records(np.full((n, m), avhip.ABSENT_WORD, np.uint32))
    model = Model(0, m)
    seen = list(EDGE)
    assert eng.catalog_intern(seen).tolist() == model.intern(seen)
    for op in range(2000):
        live = list(model.slot_of)
        if live and (rng.random() < 0.5 or not model.free):
            h = live[int(rng.integers(0, len(live)))]
            assert eng.catalog_retire([h]).tolist() == [True], op
            model.retire(h)
        else:
            h = int(rand_hashes(rng, 1)[0]) if rng.random() < 0.7 else seen[int(rng.integers(0, len(seen)))]
            seen.append(h)
            assert eng.catalog_intern([h]).tolist() == model.intern([h]), op
        if op % 50 == 49:
            check_catalog(eng, model, np.array(seen, np.int64), op)
    hs, used = eng.catalog_hashes()
    assert {int(h): s for s, (h, u) in enumerate(zip(hs, used)) if u} == model.slot_of
    eng.close()


def test_retire():
    n, m = 16, 64
    eng = avhip.Engine(n, m, k=8, seed=5)
    A, B, C, D = 1234567890123, -5, I64.min, 77
    sa, sb, sc = eng.catalog_intern([A, B, C]).tolist()
    assert (sa, sb, sc) == (0, 1, 2)
    assert eng.catalog_retire([A, B, C, D], commit=False).tolist() == [True, True, True, False]  # no records at all
    assert eng.add_targets(3, [sa], [1]).tolist() == [True]  # one live record on one node
    assert eng.catalog_retire([A, A, D], commit=False).tolist() == [False, False, False]
    eng.set_valid(sa, False)  # a record of an invalid target is still a record
    assert eng.catalog_retire([A]).tolist() == [False] and eng.catalog_find([A]).tolist() == [sa]
    eng.write_records(np.full((1, 1), avhip.ABSENT_WORD, np.uint32), n0=3, t0=sa)
    assert eng.catalog_retire([A], commit=False).tolist() == [True]
    assert eng.catalog_find([A]).tolist() == eng.catalog_find_device([A]).tolist() == [sa]  # commit = 0 changes nothing
    # StatusUpdates pending: every node finalizes B's slot
    assert (eng.admit_targets([sb], avhip.INIT_ACCEPTED) == n).all()
    for _ in range(40):
        eng.run_rounds(1)
        if eng.finalized_count() == n:
            break
    assert eng.finalized_count() == n and eng.updates_count() > 0
    assert code_of(lambda: eng.catalog_retire([A])) == avhip.AV_ERR_UNSUPPORTED
    assert eng.catalog_find([A, B]).tolist() == eng.catalog_find_device([A, B]).tolist() == [sa, sb]
    assert eng.catalog_retire([A, B], commit=False).tolist() == [True, True]  # asking is allowed
    assert len(eng.fetch_updates()) > 0
    assert eng.catalog_retire([B, A, B, D, A]).tolist() == [True, True, True, False, True]
    assert eng.catalog_find([A, B, C]).tolist() == eng.catalog_find_device([A, B, C]).tolist() == [-1, -1, sc]
    hs, used = eng.catalog_hashes()
    assert used.tolist() == [False, False, True] + [False] * (m - 3) and hs[2] == C
    # a new hash in the freed slot whose validity was off: valid again
    assert eng.catalog_intern([D]).tolist() == [sa]
    assert eng.add_targets(2, [sa], [1]).tolist() == [True]
    assert sa in eng.get_invs(2).tolist()
    eng.close()


def hashed_batch(rng, n, m, hashes, mode):
    """A batch in the shape of test_register_votes_batch_vs_oracle's, as slots (-1 = a hash that is
    not catalogued) and as the hashes that stand for them."""
    n_resp = int(rng.integers(1, 60))
    nodes = rng.integers(0, n, size=n_resp)
    parts = []
    for r in range(n_resp):
        size = int(rng.integers(0, 200))
        if mode == "random":
            t = rng.integers(-3, m + 3, size=size)
            t[rng.random(size) < 0.1] = -1
        else:  # slot-ascending, uncatalogued hashes before and after (gaps: anywhere in between too)
            t = np.sort(rng.choice(np.arange(-3, m + 3), size=size, replace=False))
            if mode == "gaps":
                t = np.insert(t, np.sort(rng.integers(0, size + 1, size // 8)), -1)
        parts.append(t)
    if mode == "reversed" and n_resp:
        parts[n_resp // 2] = parts[n_resp // 2][::-1].copy()
    offsets = np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int64)
    slots = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    known = (slots >= 0) & (slots < m)
    slots[~known] = -1
    hs = rand_hashes(rng, slots.size)  # uncatalogued with overwhelming probability; checked by the caller
    hs[known] = hashes[slots[known]]
    errs = rng.choice(ERRS, size=slots.size)
    return nodes, offsets, slots, hs, errs


@pytest.mark.parametrize("seed,mode", [(11, "random"), (12, "random"), (13, "ascending"), (14, "gaps"),
                                       (15, "reversed")])
def test_register_votes_hashed_vs_oracle(oracle, seed, mode):
    """The protocol of test_register_votes_batch_vs_oracle with the targets random 64-bit hashes:
    statuses per Response == the oracle's RegisterVotes on the translated slots; records and
    statuses bit-identical to a twin fed the slots, with dropin_fast 1 and 0."""
    rng = np.random.default_rng(seed)
    n, m = 40, 300
    hashes = rand_hashes(rng, m)
    assert len(set(hashes.tolist())) == m
    engs = [avhip.Engine(n, m, k=8, seed=seed) for _ in range(3)]  # hashed fast, hashed general, twin (slots)
    engs[1].set_option("dropin_fast", 0)
    sim = oracle.Sim(n, m, 8, seed=seed, init_mode=3, init_param=int(0.6 * 2**32))
    for e in engs:
        e.init_records(avhip.INIT_BERNOULLI, int(0.6 * 2**32))
    for e in engs[:2]:
        assert e.catalog_intern(hashes).tolist() == list(range(m))
    for t in (7, 100):
        sim.set_valid(t, False)
        for e in engs:
            e.set_valid(t, False)
    for _ in range(16):  # records close to 128: batches finalize some of them
        for e in engs:
            e.run_rounds(1)
        sim.run_round()
    for e in engs:
        e.discard_updates()
    for batch in range(8):
        nodes, offsets, slots, hs, errs = hashed_batch(rng, n, m, hashes, mode)
        assert (engs[0].catalog_find(hs) == slots).all()
        got = [e.register_votes_hashed(nodes, offsets, hs, errs) for e in engs[:2]]
        twin = engs[2].register_votes_batch(nodes, offsets, slots, errs)
        assert np.array_equal(got[0], twin) and np.array_equal(got[1], twin), batch
        assert (twin[slots < 0] == -1).all()
        for i in range(len(nodes)):
            a, b = int(offsets[i]), int(offsets[i + 1])
            kn = slots[a:b] >= 0
            exp = sim.register_votes(int(nodes[i]), slots[a:b][kn], errs[a:b][kn])
            have = [(int(slots[v]), int(twin[v])) for v in range(a, b) if twin[v] >= 0]
            assert have == exp, (batch, i)
        dump = sim.dump()
        for e in engs:
            assert np.array_equal(e.read_records(), dump), batch
    exp_u, _ = sim.run_round()
    for e in engs:
        e.run_rounds(1)
        assert np.array_equal(e.fetch_updates(), exp_u)
        e.close()


def test_register_votes_hashed_device_grouping(oracle):
    """One batch of >= 65536 hashed votes down the sort-grouped path, then a sim round."""
    rng = np.random.default_rng(77)
    n, m = 300, 700
    hashes = rand_hashes(rng, m)
    eng = avhip.Engine(n, m, k=8, seed=77)
    eng.init_records(avhip.INIT_BERNOULLI, int(0.6 * 2**32))
    sim = oracle.Sim(n, m, 8, seed=77, init_mode=3, init_param=int(0.6 * 2**32))
    assert eng.catalog_intern(hashes).tolist() == list(range(m))
    eng.set_valid(11, False)
    sim.set_valid(11, False)
    for _ in range(14):
        eng.run_rounds(1)
        sim.run_round()
    eng.discard_updates()
    n_resp = 900
    nodes = rng.integers(0, n, size=n_resp)
    offsets = np.concatenate([[0], np.cumsum(rng.integers(0, 200, size=n_resp))]).astype(np.int64)
    assert offsets[-1] >= 1 << 16
    slots = rng.integers(-3, m + 3, size=int(offsets[-1]))
    known = (slots >= 0) & (slots < m)
    slots[~known] = -1
    hs = rand_hashes(rng, slots.size)
    hs[known] = hashes[slots[known]]
    errs = rng.choice(ERRS, size=slots.size)
    got = eng.register_votes_hashed(nodes, offsets, hs, errs)
    for i in range(n_resp):
        a, b = int(offsets[i]), int(offsets[i + 1])
        kn = slots[a:b] >= 0
        exp = sim.register_votes(int(nodes[i]), slots[a:b][kn], errs[a:b][kn])
        assert [(int(slots[v]), int(got[v])) for v in range(a, b) if got[v] >= 0] == exp, i
    assert np.array_equal(eng.read_records(), sim.dump())
    eng.run_rounds(1)
    exp_u, _ = sim.run_round()
    assert np.array_equal(eng.fetch_updates(), exp_u)
    eng.close()


def test_slot_reuse_end_to_end(oracle):
    """A stream of transactions through a full catalog: A finalizes everywhere, is retired, B takes
    its slot, is admitted and voted on; votes on A no longer reach anything. The oracle runs on slots."""
    n, m, seed = 64, 32, 21
    rng = np.random.default_rng(seed)
    eng = avhip.Engine(n, m, k=8, seed=seed)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    sim = oracle.Sim(n, m, 8, seed=seed, init_mode=avhip.INIT_ACCEPTED, init_param=0)
    hashes = rand_hashes(rng, m + 1)
    A, B, slot = int(hashes[9]), int(hashes[m]), 9
    assert eng.catalog_intern(hashes).tolist() == list(range(m)) + [-1]  # full: B has to wait
    assert eng.catalog_retire([A], commit=False).tolist() == [False]
    for r in range(60):
        if eng.finalized_count() == n * m:
            break
        eng.run_rounds(1)
        exp_u, _ = sim.run_round()
        assert np.array_equal(eng.fetch_updates(), exp_u), r
    assert eng.finalized_count() == n * m and eng.updates_count() == 0
    assert eng.catalog_retire([A]).tolist() == [True]
    assert eng.catalog_intern([B]).tolist() == [slot]
    assert (eng.admit_targets([slot], avhip.INIT_REJECTED) == n).all()
    for node in range(n):
        assert sim.add(node, slot, 0)
    nodes = np.array([3, 5, 3, 60], np.int64)
    offsets = np.array([0, 3, 5, 9, 10], np.int64)
    hs = np.array([A, B, A, B, B, A, A, B, hashes[2], B], np.int64)
    errs = np.array([0, 0, 1, 1, 0, 0, 0, 0, 0, 0x80000000], np.uint32)
    got = eng.register_votes_hashed(nodes, offsets, hs, errs)
    assert (got[hs == A] == -1).all()
    for i in range(len(nodes)):
        a, b = int(offsets[i]), int(offsets[i + 1])
        sl = np.array(eng.catalog_find(hs[a:b]))
        exp = sim.register_votes(int(nodes[i]), sl[sl >= 0], errs[a:b][sl >= 0])
        assert [(int(sl[v - a]), int(got[v])) for v in range(a, b) if got[v] >= 0] == exp, i
    assert np.array_equal(eng.read_records(), sim.dump())
    assert ((eng.read_records()[:, slot] >> 17) < 128).all()  # B's records live
    eng.run_rounds(1)
    exp_u, _ = sim.run_round()
    assert np.array_equal(eng.fetch_updates(), exp_u)
    eng.close()


def test_target_shard(oracle):
    """A target shard's catalog hands out its own range; hashes of another shard are skipped."""
    n, m, seed = 8, 130, 31
    rng = np.random.default_rng(seed)
    eng = avhip.Engine(n, m, k=8, seed=seed, target_range=(32, 96))
    low = avhip.Engine(n, m, k=8, seed=seed, target_range=(0, 32))
    sim = oracle.Sim(n, m, 8, seed=seed, init_mode=avhip.INIT_ACCEPTED, init_param=0)
    for e in (eng, low):
        e.init_records(avhip.INIT_ACCEPTED, 0)
    hashes = rand_hashes(rng, 70)
    other = rand_hashes(rng, 10)
    assert eng.catalog_intern(hashes).tolist() == list(range(32, 96)) + [-1] * 6
    assert low.catalog_intern(other).tolist() == list(range(10))
    hs, used = eng.catalog_hashes()
    assert hs.tolist() == hashes[:64].tolist() and used.all()
    q = np.concatenate([hashes, other])
    exp = list(range(32, 96)) + [-1] * 16
    assert eng.catalog_find(q).tolist() == eng.catalog_find_device(q).tolist() == exp
    nodes = np.array([1, 6, 1], np.int64)
    offsets = np.array([0, 30, 50, 86], np.int64)
    votes = rng.choice(q, 86)
    errs = rng.choice(ERRS, 86)
    got = eng.register_votes_hashed(nodes, offsets, votes, errs)
    slots = np.array(eng.catalog_find(votes))
    assert (slots >= 0).any() and (slots < 0).any() and (got[slots < 0] == -1).all()
    for i in range(3):
        a, b = int(offsets[i]), int(offsets[i + 1])
        kn = slots[a:b] >= 0
        exp = sim.register_votes(int(nodes[i]), slots[a:b][kn], errs[a:b][kn])
        assert [(int(slots[v]), int(got[v])) for v in range(a, b) if got[v] >= 0] == exp, i
    assert np.array_equal(eng.read_records(), sim.dump()[:, 32:96])
    eng.close()
    low.close()


def test_serial_peer_group(oracle):
    """On a peer-push engine the catalog calls work and the hashed votes are refused like every record
    write outside a round."""
    n, m = 64, 70
    engs = [avhip.Engine(n, m, k=8, seed=11, node_range=(r * 32, (r + 1) * 32)) for r in range(2)]
    for e in engs:
        e.init_records(avhip.INIT_ACCEPTED, 0)
    avhip.peer_group_serial(engs)
    sim = oracle.Sim(n, m, 8, seed=11, init_mode=avhip.INIT_ACCEPTED, init_param=0)
    hs = np.array(EDGE + [99], np.int64)
    for e in engs:
        lo = e.node_range[0]
        assert e.catalog_intern(hs).tolist() == list(range(len(hs)))
        assert e.catalog_find_device([99, 98, 0]).tolist() == e.catalog_find([99, 98, 0]).tolist() == [6, -1, 0]
        assert e.catalog_retire(hs, commit=False).tolist() == [False] * len(hs)  # every node holds records
        assert code_of(lambda: e.register_votes_hashed([lo], [0, 2], [99, 0], [0, 0])) == avhip.AV_ERR_UNSUPPORTED
    assert np.array_equal(np.concatenate([e.read_records() for e in engs]), sim.dump())
    engs[0].close()


def test_cpp_mirror_catalog():
    """Engine::RegisterVotesBatch, Engine::Retire and more hashes than slots over an engine's life in
    the C++ mirror (host/avalanche_catalog_tests.cpp)."""
    exe = os.path.join(ROOT, "go-avalanche_amd", "bin", "avalanche_catalog_tests")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("RegisterVotesBatch", "Retire", "HashStream"):
        assert f"PASS {name}" in r.stdout
