"""The drop-in write batches at the sizes where their buffer layout (csrc/batch_layout.h) changes
shape: m = 1 .. 257 entries in 1 .. 3 Responses, every call kind on both of its paths, on one engine
whose scratch is therefore carved large, small and large again. Every call is checked against the
oracle: the statuses or added flags it returns and the records it leaves. A layout that lets two
regions share memory reads as wrong results here; the extents are tests/test_batch_layout_cpu.py's."""
import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

N, M = 6, 70  # three blocks per node, the last one partial
ERRS = np.array([0, 0, 0, 0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
I64 = np.iinfo(np.int64)
# large, small, large
SHAPES = [(m, r) for r in (3, 1, 2) for m in (257, 1, 65, 2, 64, 3, 5) if r <= m] + [(257, 3)]
ONLY_UNKNOWN = (2, 1)  # the shape whose batches hold unknown targets only


def start_words(rng):
    """Live records of every confidence, absent ones with either decision."""
    votes = rng.integers(0, 256, (N, M)).astype(np.uint32)
    cons = rng.integers(0, 256, (N, M)).astype(np.uint32)
    conf = rng.integers(0, 2 * 127, (N, M)).astype(np.uint32)
    live = votes | (cons << np.uint32(8)) | (conf << np.uint32(16))
    kind = rng.integers(0, 3, (N, M))
    absent = np.uint32(avhip.ABSENT_WORD)
    return np.where(kind == 0, absent, np.where(kind == 1, absent | np.uint32(1 << 16), live)).astype(np.uint32)


def split(rng, m, n_resp):
    """n_resp Responses of m entries in all (none empty), one node in two of them where there are two."""
    cuts = np.sort(rng.choice(np.arange(1, m), n_resp - 1, replace=False)) if n_resp > 1 else []
    offsets = np.concatenate([[0], cuts, [m]]).astype(np.int64)
    nodes = rng.choice(N, n_resp, replace=False).astype(np.int64)
    if n_resp > 1:
        nodes[-1] = nodes[0]
    return nodes, offsets


def targets_for(rng, offsets, shape, ascending):
    """Targets per Response: strictly ascending ones (a poll set's order; past M they are foreign) or
    any order with repeats. Every batch of two or more entries holds an unknown target."""
    parts = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        size = int(b - a)
        if shape == ONLY_UNKNOWN:
            t = M + 1 + np.arange(size)
        elif ascending:
            t = np.sort(rng.choice(np.arange(0, max(M, size) + 8), size, replace=False))
        else:
            t = rng.integers(-2, M + 3, size)
        parts.append(t)
    t = np.concatenate(parts).astype(np.int64)
    if t.size > 1 and ((t >= 0) & (t < M)).all():
        t[-1] = M + 5  # the last vote of the last Response: still ascending
    return t


def check_votes(sim, nodes, offsets, slots, errs, got, where):
    """got == the oracle's RegisterVotes per Response, in call order, on the known slots."""
    known = (slots >= 0) & (slots < M)
    assert (got[~known] == -1).all(), where
    for i, node in enumerate(nodes.tolist()):
        a, b = int(offsets[i]), int(offsets[i + 1])
        kn = known[a:b]
        exp = sim.register_votes(node, slots[a:b][kn], errs[a:b][kn])
        assert [(int(slots[v]), int(got[v])) for v in range(a, b) if got[v] >= 0] == exp, (where, i)


def test_batch_shapes(oracle):
    rng = np.random.default_rng(2024)
    eng = avhip.Engine(N, M, k=8, seed=9)
    sim = oracle.Sim(N, M, 8, seed=9, init_mode=avhip.INIT_ACCEPTED, init_param=0)
    eng.init_records(avhip.INIT_ACCEPTED, 0)
    hashes = rng.integers(I64.min, I64.max, size=M, dtype=np.int64, endpoint=True)
    assert len(set(hashes.tolist())) == M
    assert eng.catalog_intern(hashes).tolist() == list(range(M))
    words = start_words(rng)
    for x in (eng, sim):
        x.write_records(words)
        x.set_valid(41, False)  # after the hashes are interned: a new hash makes its slot valid
    saw_unknown = saw_twice = False
    touched = set()  # the call kinds that changed a record

    def same_records(where):
        assert np.array_equal(eng.read_records(), sim.dump()), where

    def to_hashes(slots):
        known = (slots >= 0) & (slots < M)
        hs = rng.integers(I64.min, I64.max, size=slots.size, dtype=np.int64, endpoint=True)
        assert not np.isin(hs, hashes).any()
        hs[known] = hashes[slots[known]]
        return hs

    for shape in SHAPES:
        m, n_resp = shape
        nodes, offsets = split(rng, m, n_resp)
        saw_twice |= len(set(nodes.tolist())) < n_resp
        # slot votes: ascending on the fast path, the same batch on the general one, then shuffled
        asc = targets_for(rng, offsets, shape, True)
        errs = rng.choice(ERRS, m)
        saw_unknown |= bool(((asc < 0) | (asc >= M)).any())
        for fast in (1, 0):
            eng.set_option("dropin_fast", fast)
            got = eng.register_votes_batch(nodes, offsets, asc, errs)
            check_votes(sim, nodes, offsets, asc, errs, got, (shape, "ascending", fast))
            same_records((shape, "ascending", fast))
            touched |= {("ascending", fast)} if (got >= 0).any() else set()
        eng.set_option("dropin_fast", 1)
        mixed = targets_for(rng, offsets, shape, False)
        errs = rng.choice(ERRS, m)
        got = eng.register_votes_batch(nodes, offsets, mixed, errs)
        check_votes(sim, nodes, offsets, mixed, errs, got, (shape, "shuffled"))
        same_records((shape, "shuffled"))
        touched |= {"shuffled"} if (got >= 0).any() else set()
        # hashed votes: ordered (the lookup kernel finds the fast path fit) and not
        for ascending in (True, False):
            slots = targets_for(rng, offsets, shape, ascending)
            errs = rng.choice(ERRS, m)
            got = eng.register_votes_hashed(nodes, offsets, to_hashes(slots), errs)
            check_votes(sim, nodes, offsets, slots, errs, got, (shape, "hashed", ascending))
            same_records((shape, "hashed", ascending))
            touched |= {("hashed", ascending)} if (got >= 0).any() else set()
        # adds: repeats inside a list, records the votes above finalized and deleted among them
        ts = targets_for(rng, offsets, shape, False)
        acc = rng.integers(0, 2, m).astype(np.uint8)
        got = eng.add_targets_batch(nodes, offsets, ts, acc)
        exp = []
        for i, node in enumerate(nodes.tolist()):
            a, b = int(offsets[i]), int(offsets[i + 1])
            exp += [bool(0 <= t < M and sim.add(node, t, x)) for t, x in zip(ts[a:b].tolist(), acc[a:b].tolist())]
        assert got.tolist() == exp, (shape, "adds")
        same_records((shape, "adds"))
        touched |= {"adds"} if got.any() else set()
    assert saw_unknown and saw_twice and len(touched) == 6, touched
    eng.run_rounds(1)
    exp_u, _ = sim.run_round()
    assert np.array_equal(eng.fetch_updates(), exp_u)
    eng.close()
