"""TEST INFRASTRUCTURE ONLY: one round over per-node peer lists (rule R6), with or without
lost Responses (rule R5), restated over the oracle's Sim (oracle/cabi.py), for
tests/test_connman_ref_cpu.py and tests/test_gpu_connman.py.

Node n has a list C(n) of d global ids, strictly ascending, none of them n. d <= k: slot s < d polls
C(n)[s], slots s >= d are empty (no RegisterVotes call, nothing lost). d > k: the candidate stream R1
uses, x = philox({n, r, blk, 1}, seed) for blk = 0, 1, ..., u = (x[i] * d) >> 32, the first k distinct
u in stream order; slot s polls C(n)[u_s]. A slot that is not empty is lost by R5's rule (its own
draw, lossy_ref.drawn_lost, or its listed peer is down). ConnmanRef.round calls Sim.register_votes
slot by slot on the node's round-start live valid targets."""
import numpy as np

import lossy_ref as L
from oracle import cabi

NO_PEER = -1
DOM_PEERS = 1


def listed_peers(seed, node, rnd, k, peers):
    """int64[k]: what av_sample_peers answers for a node whose list is `peers`; NO_PEER in empty slots."""
    peers = [int(q) for q in peers]
    d = len(peers)
    out = np.full(k, NO_PEER, np.int64)
    if d <= k:
        out[:d] = peers
        return out
    key = [seed & 0xFFFFFFFF, seed >> 32]
    picked, blk = [], 0
    while len(picked) < k:
        x = cabi.philox([node, rnd & 0xFFFFFFFF, blk, DOM_PEERS], key)
        for i in range(4):
            u = (int(x[i]) * d) >> 32
            if u not in picked and len(picked) < k:
                picked.append(u)
        blk += 1
    out[:] = [peers[u] for u in picked]
    return out


def peer_table(seed, lists, k, rnd, n0=0):
    """int64[len(lists), k]: listed_peers of nodes n0, n0 + 1, ..."""
    return np.array([listed_peers(seed, n0 + i, rnd, k, c) for i, c in enumerate(lists)], np.int64).reshape(-1, k)


def lost_table(seed, lists, k, rnd, thr, down=(), n0=0):
    """bool[len(lists), k]: what av_sample_lost answers on an engine with lists: 0 in empty slots."""
    down = set(int(d) for d in down)
    peers = peer_table(seed, lists, k, rnd, n0)
    out = np.zeros(peers.shape, bool)
    for i in range(len(lists)):
        drawn = L.drawn_lost(seed, n0 + i, rnd, k, thr)
        out[i] = (peers[i] != NO_PEER) & (drawn | np.array([int(q) in down for q in peers[i]]))
    return out


def complete_lists(n):
    return [[q for q in range(n) if q != j] for j in range(n)]


def group_lists(n, groups):
    """`groups` equal groups of consecutive nodes, complete inside each group."""
    size = n // groups
    return [[q for q in range(j // size * size, j // size * size + size) if q != j] for j in range(n)]


def mixed_lists(n, k, seed=1):
    """Node i gets degree [0, 1, 3, k, k + 1, 20, n - 1][i % 7]: peers drawn without replacement by a
    seeded numpy generator, sorted."""
    rng = np.random.default_rng(seed)
    degs = [0, 1, 3, k, k + 1, 20, n - 1]
    out = []
    for i in range(n):
        others = np.array([q for q in range(n) if q != i])
        out.append(sorted(int(q) for q in rng.choice(others, size=min(degs[i % 7], n - 1), replace=False)))
    return out


class ConnmanRef:
    """A Sim plus what the restated round needs beside it: the lists (None: the whole network, R1),
    validity, the nodes that are down, the nodes that do not poll, the counters. sim.round is the
    round the next call runs."""

    def __init__(self, sim, seed, lists=None):
        self.sim, self.seed, self.lists = sim, seed, lists
        self.valid = np.ones(sim.m, bool)
        self.down = set()
        self.nopoll = set()
        self.byz = np.array([sim.is_byzantine(j) for j in range(sim.n)], bool)
        self.applied = 0
        self.lost = 0
        self.unsent = 0

    def set_valid(self, t, v):
        self.valid[t] = bool(v)
        self.sim.set_valid(t, v)

    def set_polling(self, node, polls):
        (self.nopoll.discard if polls else self.nopoll.add)(int(node))
        self.sim.set_polling(node, polls)

    def set_responder(self, mode):
        self.sim.set_responder(mode)

    def set_responding(self, nodes, responds):
        for j in np.atleast_1d(nodes):
            (self.down.discard if responds else self.down.add)(int(j))

    def _errs(self, pref, peer, r):
        """The err word of every target in the Response of `peer` (main.go:179-182; Byzantine: R4)."""
        t = np.arange(self.sim.m)
        if self.byz[peer]:
            return ((r ^ t) & 1).astype(np.uint32)
        return (1 - pref[peer]).astype(np.uint32)

    def tables(self, thr=0):
        """(peers int64[n, k], lost bool[n, k]) of the round the next call runs."""
        sim, r = self.sim, self.sim.round
        return (peer_table(self.seed, self.lists, sim.k, r),
                lost_table(self.seed, self.lists, sim.k, r, thr, self.down))

    def round(self, thr=0, mode=L.SKIP):
        """One listed round by per-slot register_votes. Returns the updates int64[n, 5] (round, node,
        slot, target, status) in canonical order."""
        sim, r = self.sim, self.sim.round
        pref, words = sim.pref().copy(), sim.dump().copy()  # register_votes refreshes the Sim's own rows
        peers, lost = self.tables(thr)
        rows = []
        for node in range(sim.n):
            if node in self.nopoll:
                continue  # no query goes out: nothing unsent, nothing to lose, nothing registered
            alive = [int(t) for t in np.flatnonzero(((words[node] >> 17) < 128) & self.valid)]
            self.unsent += int((peers[node] == NO_PEER).sum())
            self.lost += int(lost[node].sum())
            for s in range(sim.k):
                if peers[node, s] == NO_PEER:
                    continue  # an empty slot: the RegisterVotes call that never happens, in either mode
                if lost[node, s] and mode == L.SKIP:
                    continue
                if not alive:
                    continue
                errs = self._errs(pref, int(peers[node, s]), r)[alive]
                if lost[node, s]:
                    errs = np.full(len(alive), L.NEUTRAL_ERR, np.uint32)
                self.applied += len(alive)
                ups = sim.register_votes(node, alive, errs)
                rows += [(r, node, s, t, st) for t, st in ups]
                gone = {t for t, st in ups if st in (0, 3)}  # finalized: deleted (processor.go:114-116)
                alive = [t for t in alive if t not in gone]
        sim.set_round_index(r + 1)
        return np.array(rows, np.int64).reshape(-1, 5)

    def plain_round(self):
        """The oracle's own round of a perfect network (no lists, no loss)."""
        ups, applied = self.sim.run_round()
        self.applied += applied
        return ups

    def live(self):
        return int(((self.sim.dump() >> 17) < 128).sum())

    def finalized(self):
        return int(((self.sim.dump() >> 17) >= 128).sum())
