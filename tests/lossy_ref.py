"""TEST INFRASTRUCTURE ONLY: one round with lost Responses and unresponsive nodes (rule R5)
restated over the oracle's Sim (oracle/cabi.py), for tests/test_lossy_ref_cpu.py and
tests/test_gpu_lossy.py.

The Response of slot s of node n in round r is lost iff philox({n, r, s >> 2, 6}, seed)[s & 3] <
threshold, or its peer (R1's draw, cabi.sample_peers) is down. SKIP: that slot's RegisterVotes call
never happens (processor.go:66-76); NEUTRAL: it registers err = 0x80000000 on every polled target
(vote.go:55-56). Two routes: LossyRef.round calls Sim.register_votes slot by slot on the node's
round-start live valid targets; LossyRef.round_replay (NEUTRAL only) hands Sim.run_round the whole
round's err array."""
import numpy as np

from oracle import cabi

SKIP, NEUTRAL = 0, 1
DOM_LOSS = 6
NEUTRAL_ERR = 0x80000000


def threshold(p):
    """The 32-bit threshold of a loss probability."""
    return int(p * 2**32)


def drawn_lost(seed, node, rnd, k, thr):
    """bool[k]: slot s drawn lost, philox({node, rnd, s >> 2, 6}, seed)[s & 3] < thr."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    out = np.zeros(k, bool)
    for blk in range((k + 3) // 4):
        x = cabi.philox([node, rnd & 0xFFFFFFFF, blk, DOM_LOSS], key)
        for i in range(4):
            if blk * 4 + i < k:
                out[blk * 4 + i] = int(x[i]) < thr
    return out


def lost_table(seed, n, k, rnd, thr, down=(), peer_mode=0):
    """bool[n, k]: what av_sample_lost answers, lost by the draw or because the peer is down."""
    down = set(int(d) for d in down)
    out = np.zeros((n, k), bool)
    for node in range(n):
        peers = cabi.sample_peers(seed, node, rnd & 0xFFFFFFFF, n, k, peer_mode)
        out[node] = drawn_lost(seed, node, rnd, k, thr) | np.array([int(q) in down for q in peers])
    return out


class LossyRef:
    """A Sim plus what the restated round needs beside it: validity, the nodes that are down, the
    counters. sim.round is the round the next call runs."""

    def __init__(self, sim, seed, peer_mode=0):
        self.sim, self.seed, self.peer_mode = sim, seed, peer_mode
        self.valid = np.ones(sim.m, bool)
        self.down = set()
        self.nopoll = set()
        self.byz = np.array([sim.is_byzantine(j) for j in range(sim.n)], bool)
        self.applied = 0
        self.lost = 0

    def set_valid(self, t, v):
        self.valid[t] = bool(v)
        self.sim.set_valid(t, v)

    def set_polling(self, node, polls):
        """A node whose run loop has returned polls nothing and still answers (main.go:160-162)."""
        (self.nopoll.discard if polls else self.nopoll.add)(int(node))
        self.sim.set_polling(node, polls)

    def set_responder(self, mode):
        """What a node answers for a target it no longer holds (Sim.set_responder: 0 = R2, 1 = IsAccepted)."""
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

    def round(self, thr, mode):
        """One lossy round by per-slot register_votes. Returns the updates int64[n, 5] (round, node,
        slot, target, status) in canonical order."""
        sim, r = self.sim, self.sim.round
        pref, words = sim.pref().copy(), sim.dump().copy()  # register_votes refreshes the Sim's own rows
        lost = lost_table(self.seed, sim.n, sim.k, r, thr, self.down, self.peer_mode)
        rows = []
        for node in range(sim.n):
            if node in self.nopoll:
                continue  # no query goes out: nothing to lose, nothing registered
            peers = cabi.sample_peers(self.seed, node, r, sim.n, sim.k, self.peer_mode)
            alive = [int(t) for t in np.flatnonzero(((words[node] >> 17) < 128) & self.valid)]
            self.lost += int(lost[node].sum())
            for s in range(sim.k):
                if lost[node, s] and mode == SKIP:
                    continue
                if not alive:
                    continue
                errs = self._errs(pref, int(peers[s]), r)[alive]
                if lost[node, s]:
                    errs = np.full(len(alive), NEUTRAL_ERR, np.uint32)
                self.applied += len(alive)
                ups = sim.register_votes(node, alive, errs)
                rows += [(r, node, s, t, st) for t, st in ups]
                gone = {t for t, st in ups if st in (0, 3)}  # finalized: deleted (processor.go:114-116)
                alive = [t for t in alive if t not in gone]
        sim.set_round_index(r + 1)
        return np.array(rows, np.int64).reshape(-1, 5)

    def round_replay(self, thr):
        """One NEUTRAL round by Sim.run_round(replay_errs=...): 0x80000000 in the lost slots."""
        sim, r = self.sim, self.sim.round
        pref = sim.pref().copy()
        lost = lost_table(self.seed, sim.n, sim.k, r, thr, self.down, self.peer_mode)
        errs = np.empty((sim.n, sim.k, sim.m), np.uint32)
        for node in range(sim.n):
            peers = cabi.sample_peers(self.seed, node, r, sim.n, sim.k, self.peer_mode)
            for s in range(sim.k):
                errs[node, s] = NEUTRAL_ERR if lost[node, s] else self._errs(pref, int(peers[s]), r)
        self.lost += int(lost[[j for j in range(sim.n) if j not in self.nopoll]].sum())
        ups, applied = sim.run_round(replay_errs=errs)
        self.applied += applied
        return ups

    def live(self):
        return int(((self.sim.dump() >> 17) < 128).sum())
