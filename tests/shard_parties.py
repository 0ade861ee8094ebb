"""Sharded networks presented as one engine, for life_schedule.Life.

TargetShards: G engines over target ranges (target_range=ranges[g]) of one network.
PeerGroup: the ranks of a serial peer group (avhip.peer_group_serial), equal node shards.
PartyAv: the binding module as Life sees it, with compact_expand / compact_header over
the list of per-shard streams a party's fetch_compact returns.
Pure Python and numpy: the binding module and the engines are passed in.

A party must not be able to hide a shard's mistake, so:
  * a single shard's output is never sorted before its own order is checked: every
    shard's updates must arrive strictly ascending by (round, node, slot, target), and
    only then are the shards' streams merged;
  * results of several shards are never combined with max / or unless at most one shard
    claims each position (merge_statuses, merge_added assert it; keys met twice in
    merged streams are refused too);
  * every shard gets the whole of a drop-in call (register_votes[_batch], add_targets) and
    every set_valid, with global ids: a shard skips foreign targets as the reference skips
    unknown hashes, and nothing here does that for it;
  * a cell query goes to the owning shard, and one non-owning shard must answer "no
    record" (False / VoteRecordNotFound)."""
import numpy as np

CENSUS_KEYS = ("target_classes", "target_count_sum", "node_classes", "count_hist")
M64 = (1 << 64) - 1


# ---- pure helpers
def merge_digests(parts):
    """(count, sum, xor) digests of disjoint update sets: count and sum add mod 2^64, xor xors."""
    count = total = x = 0
    for c, s, v in parts:
        count, total, x = (count + int(c)) & M64, (total + int(s)) & M64, x ^ int(v)
    return count, total, x


def update_keys(rows):
    """One integer per decoded update row, ordered as (round, node, slot, target)."""
    u = np.asarray(rows, np.int64).reshape(-1, 5)
    assert u.size == 0 or (u[:, :4].min() >= 0 and u[:, 1].max() < 1 << 24 and u[:, 2].max() < 16 and
                           u[:, 3].max() < 1 << 22 and u[:, 0].max() < 1 << 12)
    return (((u[:, 0] << 24 | u[:, 1]) << 4 | u[:, 2]) << 22) | u[:, 3]


def _merge(parts, keys, what):
    for g, k in enumerate(keys):
        assert np.all(k[1:] > k[:-1]), f"{what}: part {g} is not strictly ascending by (round, node, slot, target)"
    if not parts:
        return None
    allk = np.concatenate(keys)
    order = np.argsort(allk, kind="stable")  # every part ascending: a stable sort of the concatenation merges them
    merged = allk[order]
    assert np.all(merged[1:] > merged[:-1]), f"{what}: two parts hold an update of the same (round, node, slot, target)"
    return np.concatenate(parts)[order]


def merge_updates(parts):
    """Decoded update rows int64 [n][5] of disjoint shards, each in canonical order, merged."""
    parts = [np.asarray(p, np.int64).reshape(-1, 5) for p in parts]
    out = _merge(parts, [update_keys(p) for p in parts], "merge_updates")
    return np.zeros((0, 5), np.int64) if out is None else out


def merge_words(parts):
    """The same for packed uint64 update words (status in bits [1:0], the order above it)."""
    parts = [np.asarray(p, np.uint64).reshape(-1) for p in parts]
    out = _merge(parts, [p >> np.uint64(2) for p in parts], "merge_words")
    return np.zeros(0, np.uint64) if out is None else out


def _split(start, arr, ranges, axis):
    arr = np.asarray(arr)
    out = []
    for g, (a, b) in enumerate(ranges):
        lo, hi = max(a, start), min(b, start + arr.shape[axis])
        if lo < hi:
            index = [slice(None)] * arr.ndim
            index[axis] = slice(lo - start, hi - start)
            out.append((g, lo, arr[tuple(index)]))
    return out


def split_columns(rect_t0, words, ranges):
    """An array whose last axis holds targets rect_t0.. cut at the shards' target ranges:
    [(shard, first target, piece)], empty pieces dropped."""
    return _split(rect_t0, words, ranges, np.asarray(words).ndim - 1)


def split_rows(rect_n0, words, ranges):
    """An array whose first axis holds nodes rect_n0.. cut at the ranks' node ranges."""
    return _split(rect_n0, words, ranges, 0)


def merge_statuses(parts):
    """Per-vote statuses of the shards of one drop-in call (-1 = none): at most one shard may
    give a vote a status; that shard's value."""
    st = np.stack([np.asarray(p, np.int64) for p in parts])
    assert (st >= -1).all(), "merge_statuses: a status below -1"
    claims = (st >= 0).sum(axis=0)
    assert (claims <= 1).all(), f"merge_statuses: votes {np.flatnonzero(claims > 1).tolist()} have a status on two shards"
    return st.max(axis=0).astype(np.int32)


def merge_added(parts):
    """add_targets results of the shards: at most one shard may add a position."""
    ad = np.stack([np.asarray(p, bool) for p in parts])
    claims = ad.sum(axis=0)
    assert (claims <= 1).all(), f"merge_added: positions {np.flatnonzero(claims > 1).tolist()} added by two shards"
    return ad.any(axis=0)


def merge_census_targets(parts):
    """Censuses of target shards over the same nodes: target-indexed outputs concatenate,
    node_classes and count_hist add."""
    return {"target_classes": np.concatenate([p["target_classes"] for p in parts]),
            "target_count_sum": np.concatenate([p["target_count_sum"] for p in parts]),
            "node_classes": sum(p["node_classes"] for p in parts),
            "count_hist": sum(p["count_hist"] for p in parts)}


def merge_census_nodes(parts):
    """Censuses of consecutive node ranges over the same targets: node_classes concatenates, the rest add."""
    return {"target_classes": sum(p["target_classes"] for p in parts),
            "target_count_sum": sum(p["target_count_sum"] for p in parts),
            "node_classes": np.concatenate([p["node_classes"] for p in parts]),
            "count_hist": sum(p["count_hist"] for p in parts)}


def merge_invs(parts):
    """Poll sets (offsets, targets) of target shards over the same nodes: per node, the shards'
    lists concatenated in shard order."""
    n = len(parts[0][0]) - 1
    assert all(len(offs) == n + 1 and offs[0] == 0 and offs[-1] == len(tg) for offs, tg in parts)
    rows = [np.concatenate([np.asarray(tg)[offs[i]:offs[i + 1]] for offs, tg in parts]) for i in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return offsets, (np.concatenate(rows) if rows else np.zeros(0, np.int32)).astype(np.int32)


def concat_invs(parts):
    """Poll sets of consecutive node ranges: the ranges' rows one after the other."""
    assert all(offs[0] == 0 and offs[-1] == len(tg) for offs, tg in parts)
    base = np.concatenate([[0], np.cumsum([len(tg) for _, tg in parts])])
    offsets = np.concatenate([[0]] + [np.asarray(offs[1:], np.int64) + base[g] for g, (offs, _) in enumerate(parts)])
    return offsets.astype(np.int64), np.concatenate([np.asarray(tg, np.int32) for _, tg in parts])


def _common(values, what):
    assert len(set(values)) == 1, f"{what} differs between the shards: {values}"
    return values[0]


class Streams(list):
    """A party's fetch_compact: the shards' streams, with the bases their headers must name."""

    def __init__(self, streams, bases):
        super().__init__(streams)
        self.bases = bases  # per stream (node_base, target_base)


class PartyAv:
    """The binding module for a Life whose engines are parties."""

    def __init__(self, av):
        self.av = av
        self.VoteRecordNotFound = av.VoteRecordNotFound
        self.decode_updates = av.decode_updates

    def compact_expand(self, streams):
        self.compact_header(streams)  # a wrong base would shift every expanded word
        return merge_words([self.av.compact_expand(s) for s in streams])  # (merge_words checks each one's order)

    def compact_header(self, streams):
        heads = [self.av.compact_header(s) for s in streams]
        for h, (node_base, target_base) in zip(heads, streams.bases):
            assert (h["node_base"], h["target_base"]) == (node_base, target_base), \
                f"compact header bases {(h['node_base'], h['target_base'])}, the shard's are {(node_base, target_base)}"
        return {"log_base": _common([h["log_base"] for h in heads], "compact log_base"),
                "n_updates": sum(h["n_updates"] for h in heads)}


class _Party:
    """What both parties do the same way: fan-outs, sums and values every shard must agree on."""

    def __init__(self, engines, av):
        self.engines, self.av = list(engines), av

    def set_option(self, name, value):
        for e in self.engines:
            e.set_option(name, value)

    def materialize(self):
        for e in self.engines:
            e.materialize()

    def discard_updates(self):
        for e in self.engines:
            e.discard_updates()

    def set_valid(self, target, valid):
        for e in self.engines:  # every shard, not only the owner
            e.set_valid(target, valid)

    def set_loss(self, threshold, mode=0):
        for e in self.engines:
            e.set_loss(threshold, mode)

    def set_responding(self, nodes, responds):
        for e in self.engines:  # global node ids, on every shard
            e.set_responding(nodes, responds)

    def sample_lost(self, rnd, n0=0, n1=None):
        tables = [e.sample_lost(rnd, n0, n1) for e in self.engines]
        assert all(np.array_equal(t, tables[0]) for t in tables[1:]), "sample_lost differs between the shards"
        return tables[0]

    def lost_responses(self):
        return _common([e.lost_responses() for e in self.engines], "lost_responses")

    def updates_digest(self, n0=None, n1=None):
        return merge_digests([e.updates_digest(n0, n1) for e in self.engines])

    def updates_count(self):
        return sum(e.updates_count() for e in self.engines)

    def alg_bytes(self):
        return sum(e.alg_bytes() for e in self.engines)

    def applied_votes(self):
        return sum(e.applied_votes() for e in self.engines)

    def finalized_count(self):
        return sum(e.finalized_count() for e in self.engines)

    def live_records(self, honest_only=False):
        return sum(e.live_records(honest_only) for e in self.engines)

    def log_base_round(self):
        return _common([e.log_base_round() for e in self.engines], "log_base_round")

    @property
    def round(self):
        return _common([e.round for e in self.engines], "round")

    def fetch_updates(self):
        return merge_updates([e.fetch_updates() for e in self.engines])

    def fetch_compact(self):
        return Streams([e.fetch_compact() for e in self.engines],
                       [(e.node_range[0], e.target_range[0]) for e in self.engines])

    def _cell(self, owner, other, node, target):
        """The owner of a cell and one engine that does not hold it, which must say so."""
        assert other.is_accepted(node, target) is False, "is_accepted of a foreign cell is not False"
        try:
            other.get_confidence(node, target)
        except self.av.VoteRecordNotFound:
            return owner
        raise AssertionError("get_confidence of a foreign cell did not raise VoteRecordNotFound")


class TargetShards(_Party):
    """G engines over target_range=ranges[g] as one engine of the whole network."""

    def __init__(self, engines, ranges, av):
        super().__init__(engines, av)
        self.ranges = [tuple(r) for r in ranges]
        assert [tuple(e.target_range) for e in self.engines] == self.ranges
        self.n, self.m = self.engines[0].n_nodes, self.engines[0].n_targets
        assert self.ranges[0][0] == 0 and self.ranges[-1][1] == self.m
        assert all(a[1] == b[0] for a, b in zip(self.ranges, self.ranges[1:]))

    def init_records(self, mode, param):
        for e in self.engines:
            e.init_records(mode, param)

    def run_rounds(self, rounds=1):
        for e in self.engines:
            e.run_rounds(rounds)

    def replay_round_errs(self, errs):
        assert errs.shape[0] == self.n and errs.shape[2] == self.m
        for e, (t0, t1) in zip(self.engines, self.ranges):
            e.replay_round_errs(errs[:, :, t0:t1])

    def register_votes(self, node, targets, errs):
        return merge_statuses([e.register_votes(node, targets, errs) for e in self.engines])

    def register_votes_batch(self, nodes, offsets, targets, errs):
        return merge_statuses([e.register_votes_batch(nodes, offsets, targets, errs) for e in self.engines])

    def add_targets(self, node, targets, accepted):
        return merge_added([e.add_targets(node, targets, accepted) for e in self.engines])

    def write_records(self, words, n0=0, t0=0):
        for g, start, piece in split_columns(t0, words, self.ranges):
            self.engines[g].write_records(piece, n0=n0, t0=start)

    def read_records(self, n0=None, n1=None, t0=None, t1=None):
        n0, n1 = (0 if n0 is None else n0), (self.n if n1 is None else n1)
        t0, t1 = (0 if t0 is None else t0), (self.m if t1 is None else t1)
        parts = [self.engines[g].read_records(n0, n1, max(a, t0), min(b, t1))
                 for g, (a, b) in enumerate(self.ranges) if max(a, t0) < min(b, t1)]
        return np.concatenate(parts, axis=1) if parts else np.zeros((n1 - n0, 0), np.uint32)

    def read_pref(self):
        return np.concatenate([e.read_pref() for e in self.engines], axis=1)

    def _owner(self, node, target):
        g = next(i for i, (a, b) in enumerate(self.ranges) if a <= target < b)
        return self._cell(self.engines[g], self.engines[(g + 1) % len(self.engines)], node, target)

    def is_accepted(self, node, target):
        return self._owner(node, target).is_accepted(node, target)

    def get_confidence(self, node, target):
        return self._owner(node, target).get_confidence(node, target)

    def get_invs_batch(self, n0=None, n1=None):
        return merge_invs([e.get_invs_batch(n0, n1) for e in self.engines])

    def census(self, n0=None, n1=None, honest_only=False):
        return merge_census_targets([e.census(n0, n1, honest_only=honest_only) for e in self.engines])

    def close(self):
        for e in self.engines:
            e.close()


class PeerGroup(_Party):
    """The node-shard engines of one network (rank order) as one engine: created and initialised
    one by one, then made a serial peer group by group(). The record writes a peer-push engine
    refuses (register_votes[_batch], add_targets, write_records) are not offered."""

    def __init__(self, engines, av):
        super().__init__(engines, av)
        self.ranges = [tuple(e.node_range) for e in self.engines]
        self.n, self.m = self.engines[0].n_nodes, self.engines[0].n_targets
        assert self.ranges[0][0] == 0 and self.ranges[-1][1] == self.n
        assert all(a[1] == b[0] for a, b in zip(self.ranges, self.ranges[1:]))
        self.grouped = False

    def group(self):
        self.av.peer_group_serial(self.engines)
        self.grouped = True

    def init_records(self, mode, param):
        for e in self.engines:  # collective: every rank re-initialises, in rank order
            e.synchronize()
            e.discard_updates()
            e.init_records(mode, param)

    def run_rounds(self, rounds=1):
        self.av.run_group_rounds(self.engines, rounds)

    def replay_round_errs(self, errs):
        pieces = split_rows(0, errs, self.ranges)
        assert [g for g, _, _ in pieces] == list(range(len(self.engines)))
        for g, _, piece in pieces:
            self.engines[g].replay_round_errs(piece)

    def _cut(self, n0, n1):
        n0, n1 = (0 if n0 is None else n0), (self.n if n1 is None else n1)
        return [(self.engines[g], max(a, n0), min(b, n1)) for g, (a, b) in enumerate(self.ranges)
                if max(a, n0) < min(b, n1)]

    def read_records(self, n0=None, n1=None, t0=None, t1=None):
        parts = [e.read_records(a, b, t0, t1) for e, a, b in self._cut(n0, n1)]
        return np.concatenate(parts)

    def read_pref(self):
        # a rank's own rows: under masked pushes its copy of foreign rows may lawfully lag
        return np.concatenate([e.read_pref(*e.node_range) for e in self.engines])

    def _owner(self, node, target):
        g = next(i for i, (a, b) in enumerate(self.ranges) if a <= node < b)
        return self._cell(self.engines[g], self.engines[(g + 1) % len(self.engines)], node, target)

    def is_accepted(self, node, target):
        return self._owner(node, target).is_accepted(node, target)

    def get_confidence(self, node, target):
        return self._owner(node, target).get_confidence(node, target)

    def get_invs_batch(self, n0=None, n1=None):
        return concat_invs([e.get_invs_batch(a, b) for e, a, b in self._cut(n0, n1)])

    def census(self, n0=None, n1=None, honest_only=False):
        return merge_census_nodes([e.census(a, b, honest_only=honest_only) for e, a, b in self._cut(n0, n1)])

    def close(self):
        if self.grouped:
            self.engines[0].close()  # a member takes the whole group with it
        else:
            for e in self.engines:
                e.close()
