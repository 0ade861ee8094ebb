"""Peer-list topologies for the tools (rule R6, Engine.set_peer_lists_csr), built with numpy at any
network size: int64 offsets[n + 1] and int64 peers, every list strictly ascending and without its own
node."""
import numpy as np


def random_lists(n, degree, seed=1):
    """Random out-lists of `degree` peers per node. Node i's j-th peer sits at distance
    1 + j * stride + U[0, stride) ahead of it (mod n), stride = (n - 1) // degree: one uniform pick from
    each of `degree` disjoint arcs of the ring, so the peers are distinct, never i, and spread over the
    whole network."""
    assert 0 < degree <= n - 1
    rng = np.random.default_rng(seed)
    stride = (n - 1) // degree
    peers = np.empty((n, degree), np.int64)
    step = max(1, (1 << 24) // degree)  # rows per chunk: bounds the temporaries
    base = 1 + np.arange(degree, dtype=np.int64) * stride
    for a in range(0, n, step):
        b = min(n, a + step)
        rel = base + rng.integers(0, stride, size=(b - a, degree), dtype=np.int64)
        peers[a:b] = (np.arange(a, b, dtype=np.int64)[:, None] + rel) % n
    peers.sort(axis=1)
    return np.arange(n + 1, dtype=np.int64) * degree, peers.reshape(-1)


def group_lists(n, groups):
    """`groups` equal groups of consecutive nodes, complete lists inside each group."""
    assert groups >= 1 and n % groups == 0 and n // groups >= 2
    size = n // groups
    d = size - 1
    if n * d >= 2**31:  # (before anything of that size is allocated)
        raise ValueError(f"{n} nodes in groups of {size}: {n * d} list entries, av_set_peer_lists takes fewer than 2^31")
    peers = np.empty((n, d), np.int64)
    inner = np.arange(size, dtype=np.int64)
    # member j of a group lists 0..j-1, j+1..size-1 of it
    one = np.array([np.delete(inner, j) for j in range(size)], np.int64)
    for g in range(groups):
        peers[g * size:(g + 1) * size] = one + g * size
    return np.arange(n + 1, dtype=np.int64) * d, peers.reshape(-1)
