"""Numpy statement of the network census (include/avhip.h av_census) over the
canonical record words of av_read_records / the oracle's dump:
  absent = (w >> 17) >= 128, a = (w >> 16) & 1, class = 2 * absent + a,
  count = (w >> 17) & 127 for live records."""
import numpy as np

LIVE_REJECTED, LIVE_ACCEPTED, ABSENT_REJECTED, ABSENT_ACCEPTED = 0, 1, 2, 3


def census_from_words(words, honest_mask=None):
    """words: uint32 [nodes][targets]; honest_mask: bool [nodes], the nodes counted (None = all).
    Returns the four outputs of av_census; rows of node_classes of uncounted nodes are zero."""
    w = np.asarray(words, np.uint32)
    n, m = w.shape
    counted = np.ones(n, bool) if honest_mask is None else np.asarray(honest_mask, bool)
    absent = (w >> np.uint32(17)) >= 128
    a = ((w >> np.uint32(16)) & np.uint32(1)).astype(np.int64)
    cls = 2 * absent.astype(np.int64) + a
    count = ((w >> np.uint32(17)) & np.uint32(127)).astype(np.int64)
    live = ~absent & counted[:, None]
    target_classes = np.zeros((m, 4), np.int64)
    node_classes = np.zeros((n, 4), np.int32)
    for c in range(4):
        is_c = (cls == c) & counted[:, None]
        target_classes[:, c] = is_c.sum(axis=0)
        node_classes[:, c] = is_c.sum(axis=1)
    count_hist = np.zeros((2, 128), np.int64)
    for acc in (0, 1):
        count_hist[acc] = np.bincount(count[live & (a == acc)], minlength=128)
    return {
        "target_classes": target_classes,
        "target_count_sum": np.where(live, count, 0).sum(axis=0).astype(np.int64),
        "node_classes": node_classes,
        "count_hist": count_hist,
    }


def check_identities(c, n_counted, n_targets, counted=None):
    """Every counted node has exactly one class per target."""
    assert (c["target_classes"].sum(axis=1) == n_counted).all()
    rows = c["node_classes"].sum(axis=1)
    if counted is None:
        assert (rows == n_targets).all()
    else:
        assert (rows[counted] == n_targets).all() and (rows[~counted] == 0).all()
