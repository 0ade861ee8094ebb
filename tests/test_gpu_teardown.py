"""Teardown after the engine's lazily created resources. Each case makes an
engine allocate something it does not have after av_create (the responder's
re-add planes, the non-polling bitset, a compact delivery slot with a copy in
flight, the poll-set staging, the solo barrier's arrival slots, re-allocated
snapshot buffers, a serial peer group), destroys it, and then checks that a
fresh engine still runs three rounds bit for bit against the oracle: what a
destroyed engine owned is released by its members' owners (csrc/engine_mem.h),
and a double free or a buffer freed under a running stream would show here.

Nothing is asserted about free device memory: the card is shared.

Shapes: 64 nodes x 96 targets (uncapped, k = 8) and 8 nodes x 4128 targets
(capped), the smallest that take the sweep kernel and the node kernel."""
import functools

import numpy as np
import pytest

import avhip

pytestmark = pytest.mark.gpu

P80 = int(0.8 * 2**32)
SHAPES = {"uncapped": (64, 96), "capped": (8, 4128)}
K, SEED, ROUNDS = 8, 23, 3


def make(shape, node_range=None):
    n, m = SHAPES[shape]
    e = avhip.Engine(n, m, k=K, seed=SEED, node_range=node_range)
    e.init_records(avhip.INIT_BERNOULLI, P80)
    return e


@functools.lru_cache(maxsize=None)
def expected(shape):
    """Three oracle rounds of the shape: (records, sorted updates); computed once, read only."""
    from oracle import cabi

    n, m = SHAPES[shape]
    sim = cabi.Sim(n, m, K, seed=SEED, byz_threshold=0, init_mode=3, init_param=P80)
    upd = np.concatenate([sim.run_round()[0] for _ in range(ROUNDS)])
    rec = sim.dump()
    rec.setflags(write=False)
    upd.setflags(write=False)
    return rec, upd


def check_fresh_engine(shape):
    rec, upd = expected(shape)
    with make(shape) as e:
        e.run_rounds(ROUNDS)
        assert np.array_equal(e.fetch_updates(), upd), "StatusUpdate stream differs from the oracle"
        assert np.array_equal(e.read_records(), rec), "VoteRecord state differs from the oracle"


def responder(e):
    e.set_option("responder", 2)


def polling(e):
    e.set_polling(e.node_range[0] + 1, False)


def compact_unwaited(e):
    e.run_rounds(2)
    e.fetch_compact_async()  # the ticket is dropped: the copy may still be in flight at destroy


def invs_batch(e):
    offs, _ = e.get_invs_batch()
    assert offs[-1] > 0


def solo_barrier(e):
    e.set_option("solo_barrier", 1)


def pref_uncached(e):
    e.set_option("pref_uncached", 1)


LAZY = [responder, polling, compact_unwaited, invs_batch, solo_barrier, pref_uncached]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("lazy", LAZY, ids=lambda f: f.__name__)
def test_destroy_after_lazy_resource(oracle, shape, lazy):
    e = make(shape)
    lazy(e)
    e.close()
    check_fresh_engine(shape)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["rank0_first", "rank1_first"])
def test_destroy_serial_group_either_order(oracle, shape, order):
    n, _ = SHAPES[shape]
    engs = [make(shape, node_range=(r * n // 2, (r + 1) * n // 2)) for r in range(2)]
    avhip.peer_group_serial(engs)
    for e in engs:
        e._group = None  # Engine.close would take the group along: destroy the members one by one
    for r in order:
        engs[r].close()
    check_fresh_engine(shape)
