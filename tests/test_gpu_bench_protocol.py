"""bench.py's own step sequence pinned against the oracle ("pin
what the bench times"): bench.Runner — the class measure() drives — runs its
exact protocol on a 100k-node x 1000-target C4-shaped network: one untimed warm
epoch (one round per call, log emptied after each), goto(warmup) (re-population
with av_init_records on an engine that has already run 16 rounds, then the
warmup rounds), then the timed steps as measure() runs them (run_rounds of a
whole segment: rounds 5-15 of the second epoch, a re-population, rounds 0-8 of
the third). Every segment's StatusUpdate digest and applied votes are compared
with the oracle (a fresh network per epoch whose round counter starts where
the engine's does: Sim.set_round_index), and the full record state after each
timed segment.

Reference: vote.go:54-91, processor.go:92-117 under SURVEY.md §8(a) R1-R4.
"""
import argparse
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import avhip  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xA7A1A9C4
P80 = int(0.8 * 2**32)


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 1


@pytest.mark.parametrize("wl", ["c4_100k", "c4pb_100k"])
def test_bench_runner_protocol_vs_oracle(oracle, monkeypatch, wl):
    bench = pytest.importorskip("bench")
    n, m = 100_000, 1000
    shapes = {"c4_100k": (n, m, 8, avhip.INIT_BERNOULLI, P80, 0, False, "C4 shape at 100k nodes"),
              "c4pb_100k": (n, m, 8, avhip.INIT_PAIRS, 0, bench.BYZ20, False, "C4pb shape at 100k nodes")}
    monkeypatch.setitem(bench.WORKLOADS, wl, shapes[wl])
    _, _, k, init_mode, init_param, byz, _, _ = shapes[wl]
    args = argparse.Namespace(seed=SEED, shard="peers", plane_nt=None, kernel=None, rehearse_one_gpu=False)
    T = _threads()
    warmup, steps, epoch = 5, 20, bench.EPOCH

    # the oracle: one fresh network per epoch, started at the engine's round of that epoch
    state = {"sim": None, "sim_start": None, "checked": 0, "applied": 0}

    def on_segment(run, pos, seg):
        eng = run.eng
        end_round = eng.round  # engine rounds run so far (absolute)
        first = end_round - seg
        # pos = epoch position of the segment's first round; the epoch started at first - pos
        start = first - pos
        if state["sim_start"] != start:
            if state["sim"] is not None:
                state["sim"].close()
            sim = oracle.Sim(n, m, k, seed=SEED, byz_threshold=byz, init_mode=init_mode, init_param=init_param,
                             threads=T)
            sim.set_round_index(start)
            assert pos == 0, "an epoch's first segment starts at its round 0"
            state["sim"], state["sim_start"] = sim, start
        sim = state["sim"]
        assert sim.round == first, (sim.round, first)
        cnt, sm, xr, applied = 0, 0, 0, 0
        for _ in range(seg):
            (c, s_, x), a = sim.run_round(threads=T, collect=False, round_rel=sim.round - eng.log_base_round())
            cnt += c
            sm = (sm + s_) % (1 << 64)
            xr ^= x
            applied += a
        got = eng.updates_digest()
        assert got == (cnt, sm, xr), f"{wl} rounds {first}..{end_round - 1}: digest {got} != oracle {(cnt, sm, xr)}"
        assert eng.applied_votes() - state["applied"] == applied, f"{wl} rounds {first}..{end_round - 1}: applied"
        state["applied"] = eng.applied_votes()
        if seg > 1:  # a timed segment: the whole state after it
            recs = eng.read_records()
            exp = sim.dump(threads=T)
            assert np.array_equal(recs, exp), f"{wl}: state after rounds {first}..{end_round - 1} differs"
            state["checked"] += 1

    run = bench.Runner(wl, args, world=1, rank=0, local_rank=0, log_capacity=400_000_000)
    run.on_segment = on_segment
    try:
        # measure()'s sequence: device warm-up epoch, goto(warmup), the timed steps
        run.steps(epoch, timed=False)
        run.goto(warmup)
        elapsed, applied, emitted, segs = run.steps(steps, timed=True)
        assert segs == 2 and state["checked"] == 2
        assert applied == steps * n * m * k  # every record live in every timed round
        # the roofline pass repeats the same steps from a re-population
        run.goto(warmup)
        run.steps(3, timed=False)
    finally:
        run.close()
        if state["sim"] is not None:
            state["sim"].close()


def test_dump_outputs_are_what_the_last_timed_step_left(oracle, monkeypatch, tmp_path):
    """bench.py --dump-outputs on measure()'s plain path (3000 x 100 C4-shaped network, steps 0-2 of
    the epoch after the warm-up epoch: the fresh and two storm rounds): the sampled records and
    preferences, the segment's StatusUpdates, their per-round counts and digest are the oracle's,
    bit for bit; a second run writes the same files; the files are float32/float64."""
    import bench
    n, m, k = 3000, 100, 8
    monkeypatch.setitem(bench.WORKLOADS, "c4", (n, m, k, avhip.INIT_BERNOULLI, P80, 0, False, "C4 shape, 3000 x 100"))
    monkeypatch.setattr(bench, "DUMP_CELLS", 5 * bench.DUMP_RUN * m)  # 5 of the 47 runs of nodes: a real sample
    args = bench.parse(["--steps", "3", "--warmup", "0"])
    assert not args.full
    r = bench.measure("c4", args, 1, 0, 0, args.steps, args.warmup, dump=str(tmp_path / "a"))
    assert r["applied"] == args.steps * n * m * k and r["kavg_ms"] is None  # no roofline pass in a plain run
    bench.measure("c4", args, 1, 0, 0, args.steps, args.warmup, dump=str(tmp_path / "b"))
    got = {}
    for f in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
        got[f[:-4]] = a
    assert set(got) == {"sample_nodes", "records", "preferences", "status_updates", "updates_per_round",
                        "updates_digest"}

    T = _threads()
    sim = oracle.Sim(n, m, k, seed=args.seed, init_mode=avhip.INIT_BERNOULLI, init_param=P80, threads=T)
    first = bench.EPOCH  # the timed epoch starts where the warm-up epoch ended
    sim.set_round_index(first)
    ups = [sim.run_round(threads=T)[0] for _ in range(args.steps)]
    nodes = got["sample_nodes"].astype(np.int64)
    assert nodes.size == 5 * bench.DUMP_RUN and np.all(np.diff(nodes) > 0) and nodes[-1] < n
    assert np.array_equal(got["records"], sim.dump(threads=T)[nodes])
    assert np.array_equal(got["preferences"], sim.pref()[nodes])
    # the timed segment's whole pending stream (below the row limit: not sampled), canonical order
    assert all(len(x) > 0 for x in ups) and sum(len(x) for x in ups) <= bench.DUMP_UPDATES
    assert np.array_equal(got["status_updates"], np.concatenate(ups))
    assert got["updates_per_round"].tolist() == [len(x) for x in ups] + [0] * (bench.EPOCH - args.steps)
    u = np.concatenate(ups).astype(np.uint64)
    words = ((u[:, 0] - np.uint64(first)) << np.uint64(52)) | (u[:, 1] << np.uint64(28)) | (u[:, 2] << np.uint64(24)) \
        | (u[:, 3] << np.uint64(2)) | u[:, 4]
    cnt, sm, xr = oracle.update_digest(words)
    assert got["updates_digest"].tolist() == [cnt, sm >> 32, sm & 0xFFFFFFFF, xr >> 32, xr & 0xFFFFFFFF]
    sim.close()
