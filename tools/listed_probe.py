#!/usr/bin/env python3
"""Time the round over per-node peer lists (rule R6, k_round_listed) against the round that moves the
same planes through the same body: R5's skip round (k_round_lossy) with one node marked down, which
loses next to nothing. HIP-event kernel time per round, the variants alternated inside one process,
each on its own engine, armed from round 0 and taken through the same warm-up.

    python tools/listed_probe.py [--workload c4] [--shapes deg64,deg9,groups1000] [--warmup 1] [--rounds 3]
                                 [--reps 3] [--json out.json]

Shapes: degN = random lists of N peers per node, groupsS = complete lists inside groups of S nodes
(tools/topologies.py). With --warmup 1 --rounds 3 the timed rounds are rounds 1-3 of the network.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-avalanche_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import avhip  # noqa: E402
import topologies  # noqa: E402
from bench import WORKLOADS  # noqa: E402

BASE = "lossy_skip_1down"


def lists_of(shape, n):
    if shape.startswith("deg"):
        return topologies.random_lists(n, int(shape[3:]))
    if shape.startswith("groups"):
        return topologies.group_lists(n, n // int(shape[6:]))
    raise ValueError(shape)


def timed_rounds(e, init, warmup, rounds):
    """Re-initialise, run `warmup` rounds of the variant, then time `rounds` more one by one."""
    e.synchronize()
    e.discard_updates()
    e.init_records(*init)
    for _ in range(warmup):
        e.run_rounds(1)
        e.synchronize()
        e.discard_updates()
    ms, b0, u0 = [], e.alg_bytes(), e.unsent_polls()
    for _ in range(rounds):
        e.set_timing(True)
        e.kernel_stats()
        e.run_rounds(1)
        t, n = e.kernel_stats()
        e.set_timing(False)
        assert n == 1, n
        e.discard_updates()
        ms.append(t)
    return ms, e.alg_bytes() - b0, e.unsent_polls() - u0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--shapes", default="deg64,deg9,groups1000")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, m, k, init_mode, init_param, byz, replay, desc = WORKLOADS[args.workload]
    assert not replay and m <= 4096
    shapes = [s for s in args.shapes.split(",") if s]
    variants = [BASE] + shapes
    entries, engines = {}, {}
    for name in variants:
        e = avhip.Engine(n, m, k=k, seed=0xA7A1A9C4, byz_threshold=byz, log_capacity=0)
        lanes = e.layout_info()["lanes"]
        e.resize_log(2 * lanes, lanes, lanes)
        # armed once: the down node, or the lists, stand through every re-initialisation
        if name == BASE:
            e.set_responding([0], 0)
        else:
            t0 = time.perf_counter()
            offs, peers = lists_of(name, n)
            t1 = time.perf_counter()
            e.set_peer_lists_csr(offs, peers)
            entries[name] = int(peers.size)
            del offs, peers  # (one shape's host arrays at a time)
            print(json.dumps({"shape": name, "list_entries": entries[name], "build_s": round(t1 - t0, 1),
                              "set_s": round(time.perf_counter() - t1, 1)}), flush=True)
        engines[name] = e
    lanes = engines[BASE].layout_info()["lanes"]
    rows = []
    for rep in range(args.reps + 1):  # the first pass warms every shape up and is not reported
        for name in variants:
            ms, nbytes, unsent = timed_rounds(engines[name], (init_mode, init_param), args.warmup, args.rounds)
            if rep == 0:
                continue
            row = {"variant": name, "rep": rep, "ms_per_round": ms, "ms_median": sorted(ms)[len(ms) // 2],
                   "model_bytes_per_lane": nbytes / (args.rounds * lanes), "unsent_per_round": unsent / args.rounds}
            rows.append(row)
            print(json.dumps(row), flush=True)
    med = {v: sorted(r["ms_median"] for r in rows if r["variant"] == v)[args.reps // 2] for v in variants}
    out = {"workload": desc, "n_nodes": n, "n_targets": m, "k": k, "warmup": args.warmup, "rounds": args.rounds,
           "list_entries": entries, "median_ms": med,
           "over_" + BASE: {s: med[s] / med[BASE] for s in shapes}, "rows": rows}
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "rows"}, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
