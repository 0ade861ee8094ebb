#!/usr/bin/env python3
"""Admission (av_admit_targets) against bulk initialisation (av_init_records) on one workload's
engine: host-clock time of each call, which ends in a stream synchronise, as the median of --reps
after one warm-up.

    python tools/admit_probe.py [--workload c4] [--reps 5] [--sweep 1,2,4,8,16,24,32] [--json out.json]

 (a) init_records(BERNOULLI)
 (b) admit_targets of every target on an AV_INIT_NONE engine
 (c) admit_targets of one 32-target block after that block was written absent
 (d) the same one block through both thread mappings (option admit_map 1 / 2)
 b_uncounted, c_uncounted: (b) and (c) with added_nodes = NULL (nothing counted or copied back)
 sweep: the first TB blocks of an AV_INIT_NONE engine through both mappings (the host's switch point)

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-avalanche_amd", "python"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import avhip  # noqa: E402
from bench import WORKLOADS  # noqa: E402

P80 = int(0.8 * 2**32)


def timed(reps, prepare, call):
    """Median milliseconds of call() over reps runs after one warm-up; prepare() runs untimed before each."""
    ms = []
    for i in range(reps + 1):
        prepare()
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if i:
            ms.append(dt)
    return round(statistics.median(ms), 4), [round(v, 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="1,2,4,8,16,24,32")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, m, k, _, _, byz, _, _ = WORKLOADS[args.workload]
    e = avhip.Engine(n, m, k=k, seed=0xA7A1A9C4, byz_threshold=byz, log_capacity=0)
    bl = e.layout_info()["local_blocks"]
    every = np.arange(m, dtype=np.int64)
    block0 = np.arange(min(32, m), dtype=np.int64)
    absent = np.full((n, block0.size), avhip.ABSENT_WORD, np.uint32)
    out = {"workload": args.workload, "n": n, "m": m, "k": k, "blocks": bl, "reps": args.reps}

    def sync():
        e.synchronize()

    def prep(amap, fn):  # untimed: the mapping, then the state the call starts from
        def go():
            e.set_option("admit_map", amap)
            fn()
            e.synchronize()
        return go

    def admit(targets, expect=None):
        got = e.admit_targets(targets, avhip.INIT_BERNOULLI, P80, count=expect is not None)
        if expect is not None:
            assert (got == expect).all(), (got.min(), got.max(), expect)

    out["a_init_ms"], out["a_all"] = timed(args.reps, sync, lambda: e.init_records(avhip.INIT_BERNOULLI, P80))
    out["b_admit_all_ms"], out["b_all"] = timed(args.reps, prep(0, lambda: e.init_records(avhip.INIT_NONE, 0)),
                                                lambda: admit(every, n))
    out["b_uncounted_ms"], _ = timed(args.reps, prep(0, lambda: e.init_records(avhip.INIT_NONE, 0)), lambda: admit(every))
    one_absent = lambda: e.write_records(absent, t0=0)
    out["c_uncounted_ms"], _ = timed(args.reps, prep(0, one_absent), lambda: admit(block0))
    out["c_admit_block_ms"], out["c_all"] = timed(args.reps, prep(0, one_absent), lambda: admit(block0, n))
    out["d_block_major_ms"], out["d1_all"] = timed(args.reps, prep(1, one_absent), lambda: admit(block0, n))
    out["d_lane_major_ms"], out["d2_all"] = timed(args.reps, prep(2, one_absent), lambda: admit(block0, n))
    out["c_over_b"] = round(out["c_admit_block_ms"] / out["b_admit_all_ms"], 4)
    out["b_over_a"] = round(out["b_admit_all_ms"] / out["a_init_ms"], 4)
    sweep = []
    for tb in [int(x) for x in args.sweep.split(",") if x]:
        tb = min(tb, bl)
        targets = np.arange(min(32 * tb, m), dtype=np.int64)
        row = {"touched_blocks": tb}
        for name, amap in (("block_major_ms", 1), ("lane_major_ms", 2)):
            row[name], _ = timed(args.reps, prep(amap, lambda: e.init_records(avhip.INIT_NONE, 0)), lambda: admit(targets, n))
        sweep.append(row)
    out["sweep"] = sweep
    e.close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
