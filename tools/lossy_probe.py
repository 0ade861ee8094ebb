#!/usr/bin/env python3
"""Time the round with lost Responses (rule R5, k_round_lossy) against the existing kernels that move
the same planes: skip mode against the first-generation round (option kernel = 1) in its warm form,
neutral mode against the same round with warm_skip = 0. HIP-event kernel time per round, the
variants alternated inside one process, each on its own engine taken through the same warm-up.

    python tools/lossy_probe.py [--workload c4] [--loss 0.1] [--warmup 3] [--rounds 8] [--reps 3] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-avalanche_amd", "python"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

import avhip  # noqa: E402
from bench import WORKLOADS  # noqa: E402

VARIANTS = {
    # name: (options set at creation, loss mode or None)
    "firstgen_warm": ({"kernel": 1}, None),
    "lossy_skip": ({"kernel": 1}, avhip.LOSS_SKIP),
    "firstgen_full": ({"kernel": 1, "warm_skip": 0}, None),
    "lossy_neutral": ({"kernel": 1, "warm_skip": 0}, avhip.LOSS_NEUTRAL),
}


def timed_rounds(e, init, warmup, rounds, thr, mode):
    """Re-initialise, run `warmup` plain rounds, then time `rounds` rounds one by one."""
    e.set_loss(0)
    e.synchronize()
    e.discard_updates()
    e.init_records(*init)
    for _ in range(warmup):
        e.run_rounds(1)
        e.synchronize()
        e.discard_updates()
    if mode is not None:
        e.set_loss(thr, mode)
    ms, b0, l0 = [], e.alg_bytes(), e.lost_responses()
    for _ in range(rounds):
        e.set_timing(True)
        e.kernel_stats()
        e.run_rounds(1)
        t, n = e.kernel_stats()
        e.set_timing(False)
        assert n == 1, n
        e.discard_updates()
        ms.append(t)
    return ms, e.alg_bytes() - b0, e.lost_responses() - l0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4", choices=sorted(WORKLOADS))
    ap.add_argument("--loss", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    n, m, k, init_mode, init_param, byz, replay, desc = WORKLOADS[args.workload]
    assert not replay and m <= 4096
    thr = int(args.loss * 2**32)
    engines = {}
    for name, (opts, _) in VARIANTS.items():
        e = avhip.Engine(n, m, k=k, seed=0xA7A1A9C4, byz_threshold=byz, log_capacity=0)
        lanes = e.layout_info()["lanes"]
        e.resize_log(2 * lanes, lanes, lanes)
        for o, v in opts.items():
            e.set_option(o, v)
        engines[name] = e
    lanes = engines["lossy_skip"].layout_info()["lanes"]
    rows = []
    for rep in range(args.reps + 1):  # the first pass warms every shape up and is not reported
        for name, (_, mode) in VARIANTS.items():
            ms, nbytes, lost = timed_rounds(engines[name], (init_mode, init_param), args.warmup, args.rounds, thr, mode)
            if rep == 0:
                continue
            row = {"variant": name, "rep": rep, "ms_per_round": ms, "ms_median": sorted(ms)[len(ms) // 2],
                   "model_bytes_per_lane": nbytes / (args.rounds * lanes), "lost_per_round": lost / args.rounds}
            rows.append(row)
            print(json.dumps(row), flush=True)
    med = {v: sorted(r["ms_median"] for r in rows if r["variant"] == v)[args.reps // 2] for v in VARIANTS}
    out = {"workload": desc, "n_nodes": n, "n_targets": m, "k": k, "loss": args.loss, "warmup": args.warmup,
           "median_ms": med, "skip_over_firstgen_warm": med["lossy_skip"] / med["firstgen_warm"],
           "neutral_over_firstgen_full": med["lossy_neutral"] / med["firstgen_full"], "rows": rows}
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "rows"}, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
