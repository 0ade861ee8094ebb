#!/usr/bin/env python3
"""Run a BASELINE config until every honest node has finalized every target
(or a round limit), one GPU, and report rounds-to-finalization plus the
per-round kernel throughput.

    python tools/run_to_finalization.py --workload c3 [--max-rounds 512] [--json out.json] [--census]
                                        [--loss P] [--loss-mode skip|neutral] [--down F]
                                        [--degree D | --partition G]

--census adds, per round and from one Engine.census() call over the honest nodes: the targets on
which no honest node holds a live record, the honest nodes that hold none at all (the example's
"fully finalized" nodes, main.go:143-162), and the minimum over targets of the larger of the two
accepted-side node counts (nodes holding the target accepted, nodes that finalized it accepted):
how far the least advanced target's acceptance has got.

--loss P loses each Response with probability P (rule R5, av_set_loss), --loss-mode says what a lost
Response does (skip: it never arrives; neutral: it arrives with neutral votes), --down F marks a
fraction F of the nodes, evenly spread, as not responding (av_set_responding). Defaults: a perfect
network. The report then carries the lost Responses per round.

--degree D gives every node a random ascending list of D peers to poll from, --partition G splits the
network into G equal groups with complete lists inside each group (rule R6, av_set_peer_lists;
tools/topologies.py builds both). The report then carries the unsent polls per round (nodes with
fewer than k peers); a partitioned network finalizes group by group, each on its own majority.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-avalanche_amd", "python"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import avhip  # noqa: E402
import topologies  # noqa: E402
from bench import WORKLOADS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=["c3", "c4", "c5"])
    ap.add_argument("--max-rounds", type=int, default=512)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xA7A1A9C4)
    ap.add_argument("--json", default=None)
    ap.add_argument("--census", action="store_true", help="per-round network census (see above)")
    ap.add_argument("--loss", type=float, default=0.0, help="probability that a Response is lost")
    ap.add_argument("--loss-mode", default="skip", choices=["skip", "neutral"])
    ap.add_argument("--down", type=float, default=0.0, help="fraction of the nodes that do not respond")
    topo = ap.add_mutually_exclusive_group()
    topo.add_argument("--degree", type=int, default=0, help="random peer lists of this many peers per node")
    topo.add_argument("--partition", type=int, default=0, help="this many equal groups, complete inside")
    args = ap.parse_args()
    n, m, k, init_mode, init_param, byz, replay, desc = WORKLOADS[args.workload]
    assert not replay
    # log sized for the heaviest round (every record can emit up to 2 updates per round at k=8);
    # capped at 2^31 entries (16 GB) — a round beyond that is reported as overflow
    log_cap = min(2 * n * m + (1 << 20), 1 << 31)
    e = avhip.Engine(n, m, k=k, seed=args.seed, byz_threshold=byz, log_capacity=log_cap)
    e.init_records(init_mode, init_param)
    lossy = args.loss > 0 or args.down > 0
    if args.loss > 0:
        e.set_loss(min(int(args.loss * 2**32), 2**32 - 1),
                   avhip.LOSS_NEUTRAL if args.loss_mode == "neutral" else avhip.LOSS_SKIP)
    elif args.down > 0:
        e.set_loss(0, avhip.LOSS_NEUTRAL if args.loss_mode == "neutral" else avhip.LOSS_SKIP)
    n_down = int(args.down * n)
    if n_down:
        e.set_responding(np.arange(n_down, dtype=np.int64) * n // n_down, 0)
    listed = args.degree > 0 or args.partition > 0
    if listed:
        e.set_peer_lists_csr(*(topologies.random_lists(n, args.degree, args.seed & 0xFFFFFFFF) if args.degree
                               else topologies.group_lists(n, args.partition)))
    honest_records = e.live_records(honest_only=True)
    per_round = []
    t_start = time.perf_counter()
    done_round = None
    for r in range(args.max_rounds):
        a0, f0 = e.applied_votes(), e.finalized_count()
        l0 = e.lost_responses() if lossy else 0
        u0 = e.unsent_polls() if listed else 0
        e.set_timing(True)
        e.run_rounds(1)
        ms, _ = e.kernel_stats()
        e.set_timing(False)
        emitted = e.updates_count()  # StatusUpdates this round (log sized for the heaviest round)
        e.discard_updates()  # convergence only needs the counters
        live = e.live_records(honest_only=True)
        per_round.append({"round": r, "kernel_ms": ms, "applied": e.applied_votes() - a0,
                          "finalized": e.finalized_count() - f0, "emitted": emitted, "honest_live": live})
        if lossy:
            per_round[-1]["lost"] = e.lost_responses() - l0
        if listed:
            per_round[-1]["unsent"] = e.unsent_polls() - u0
        if args.census:
            c = e.census(honest_only=True, count_sum=False, hist=False)
            tc, nc = c["target_classes"], c["node_classes"]
            counted = nc.sum(axis=1) > 0  # Byzantine rows are zero
            larger = np.maximum(tc[:, avhip.CENSUS_LIVE_ACCEPTED], tc[:, avhip.CENSUS_ABSENT_ACCEPTED])
            per_round[-1].update({
                "targets_without_live": int(((tc[:, 0] + tc[:, 1]) == 0).sum()),
                "honest_nodes_done": int((counted & ((nc[:, 0] + nc[:, 1]) == 0)).sum()),
                "min_accepted_side_nodes": int(larger.min()),
            })
        if live == 0:
            done_round = r
            break
    wall = time.perf_counter() - t_start
    total_applied = e.applied_votes()
    kern = sum(x["kernel_ms"] for x in per_round)
    out = {
        "workload": desc,
        "n_nodes": n, "n_targets": m, "k": k,
        "honest_records": honest_records,
        "rounds_to_finalization": None if done_round is None else done_round + 1,
        "rounds_run": len(per_round),
        "honest_live_at_end": per_round[-1]["honest_live"],
        "applied_votes": total_applied,
        **({"loss": args.loss, "loss_mode": args.loss_mode, "nodes_down": n_down,
            "lost_responses": e.lost_responses()} if lossy else {}),
        **({"degree": args.degree, "partition": args.partition, "unsent_polls": e.unsent_polls()} if listed else {}),
        "kernel_ms_total": kern,
        "updates_per_s_kernel": total_applied / (kern * 1e-3) if kern else None,
        "wall_s": wall,
        "per_round": per_round,
    }
    print(json.dumps({k_: v for k_, v in out.items() if k_ != "per_round"}, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
