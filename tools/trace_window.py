#!/usr/bin/env python3
"""The headline workload's timed window in a rocprofv3 kernel trace of the plain `python bench.py`
(no counting-build dispatch in the trace): the `launches` sweep-round dispatches before the trace's
last write-back (`k_materialize`), which ends the last timed segment; `--writebacks` adds the
window's write-backs to the listing and to the rows written.

With `--full`: the headline workload's roofline-pass dispatches in a rocprofv3 kernel trace of `python bench.py --full`
(`--kernel-trace --output-format csv`): the bench runs the headline first, and its roofline pass is
the `launches` sweep-round dispatches before the last write-back (`k_materialize`) that precedes its
exchange pass, whose warm rounds are the first dispatches of the counting kernel build
(`k_round_sweep<8, 0, 1, false, true>`). Prints their mean
duration (to compare with the line's `roofline.kernel_ms_avg`) and writes the window's rows.

    python tools/trace_window.py TRACE.csv [--launches 20] [--writebacks] [--out window.csv]
"""
import argparse
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--writebacks", action="store_true", help="list the window's k_materialize dispatches too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = list(csv.DictReader(open(args.trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    sweep = [i for i, r in enumerate(rows) if "k_round_sweep<" in r["Kernel_Name"]]
    cc = [i for i in sweep if "k_round_sweep<8, 0, 1, false, true>" in rows[i]["Kernel_Name"]]
    # the roofline pass ends with its last segment's write-back (k_materialize) before the exchange
    # pass (whose first rounds, before count_changed is set, are ordinary sweep dispatches); a plain
    # run's timed window ends with the trace's last write-back
    limit = cc[0] if cc else len(rows)
    mats = [i for i, r in enumerate(rows) if "k_materialize" in r["Kernel_Name"] and i < limit]
    if not mats and not cc:
        raise SystemExit("neither a write-back nor a counting-build dispatch (exchange pass) in the trace")
    end = mats[-1] if mats else cc[0]
    before = [i for i in sweep if i < end]
    win = before[-args.launches:]
    nsweep = len(win)
    if args.writebacks and win:
        win = sorted(win + [i for i in mats if win[0] < i <= end])
    durs = [(int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e6 for i in win]
    sd = [d for i, d in zip(win, durs) if "k_round_sweep<" in rows[i]["Kernel_Name"]]
    print(f"{nsweep} dispatches, mean {sum(sd) / len(sd):.4f} ms, total {sum(sd):.4f} ms")
    if len(durs) > len(sd):
        print(f"{len(durs) - len(sd)} write-backs, total {sum(durs) - sum(sd):.4f} ms; window total {sum(durs):.4f} ms")
    for i, d in zip(win, durs):
        print(f"  {rows[i]['Kernel_Name'][:60]:60s} {d:.4f} ms")
    if args.out:
        with open(args.out, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
            w.writeheader()
            for i in win:
                w.writerow(rows[i])


if __name__ == "__main__":
    main()
