#!/usr/bin/env python3
"""Variant RTL with the packed two-seeds-per-lane kernels off and on (bsw_set_rtl_packed): kernels-only rate of bsw_run on
resident batches of DESIGN.md §4.4's two workloads (1 M seeds of the 150 bp mix, 262 144 seeds of 250 bp / w500), device-timed.
The two routes alternate `--rounds` times in one process; each figure is median [min - max] over the rounds, a round's figure
the median of `--reps` runs.  Variant H of the same build is reported next to them.  The results with the switch on must be
the bytes of the switch off, and the packed kernel's launch counters must move only with it on.
python tools/rtl_packed_rate.py [--tasks N] [--workloads a,b] [--rounds 3] [--reps 3] [--out profiles/rtl_packed_rate.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402


def timed(ctx, b, reps):
    ctx.run(b)
    ctx.sync()
    ctx.run_history2()
    for _ in range(reps):
        ctx.run(b)
    ctx.sync()
    return float(np.median([x[0] for x in ctx.run_history2()]))


def summary(n, ms):
    rate = sorted(n / m * 1e3 for m in ms)
    return {"kernels_ms": [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)],
            "seeds_per_s": [round(float(np.median(rate))), round(rate[0]), round(rate[-1])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workloads", default="150bp_w100_mixed_bins,250bp_w500")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    host = graft.load_package().host
    out = {"format": "median [min, max] over %d alternating rounds; a round = median of %d bsw_run calls, kernels only" % (args.rounds, args.reps)}
    host.set_rtl_packed(False)
    with host.BswContext(device=0) as ctx:
        for wl in args.workloads.split(","):
            spec = dict(bench.WORKLOADS[wl])
            n = args.tasks if wl != "250bp_w500" else min(args.tasks, 262144)
            ar = host.HostArena(host.synth_arena_bound(n, **spec) + 4096)
            t, _ = host.synth_tasks(n, arena=ar.u8, seed=2000, **spec)
            res, ms = {}, {"off": [], "on": [], "H": []}
            bat = {k: ctx.upload(host.default_params(w=spec["w"], variant=v), t) for k, v in (("rtl", 2), ("H", 0))}
            launches = {}
            for rnd in range(args.rounds):
                for name in ("off", "on"):
                    s0 = host.rtl_packed_stats()
                    host.set_rtl_packed(name == "on")
                    ms[name].append(timed(ctx, bat["rtl"], args.reps))
                    host.set_rtl_packed(False)
                    launches[name] = [b - a for a, b in zip(s0, host.rtl_packed_stats())]
                    if rnd == 0:
                        res[name] = ctx.download(bat["rtl"])[:n].copy()
                ms["H"].append(timed(ctx, bat["H"], args.reps))
            assert res["on"].tobytes() == res["off"].tobytes(), "the packed route changed the results"
            assert sum(launches["off"]) == 0 and sum(launches["on"]) > 0, launches
            cells = bench.cells_of(res["on"])
            cells_h = bench.cells_of(ctx.download(bat["H"])[:n])
            out[wl] = {"seeds": n, "rtl_cells_per_seed": round(cells / n, 1), "h_cells_per_seed": round(cells_h / n, 1),
                       "rtl_packed_off": summary(n, ms["off"]), "rtl_packed_on": summary(n, ms["on"]), "variant_h": summary(n, ms["H"]),
                       "packed_launches_per_round": launches["on"], "launches": bat["rtl"].info()["launches"],
                       "speedup_on_over_off": round(float(np.median(ms["off"]) / np.median(ms["on"])), 3)}
            for b in bat.values():
                b.free()
            ar.free()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
