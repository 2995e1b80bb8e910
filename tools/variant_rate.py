#!/usr/bin/env python3
"""Kernels-only rate of the recurrence variants (H, RTL by default) on resident batches of the bench workloads: seeds/s,
cells per seed and GCUPS of bsw_run (DP kernels only, device-timed), one line per workload and variant.
python tools/variant_rate.py [--tasks N] [--workloads a,b] [--variants 0,2] [--reps R]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402

NAMES = {0: "H", 1: "M", 2: "RTL"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=1_000_000)
    ap.add_argument("--workloads", default="150bp_w100_mixed_bins,250bp_w500")
    ap.add_argument("--variants", default="0,2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    host = graft.load_package().host
    out = {}
    with host.BswContext(device=0) as ctx:
        for wl in args.workloads.split(","):
            spec = dict(bench.WORKLOADS[wl])
            n = args.tasks if wl != "250bp_w500" else min(args.tasks, 262144)
            ar = host.HostArena(host.synth_arena_bound(n, **spec) + 4096)
            t, _ = host.synth_tasks(n, arena=ar.u8, seed=2000, **spec)
            for v in (int(x) for x in args.variants.split(",")):
                p = host.default_params(w=spec["w"], variant=v)
                b = ctx.upload(p, t)
                ctx.run(b)
                ctx.sync()
                r = ctx.download(b)
                ctx.run_history2()
                for _ in range(args.reps):
                    ctx.run(b)
                ctx.sync()
                ms = float(np.median([x[0] for x in ctx.run_history2()]))
                cells = bench.cells_of(r)
                out["%s/%s" % (wl, NAMES[v])] = {"seeds": n, "kernels_ms": round(ms, 3), "seeds_per_s": round(n / ms * 1e3),
                                                 "cells_per_seed": round(cells / n, 1), "gcups": round(cells / ms / 1e6, 1),
                                                 "launches": b.info()["launches"]}
                b.free()
            ar.free()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
