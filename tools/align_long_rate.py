#!/usr/bin/env python3
"""Rates of ksw_align2 on bsw_align_long_kernel (bsw_set_align_long; rows of H, E and Hmax in LDS) on one MI355X.

Shapes (query x target, 16-bit mode, xtra = KSW_XSUBO | KSW_XSTART | 19, the query a mutated piece of the target):
  2 000 x 2 600 and 8 191 x 8 400 under mode 1 (the only route such queries have);
  150 x 550 and 1 024 x 1 600 under mode 2, beside the register kernel (bsw_align_kernel) on the same tasks under mode 0.
Every configuration is run once per round, 7 rounds, in this order, in one process (so the two kernels of a shared shape alternate);
per configuration: alignments/s and GCUPS (cells = qlen x tlen per alignment: the main pass, not the start-point pass) of
bsw_align_batch, host packing and copies included, as median [min - max].  One JSON line per configuration; --out writes the list,
with the ratio register kernel / LDS-row kernel at the shared shapes.

    python3 tools/align_long_rate.py [--rounds 7] [--out profiles/align_long_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _gen  # noqa: E402

XSUBO, XSTART = 0x40000, 0x80000
# name, qlen, tlen, tasks, mode
CONFIGS = [
    ("q2000_t2600_long", 2000, 2600, 4096, 1),
    ("q8191_t8400_long", 8191, 8400, 512, 1),
    ("q150_t550_register", 150, 550, 65536, 0),
    ("q150_t550_long", 150, 550, 65536, 2),
    ("q1024_t1600_register", 1024, 1600, 8192, 0),
    ("q1024_t1600_long", 1024, 1600, 8192, 2),
]


def make_tasks(host, qlen, tlen, n, seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(64):                               # 64 distinct pairs, repeated
        t = rng.integers(0, 4, tlen).astype(np.uint8)
        q = _gen.mutate(rng, t[int(rng.integers(0, tlen - qlen)):], qlen, 0.03, 0.01)
        pairs.append((q, t))
    at = np.zeros(n, dtype=host.ATASK)
    for i in range(n):
        q, t = pairs[i % 64]
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = q.ctypes.data, t.ctypes.data, qlen, tlen, XSUBO | XSTART | 19
    return at, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    host = graft.load_package().host
    p = host.default_params()
    work = {c[0]: make_tasks(host, c[1], c[2], c[3], c[1] * 3 + c[2]) for c in CONFIGS}
    times = {c[0]: [] for c in CONFIGS}
    first = {}
    try:
        with host.BswContext(device=0) as ctx:
            for name, qlen, tlen, n, mode in CONFIGS:     # warm-up: kernels loaded, staging reserved
                host.set_align_long(mode)
                first[name] = ctx.align_batch(p, work[name][0])
            for _ in range(a.rounds):
                for name, qlen, tlen, n, mode in CONFIGS:
                    host.set_align_long(mode)
                    t0 = time.perf_counter()
                    ctx.align_batch(p, work[name][0])
                    times[name].append(time.perf_counter() - t0)
    finally:
        host.set_align_long(0)
    for shape in ("q150_t550", "q1024_t1600"):            # the two kernels computed the same
        assert first[shape + "_register"].tobytes() == first[shape + "_long"].tobytes(), shape
    rows = []
    for name, qlen, tlen, n, mode in CONFIGS:
        ts = sorted(times[name])
        cells = float(qlen) * tlen * n

        def rate(t):
            return dict(aln_per_s=round(n / t, 1), gcups=round(cells / t / 1e9, 3))
        r = dict(config=name, qlen=qlen, tlen=tlen, tasks=n, align_long_mode=mode, kernel="bsw_align_kernel" if mode == 0 else "bsw_align_long_kernel",
                 rounds=len(ts), seconds=[round(t, 5) for t in times[name]], median=rate(statistics.median(ts)), slowest=rate(ts[-1]), fastest=rate(ts[0]),
                 mean_score=float(first[name]["score"].mean()))
        print(json.dumps(r), flush=True)
        rows.append(r)
    by = {r["config"]: r for r in rows}
    for shape in ("q150_t550", "q1024_t1600"):
        r = dict(config=shape + "_register_over_long", ratio_of_median_aln_per_s=round(by[shape + "_register"]["median"]["aln_per_s"] / by[shape + "_long"]["median"]["aln_per_s"], 2))
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
