#!/usr/bin/env python3
"""Rates of the banded global alignment with CIGAR (bsw_global_batch) against the scalar oracle.

Shapes: bwa_gen_cigar2's (query 2 000 / 5 000 bases, target +- 3 %, w = 50 / 100 / 500), full width at 1 024 and 8 191
columns, and 1 000-base tasks (w = 100) on the register kernel and, in a child process under BSW_GLOBAL_LONG=1, on the LDS
ring kernel.  Per shape: alignments/s and GCUPS (cells = the oracle's banded cell count) of the batch API with CIGARs
(host packing and copies included, best of --reps), the same without CIGARs, their difference as a share of the CIGAR run
(backtrack-matrix writes + traceback + CIGAR copy: an upper bound of the traceback's share), and the oracle's
ksw_global2_ref on --threads CPU threads.  One JSON line per shape; --out writes them all as one JSON list.

    python3 tools/global_rate.py [--reps 3] [--threads 16] [--out profiles/global_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _gen  # noqa: E402
from test_gpu_global import make_gtasks  # noqa: E402

# name, qlen, w, tasks, oracle tasks timed
SHAPES = [
    ("cigar2_q2000_w50", 2000, 50, 4096, 256),
    ("cigar2_q2000_w100", 2000, 100, 4096, 256),
    ("cigar2_q2000_w500", 2000, 500, 2048, 128),
    ("cigar2_q5000_w50", 5000, 50, 2048, 128),
    ("cigar2_q5000_w100", 5000, 100, 2048, 128),
    ("cigar2_q5000_w500", 5000, 500, 1024, 64),
    ("full_q1024", 1024, 1024, 2048, 128),
    ("full_q8191", 8191, 8191, 256, 32),
]
SHAPE_1000 = ("q1000_w100", 1000, 100, 8192, 512)


def make_pairs(qlen, n, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, 4 * qlen + 1000).astype(np.uint8)
    pairs = []
    for k in range(min(n, 64)):                       # 64 distinct pairs, repeated
        tl = qlen + int(rng.integers(-qlen * 3 // 100, qlen * 3 // 100 + 1))
        s = int(rng.integers(0, len(ref) - tl))
        t = ref[s:s + tl].copy()
        pairs.append((_gen.mutate(rng, t, qlen, 0.02, 0.01), t))
    return [pairs[k % len(pairs)] for k in range(n)]


def measure(host, orc, ctx, shape, reps, threads):
    name, qlen, w, n, n_orc = shape
    p = host.default_params()
    pairs = make_pairs(qlen, n, qlen * 7 + w)
    ws = [max(w, abs(len(q) - len(t))) for q, t in pairs]
    gt, keep = make_gtasks(host, pairs, ws)
    max_cigar = 64 + qlen // 8
    ctx.global_batch(p, gt[:min(n, 64)], max_cigar=max_cigar)        # warm-up: kernels loaded, staging reserved
    best = {}
    for want in (True, False):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.global_batch(p, gt, max_cigar=max_cigar, want_cigar=want)
            ts.append(time.perf_counter() - t0)
        best[want] = min(ts)
    mat = p["mat"][0]
    cells_one = [orc.global2(q, t, mat, 6, 1, 6, 1, wk, want_cigar=False)["cells"] for (q, t), wk in zip(pairs[:64], ws[:64])]
    cells = sum(cells_one[k % len(cells_one)] for k in range(n))
    sub = list(zip(pairs[:n_orc], ws[:n_orc]))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:                           # ctypes drops the GIL inside ksw_global2_ref
        list(ex.map(lambda a: orc.global2(a[0][0], a[0][1], mat, 6, 1, 6, 1, a[1]), sub))
    t_orc = time.perf_counter() - t0
    orc_cells = sum(cells_one[k % len(cells_one)] for k in range(n_orc))
    r = dict(shape=name, qlen=qlen, w=w, tasks=n, cells=int(cells), force_long=os.environ.get("BSW_GLOBAL_LONG", ""),
             gpu_s=round(best[True], 5), gpu_score_only_s=round(best[False], 5),
             aln_per_s=round(n / best[True], 1), gcups=round(cells / best[True] / 1e9, 3),
             gcups_score_only=round(cells / best[False] / 1e9, 3),
             cigar_share=round(max(0.0, best[True] - best[False]) / best[True], 3),
             oracle_threads=threads, oracle_aln_per_s=round(n_orc / t_orc, 1), oracle_gcups=round(orc_cells / t_orc / 1e9, 4))
    r["speedup_vs_oracle"] = round(r["gcups"] / r["oracle_gcups"], 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--only-1000", action="store_true", help="(internal) the 1 000-base shape alone")
    a = ap.parse_args()
    host, orc = graft.load_package().host, graft.load_oracle()
    rows = []
    with host.BswContext(device=0) as ctx:
        for shape in ([SHAPE_1000] if a.only_1000 else SHAPES + [SHAPE_1000]):
            r = measure(host, orc, ctx, shape, a.reps, a.threads)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.only_1000:
        return
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-1000", "--reps", str(a.reps), "--threads", str(a.threads)],
                           env=dict(os.environ, BSW_GLOBAL_LONG="1"), capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit("BSW_GLOBAL_LONG=1 child failed:\n" + child.stderr[-3000:])
    for line in child.stdout.splitlines():
        if line.startswith("{"):
            print(line, flush=True)
            rows.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
