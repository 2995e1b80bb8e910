#!/usr/bin/env python3
"""Rates of bwa_gen_cigar2 against the resident reference (bsw_cigar_ref_batch): score, CIGAR, NM and MD per alignment.

Shapes: reads of 150, 250 and 2 000 bases from both strands of a synthetic genome (2 % substitutions, 0.5 % indels), target
+- 3 %, w_ = 100; once with every task a single try and once with 10 % of them in mem_reg2aln's loop (w_ = 25, w_cap = 100,
min_score out of reach, up to 3 tries).  Per shape: alignments/s and GCUPS (cells = banded cells of every try the
restatement in tests/_gencigar_ref.py runs) of bsw_cigar_ref_batch (reads cross PCIe, best of --reps), and beside it
bsw_global_batch on the same first tries with targets fetched, reversed and banded on the host (the DP and traceback
without the resident fetch, retries or NM / MD; host fetch time not counted).  Both are timed as the C call alone, into
output arrays allocated beforehand.  --stats DIR merges a rocprofv3
--kernel-trace --stats run of this tool (its *kernel_stats.csv) into --out as each kernel's share of the GPU time.

    python3 tools/cigar_rate.py [--reps 5] [--out profiles/cigar_rate.json]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python3 tools/cigar_rate.py --reps 2
    python3 tools/cigar_rate.py --stats DIR --out profiles/cigar_rate.json       (merge only)
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _gen  # noqa: E402
import _gencigar_ref as gc  # noqa: E402

L_PAC = 4_000_003
SHAPES = [("q150", 150, 65536), ("q250", 250, 40960), ("q2000", 2000, 4096)]


def make_specs(pac, qlen, n, retry_frac, seed):
    rng = np.random.default_rng(seed)
    reads = np.zeros((n, qlen), dtype=np.uint8)
    rows = []
    for i in range(n):
        rlen = qlen + int(rng.integers(-qlen * 3 // 100, qlen * 3 // 100 + 1))
        strand = i & 1
        rb = (L_PAC if strand else 0) + int(rng.integers(0, L_PAC - rlen))
        reads[i] = _gen.mutate(rng, gc.bns_get_seq(pac, L_PAC, rb, rb + rlen), qlen, 0.02, 0.005)
        retry = rng.random() < retry_frac
        rows.append((rb, rb + rlen, 25 if retry else 100, 100 if retry else 0, 1 << 30 if retry else -(1 << 31), 3 if retry else 1))
    return reads, rows


def measure(host, ctx, ref, pac, name, qlen, n, retry_frac, reps):
    p = host.default_params()
    mat, pen = p["mat"][0], (int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0]))
    reads, rows = make_specs(pac, qlen, n, retry_frac, qlen * 13 + int(retry_frac * 100))
    ct = np.zeros(n, dtype=host.CTASK)
    for i, (rb, re, w, w_cap, min_score, max_tries) in enumerate(rows):
        ct[i]["query"], ct[i]["l_query"], ct[i]["w"], ct[i]["rb"], ct[i]["re"] = reads[i].ctypes.data, qlen, w, rb, re
        ct[i]["w_cap"], ct[i]["min_score"], ct[i]["max_tries"] = w_cap, min_score, max_tries
    max_cigar, max_md = 64 + qlen // 8, 256 + qlen * 2
    # the C call alone, into output arrays allocated and touched once (the Python wrapper's MD strings are not timed)
    res = np.zeros(n, dtype=host.CRESULT)
    cig = np.zeros((n, max_cigar), dtype=np.uint32)
    md = np.zeros((n, max_md), dtype=np.uint8)
    L = host.lib()

    def call():
        rc = L.bsw_cigar_ref_batch(ctx.handle, p.ctypes.data, ref, ct.ctypes.data, n, max_cigar, cig.ctypes.data, max_md,
                                   md.ctypes.data, res.ctypes.data)
        assert rc == 0, rc
    call()                                                                                   # warm-up (allocations)
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        best = min(best, time.perf_counter() - t0)
    # cells: every try bsw_cigar_ref_batch runs (a try whose band repeats the previous one is not run)
    cells, cells1 = 0, 0
    gt = np.zeros(n, dtype=host.GTASK)
    keep = []
    for i, (rb, re, w, w_cap, min_score, max_tries) in enumerate(rows):
        rlen = re - rb
        bands, w2 = [], w
        for _ in range(int(res["tries"][i])):
            w2 = min(w2, w_cap or w)
            b = gc.band(mat, *pen, qlen, rlen, w2)
            if not bands or b != bands[-1]:
                bands.append(b)
            w2 <<= 1
        cells += sum(min(qlen, 2 * b + 1) * rlen for b in bands)
        cells1 += min(qlen, 2 * bands[0] + 1) * rlen
        rseq = gc.bns_get_seq(pac, L_PAC, rb, re)
        q = reads[i]
        if rb >= L_PAC:
            q, rseq = q[::-1].copy(), rseq[::-1].copy()
        keep += [q, rseq]
        gt[i]["query"], gt[i]["target"], gt[i]["qlen"], gt[i]["tlen"], gt[i]["w"] = q.ctypes.data, rseq.ctypes.data, qlen, rlen, bands[0]
    gres = np.zeros(n, dtype=host.GRESULT)

    def gcall():
        rc = L.bsw_global_batch(ctx.handle, p.ctypes.data, gt.ctypes.data, n, max_cigar, gres.ctypes.data, cig.ctypes.data)
        assert rc == 0, rc
    gcall()
    gbest = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        gcall()
        gbest = min(gbest, time.perf_counter() - t0)
    return dict(shape=name, qlen=qlen, tasks=n, retried=retry_frac, tries_mean=round(float(res["tries"].mean()), 3),
                status_nonzero=int((res["status"] != 0).sum()), cells=int(cells), s=round(best, 5),
                aln_per_s=round(n / best, 1), gcups=round(cells / best / 1e9, 3),
                global_batch_s=round(gbest, 5), global_batch_aln_per_s=round(n / gbest, 1),
                global_batch_gcups=round(cells1 / gbest / 1e9, 3))


def merge_stats(d, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel_stats.csv under %s" % d
    tot, per = 0.0, {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            name = row["Name"].split("(")[0].replace("void ", "")
            per[name] = per.get(name, 0.0) + ns
            tot += ns
    shares = {k: round(v / tot, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_share"] = dict(note="share of GPU kernel time in a rocprofv3 --kernel-trace --stats run of this tool "
                                    "(--reps 2: every shape, bsw_cigar_ref_batch and bsw_global_batch)", shares=shares)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["kernel_share"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        merge_stats(a.stats, a.out)
        return
    host = graft.load_package().host
    rng = np.random.default_rng(1)
    pac = gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))
    rows = []
    with host.BswContext(device=0) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        try:
            for name, qlen, n in SHAPES:
                for frac in (0.0, 0.1):
                    r = measure(host, ctx, ref, pac, name, qlen, n, frac, a.reps)
                    print(json.dumps(r), flush=True)
                    rows.append(r)
        finally:
            ctx.ref_free(ref)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["rates"] = rows
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
