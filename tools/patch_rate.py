#!/usr/bin/env python3
"""Rates of mem_patch_reg against the resident reference (bsw_patch_ref_batch and its ticket forms) on one MI355X.

Shapes: those of tools/cigar_rate.py — reads of 150, 250 and 2 000 bases from both strands of a synthetic genome (2 %
substitutions, 0.5 % indels, the reference interval within 3 % of the read) — each cut at its middle into two adjacent regions
a, b with a.w = b.w = 50, so that every pair passes the pre-tests and is aligned under w_ ~ 100.  Per shape, --reps alternating
repetitions (one call of each kind per repetition, in turn), median [min - max] of the C call alone into arrays allocated before:

  patch_batch        bsw_patch_ref_batch
  cigar_batch        bsw_cigar_ref_batch on the same intervals, max_tries = 1, the band mem_patch_reg hands over, CIGAR and MD
                     returned and thrown away (what a host without this call would do)
  cigar_batch_null   the same with cigars == NULL and md == NULL (no CIGAR / MD read-back; backtrack, traceback and the NM / MD
                     kernel still run)
  patch_ticket       bsw_patch_ref_submit_t + bsw_wait_ticket
  patch_reads_ticket bsw_patch_reads_submit_t + bsw_wait_ticket on a block uploaded before (only coordinates cross PCIe)

--sweep: BSW_F4_PATCH_WORK is read once per process, so every cut 2^24 .. 2^30 (and the library's own constant) is a child
process that times the two ticket forms at the 150-base and the 2 000-base shape; the cuts are visited upwards, then downwards, --reps // 2 + 1
repetitions each time.  On several GPUs: not measured.

    python3 tools/patch_rate.py [--reps 5] [--sweep] [--out profiles/patch_rate.json]
"""
import argparse
import json
import os
import subprocess
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
SWEEP = [None] + [1 << k for k in range(24, 31)]


def genome():
    rng = np.random.default_rng(1)
    return gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))


def make_tasks(host, pac, qlen, n, seed, cache=None):
    """-> (reads uint8[n, qlen], PTASK, RD_PTASK, CTASK on the same intervals and bands, banded cells); cache: a file the
    sweep's children share (the records travel without their pointers)"""
    if cache and os.path.exists(cache):
        z = np.load(cache)
        reads, pt, rpt, ct = z["reads"], z["pt"].copy(), z["rpt"], z["ct"].copy()
        ptr = reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(qlen)
        pt["query"], ct["query"] = ptr, ptr
        return reads, pt, rpt, ct, int(z["cells"])
    rng = np.random.default_rng(seed)
    p = host.default_params()
    mat, pen = p["mat"][0], (int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0]))
    reads = np.zeros((n, qlen), dtype=np.uint8)
    pt, rpt, ct = np.zeros(n, host.PTASK), np.zeros(n, host.RD_PTASK), np.zeros(n, host.CTASK)
    cells, cut = 0, qlen // 2
    for i in range(n):
        rlen = qlen + int(rng.integers(-qlen * 3 // 100, qlen * 3 // 100 + 1))
        rb = (L_PAC if i & 1 else 0) + int(rng.integers(0, L_PAC - rlen))
        re = rb + rlen
        reads[i] = _gen.mutate(rng, gc.bns_get_seq(pac, L_PAC, rb, re), qlen, 0.02, 0.005)
        a = (rb, rb + cut, 0, cut, cut, 50)
        b = (re - (qlen - cut), re, cut, qlen, qlen - cut, 50)
        for t in (pt, rpt):
            t[i]["a"], t[i]["b"] = a, b
        pt[i]["query"], pt[i]["l_query"], rpt[i]["read"] = reads[i].ctypes.data, qlen, i
        runs, w_ = host.patch_pretest(p, L_PAC, pt[i]["a"], pt[i]["b"])
        assert runs, (a, b)
        ct[i]["query"], ct[i]["l_query"], ct[i]["w"], ct[i]["rb"], ct[i]["re"] = reads[i].ctypes.data, qlen, w_, rb, re
        ct[i]["min_score"], ct[i]["max_tries"] = -(1 << 31), 1
        cells += min(qlen, 2 * gc.band(mat, *pen, qlen, rlen, w_) + 1) * rlen
    if cache:
        np.savez(cache, reads=reads, pt=pt, rpt=rpt, ct=ct, cells=cells)
    return reads, pt, rpt, ct, cells


def spread(ts):
    ts = sorted(ts)
    return dict(median_s=round(ts[len(ts) // 2], 6), min_s=round(ts[0], 6), max_s=round(ts[-1], 6), reps=len(ts))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def calls_of(host, ctx, ref, rd, p, pt, rpt, ct, qlen):
    """the five timed calls, each into arrays allocated and touched before"""
    import ctypes as C
    L, n = host.lib(), len(pt)
    pres, cres = np.zeros(n, host.PRESULT), np.zeros(n, host.CRESULT)
    max_cigar, max_md = 64 + qlen // 8, 256 + qlen * 2
    cig, md = np.zeros((n, max_cigar), np.uint32), np.zeros((n, max_md), np.uint8)

    def ok(rc):
        assert rc == 0, (rc, ctx.last_error() if hasattr(ctx, "last_error") else "")

    def patch_batch():
        ok(L.bsw_patch_ref_batch(ctx.handle, p.ctypes.data, ref, pt.ctypes.data, n, pres.ctypes.data))

    def cigar_batch():
        ok(L.bsw_cigar_ref_batch(ctx.handle, p.ctypes.data, ref, ct.ctypes.data, n, max_cigar, cig.ctypes.data, max_md, md.ctypes.data, cres.ctypes.data))

    def cigar_batch_null():
        ok(L.bsw_cigar_ref_batch(ctx.handle, p.ctypes.data, ref, ct.ctypes.data, n, max_cigar, None, max_md, None, cres.ctypes.data))

    def patch_ticket():
        t = C.c_uint64(0)
        ok(L.bsw_patch_ref_submit_t(ctx.handle, p.ctypes.data, ref, pt.ctypes.data, n, pres.ctypes.data, C.byref(t)))
        ok(L.bsw_wait_ticket(ctx.handle, t))

    def patch_reads_ticket():
        t = C.c_uint64(0)
        ok(L.bsw_patch_reads_submit_t(ctx.handle, p.ctypes.data, ref, rd, rpt.ctypes.data, n, pres.ctypes.data, C.byref(t)))
        ok(L.bsw_wait_ticket(ctx.handle, t))
    return dict(patch_batch=patch_batch, cigar_batch=cigar_batch, cigar_batch_null=cigar_batch_null, patch_ticket=patch_ticket,
                patch_reads_ticket=patch_reads_ticket), pres, cres


def measure(host, ctx, ref, pac, name, qlen, n, reps, only=None, cache=None):
    p = host.default_params()
    reads, pt, rpt, ct, cells = make_tasks(host, pac, qlen, n, qlen * 17 + 3, cache)
    rd = ctx.reads_upload([reads[i] for i in range(n)])
    try:
        calls, pres, cres = calls_of(host, ctx, ref, rd, p, pt, rpt, ct, qlen)
        names = [k for k in calls if only is None or k in only]
        for k in names:
            calls[k]()                                                   # warm-up (allocations)
        if "cigar_batch" in names and "patch_batch" in names:
            calls["cigar_batch"]()
            want = cres["score"].copy()
            calls["patch_batch"]()
            assert (pres["gscore"] == want).all() and (pres["status"] != 1).all()       # the same alignments, the same scores
        st0 = ctx.host_stats()
        ts = {k: [] for k in names}
        for _ in range(reps):
            for k in names:
                ts[k].append(timed(calls[k]))
        st1 = ctx.host_stats()
        row = dict(shape=name, qlen=qlen, tasks=n, cells=int(cells), merged=int((pres["status"] == 0).sum()))
        for k in names:
            row[k] = dict(spread(ts[k]), aln_per_s=round(n / sorted(ts[k])[len(ts[k]) // 2], 1))
        tickets = sum(reps for k in names if k.endswith("ticket"))
        if tickets:
            row["chunks_per_ticket"] = round(float(st1["chunks"] - st0["chunks"]) / tickets, 2)
            row["d2h_bytes_per_task_ticket"] = round(float(st1["d2h_bytes"] - st0["d2h_bytes"]) / tickets / n, 2)
        return row
    finally:
        ctx.reads_free(rd)


def child(reps, out):
    host = graft.load_package().host
    pac = genome()
    with host.BswContext(device=0) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        try:
            row = {}
            for name, qlen, n in (SHAPES[0], SHAPES[2]):
                row[name] = measure(host, ctx, ref, pac, name, qlen, n, reps, only=("patch_ticket", "patch_reads_ticket"), cache="%s.%s.npz" % (out, name))
        finally:
            ctx.ref_free(ref)
    with open(out, "w") as f:
        json.dump(row, f)


def sweep(reps, tmp):
    """every cut in a fresh process, upwards then downwards; the repetitions of both visits are pooled"""
    pool = {}
    half = reps // 2 + 1
    for work in SWEEP + SWEEP[::-1]:
        env = dict(os.environ)
        env.pop("BSW_F4_PATCH_WORK", None)
        if work:
            env["BSW_F4_PATCH_WORK"] = str(work)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, "--reps", str(half)], env=env, check=True, timeout=600)
        row = json.load(open(tmp))
        pool.setdefault(work, []).append(row)
    rows = []
    for work, name in [(w, nm) for nm in (SHAPES[0][0], SHAPES[2][0]) for w in SWEEP]:
        a, b = pool[work][0][name], pool[work][1][name]
        r = dict(work=work or "library constant", shape=a["shape"], tasks=a["tasks"], cells=a["cells"], chunks_per_ticket=a["chunks_per_ticket"])
        for k in ("patch_ticket", "patch_reads_ticket"):
            lo, hi = min(a[k]["min_s"], b[k]["min_s"]), max(a[k]["max_s"], b[k]["max_s"])
            r[k] = dict(visit_medians_s=[a[k]["median_s"], b[k]["median_s"]], min_s=lo, max_s=hi, reps=a[k]["reps"] + b[k]["reps"])
        print(json.dumps(r), flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.child)
        return
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.sweep:                                                          # (before this process opens the GPU itself)
        doc["sweep"] = sweep(a.reps, (a.out or "patch_rate") + ".child.tmp")
        for ext in ("", ".q150.npz", ".q2000.npz"):
            os.remove((a.out or "patch_rate") + ".child.tmp" + ext)
    host = graft.load_package().host
    pac = genome()
    rows = []
    with host.BswContext(device=0) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        try:
            for name, qlen, n in SHAPES:
                r = measure(host, ctx, ref, pac, name, qlen, n, a.reps)
                print(json.dumps(r), flush=True)
                rows.append(r)
        finally:
            ctx.ref_free(ref)
    doc["rates"] = rows
    doc["note"] = "one MI355X; median [min - max] of alternating repetitions; several GPUs: not measured"
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
