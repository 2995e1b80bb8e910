#!/usr/bin/env python3
"""Rates of mate rescue against the resident reference (bsw_matesw_ref_batch) beside bsw_align_batch on the same tasks.

Shapes: 150 bp mates with ~550-base windows and 250 bp mates with ~1 000-base windows (a 500 +- 50 insert, the window mem_matesw
computes), 90 % of the mates reverse-complemented (is_rev, an FR library) and 10 % forward, 64 k and 256 k tasks, mem_matesw's
xtra (KSW_XSUBO | KSW_XSTART | KSW_XBYTE when l_ms * a < 250 | min_seed_len * a).  The mates come from the windows with 2 %
substitutions; one in ten windows holds nothing (random mate).

Per shape: alignments/s of bsw_matesw_ref_batch (mates in registered memory, windows fetched and mates reverse-complemented on
the GPU) and of bsw_align_batch on the same tasks with windows and reverse-complemented mates prepared on the host (in one
registered arena: the prep is not in its time).  The host prep (bns_get_seq of every window plus the reverse complement, as
vectorised numpy gathers on one thread) is timed on its own.  H2D bytes per task: sequence bytes plus the per-task records
each call sends.  Both calls are timed as the C call alone, best of --reps.

    python3 tools/matesw_rate.py [--reps 5] [--out profiles/matesw_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _gencigar_ref as gc  # noqa: E402

L_PAC = 4_000_003
SHAPES = [("m150_w550", 150, 550), ("m250_w1000", 250, 1000)]
COUNTS = [65536, 262144]
# per-task records each call sends besides the sequences (bsw_dtask 44 + bsw_rawoff 16 + bsw_adtask 32 + order 4, and bsw_refx 16
# for the resident fetch)
REC_ALIGN, REC_RESIDENT = 44 + 16 + 32 + 4, 44 + 16 + 16 + 32 + 4


def make(rng, fwd, l_ms, wlen, n):
    """windows (rb, re) on both strands, is_rev, and the mates in read order (n x l_ms)"""
    strand = rng.integers(0, 2, n)
    wl = wlen + rng.integers(-50, 51, n)
    rb = strand * L_PAC + rng.integers(0, L_PAC - wl - 1, n)
    re = rb + wl
    is_rev = (rng.random(n) < 0.9).astype(np.int32)
    mates = gather(fwd, rb, np.full(n, l_ms, np.int64), rng.integers(0, wlen - l_ms, n))
    sub = rng.random((n, l_ms)) < 0.02
    mates[sub] = (mates[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    junk = rng.random(n) < 0.1
    mates[junk] = rng.integers(0, 4, (int(junk.sum()), l_ms))
    rc = is_rev.astype(bool)
    mates[rc] = revcomp(mates[rc])
    return rb.astype(np.int64), re.astype(np.int64), is_rev, mates


def gather(fwd, rb, length, skip=None):
    """bns_get_seq of [rb + skip, rb + skip + length) for every row (one strand each): rows padded to the longest"""
    skip = np.zeros(len(rb), np.int64) if skip is None else skip
    out = np.zeros((len(rb), int(length.max())), np.uint8)
    for a in range(0, len(rb), 16384):
        s = slice(a, a + 16384)
        x = (rb[s] + skip[s])[:, None] + np.arange(out.shape[1])[None, :]
        x = np.minimum(x, np.where(rb[s] < L_PAC, L_PAC - 1, 2 * L_PAC - 1)[:, None])
        rev = x >= L_PAC
        b = fwd[np.where(rev, 2 * L_PAC - 1 - x, x)]
        out[s] = np.where(rev, 3 - b, b)
    return out


def revcomp(m):
    return np.where(m < 4, 3 - m, 4).astype(np.uint8)[:, ::-1]


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def measure(host, ctx, ref, fwd, name, l_ms, wlen, n, reps):
    p = host.default_params()
    rng = np.random.default_rng(l_ms * 7 + n)
    rb, re, is_rev, mates = make(rng, fwd, l_ms, wlen, n)
    xtra = 0x40000 | 0x80000 | (0x10000 if l_ms < 250 else 0) | 19
    arena = host.HostArena(n * l_ms + 64)
    arena.u8[:n * l_ms] = mates.reshape(-1)
    mt = np.zeros(n, dtype=host.MTASK)
    mt["mate"] = arena.ptr + l_ms * np.arange(n, dtype=np.uint64)
    mt["l_ms"], mt["is_rev"], mt["rb"], mt["re"], mt["xtra"], mt["min_score"] = l_ms, is_rev, rb, re, xtra, 19
    ctx.matesw_ref_batch(p, ref, mt[:2000])
    res = None

    def resident():
        nonlocal res
        res = ctx.matesw_ref_batch(p, ref, mt)
    t_res = best(resident, reps)

    # bsw_align_batch: the host fetches every window and reverse-complements the mates it aligns reversed
    tl = (re - rb).astype(np.int64)

    def prep():
        w = gather(fwd, rb, tl)
        q = mates.copy()
        q[is_rev.astype(bool)] = revcomp(mates[is_rev.astype(bool)])
        return w, q
    t_prep = best(prep, max(1, reps // 2))
    w, q = prep()
    wmax = w.shape[1]
    arena2 = host.HostArena(n * (l_ms + wmax) + 64)
    arena2.u8[:n * l_ms] = q.reshape(-1)
    arena2.u8[n * l_ms:n * (l_ms + wmax)] = w.reshape(-1)
    at = np.zeros(n, dtype=host.ATASK)
    at["query"] = arena2.ptr + l_ms * np.arange(n, dtype=np.uint64)
    at["target"] = arena2.ptr + n * l_ms + wmax * np.arange(n, dtype=np.uint64)
    at["qlen"], at["tlen"], at["xtra"] = l_ms, tl, xtra
    ctx.align_batch(p, at[:2000])
    ar = None

    def aligned():
        nonlocal ar
        ar = ctx.align_batch(p, at)
    t_al = best(aligned, reps)
    same = all((res["aln"][k] == ar[k]).all() for k in host.KSWR.names)
    arena.free()
    arena2.free()
    cells = int((tl * l_ms).sum())
    return {"shape": name, "tasks": n, "l_ms": l_ms, "mean_window": round(float(tl.mean()), 1), "is_rev_frac": round(float(is_rev.mean()), 3),
            "kept_frac": round(float((res["status"] == 0).mean()), 3), "aln_equal": bool(same),
            "resident": {"seconds": round(t_res, 4), "alignments_per_s": round(n / t_res), "first_pass_GCUPS": round(cells / t_res / 1e9, 1),
                         "h2d_bytes_per_task": l_ms + REC_RESIDENT},
            "align_batch": {"seconds": round(t_al, 4), "alignments_per_s": round(n / t_al), "first_pass_GCUPS": round(cells / t_al / 1e9, 1),
                            "h2d_bytes_per_task": round(l_ms + float(tl.mean()) + REC_ALIGN, 1),
                            "host_prep_seconds": round(t_prep, 4), "host_prep_us_per_task": round(t_prep / n * 1e6, 3)},
            "resident_over_align_batch": round(t_al / t_res, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matesw_rate.json"))
    a = ap.parse_args()
    pkg = graft.load_package()
    host = pkg.host
    rng = np.random.default_rng(2026)
    fwd = rng.integers(0, 4, L_PAC).astype(np.uint8)
    pac = gc.pack_pac(fwd)
    rows = []
    with host.BswContext(device=0) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        for name, l_ms, wlen in SHAPES:
            for n in COUNTS:
                r = measure(host, ctx, ref, fwd, name, l_ms, wlen, n, a.reps)
                print(json.dumps(r), flush=True)
                rows.append(r)
        ctx.ref_free(ref)
    out = {"tool": "tools/matesw_rate.py", "reps": a.reps, "l_pac": L_PAC,
           "note": "C call alone, best of reps; align_batch's host prep (window fetch + reverse complement, numpy on one thread) "
                   "is timed separately and not in its seconds",
           "rows": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
