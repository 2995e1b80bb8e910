#!/usr/bin/env python3
"""What bsw_chain2aln costs: the speculation (every seed is extended, bwa extends fewer), the host side (plan + replay), and with
--gpu the job against the bare extension ticket on the same tasks.

Workload: the seeded chains of tests/_chain2aln_ref.py (reads off both strands of a 200 kb reference with substitutions and at
most one indel; 1 - 5 chains per read: the true locus with its exact-match runs as seeds, re-seeded runs, a seed of the other
diagonal behind an indel, one-seed and thinned chains of the same locus, decoys), at fixed read lengths of 150 and 250 bases.
It is synthetic: the share of seeds that bwa skips is a property of the chains, and real chains after mem_chain_flt will differ.

  speculation   seeds extended / seeds bwa extends, from the sequential restatement alone (it extends a seed on the CPU oracle
                only when bwa's loop reaches it)
  host cost     bsw_chain2aln_plan (bsw_rd_task records) and bsw_chain2aln_replay (pair records), one thread, ns per seed,
                median [min - max] of --reps repetitions of the C call into arrays allocated before
  --gpu         bsw_chain2aln_reads_start + bsw_chain2aln_finish against bsw_submit_reads_t + bsw_wait_ticket on the plan's tasks,
                alternating repetitions, seeds per second of the C calls

    python3 tools/chain2aln_rate.py [--reads 4000] [--reps 7] [--gpu] [--out profiles/chain2aln_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _chain2aln_ref as R  # noqa: E402
import _rtl_ref  # noqa: E402


def spread(ts, n):
    ts = sorted(ts)
    return dict(median_ns_per_seed=round(ts[len(ts) // 2] / n * 1e9, 2), min_ns_per_seed=round(ts[0] / n * 1e9, 2),
                max_ns_per_seed=round(ts[-1] / n * 1e9, 2), reps=len(ts))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def cpu_row(host, oracle, read_len, n_reads, reps):
    wl = R.make_workload(n_reads, seed=100 + read_len, len_lo=read_len, len_hi=read_len)
    p = host.default_params()
    ch, sd, lens = R.arrays(host, wl)
    n = len(sd)
    regs_ref, _, cnt = R.chain2aln(R.Extender(host, oracle, _rtl_ref, p, wl), p, wl)
    L = host.lib()
    rdt = np.zeros(n, dtype=host.RD_TASK)

    def plan():
        assert L.bsw_chain2aln_plan(p.ctypes.data, wl["l_pac"], ch.ctypes.data, len(ch), sd.ctypes.data, n, lens.ctypes.data, len(lens), None,
                                    rdt.ctypes.data, None, None, 0) == 0
    plan()
    items = [(int(t["read"]), int(t["seed"]["rbeg"]), int(t["seed"]["qbeg"]), int(t["seed"]["len"]), int(t["rmax0"]), int(t["rmax1"]), int(t["tag"])) for t in rdt]
    tasks, keep = R.build_tasks(host, R.pen_of(p), wl["reads"], wl["both"], items)
    full = oracle.pair_batch(p, tasks, nthreads=8)
    pair = np.zeros(n, dtype=host.PAIR)
    for f in host.PAIR.names:
        pair[f] = full[f]
    regs, ext, start = np.zeros(n, dtype=host.CREG), np.zeros(n, dtype=np.uint8), np.zeros(len(lens) + 1, dtype=np.uint64)
    nr = C.c_size_t(0)

    def replay():
        assert L.bsw_chain2aln_replay(p.ctypes.data, None, ch.ctypes.data, len(ch), sd.ctypes.data, n, lens.ctypes.data, len(lens), pair.ctypes.data,
                                      host.RESULT_PAIR, regs.ctypes.data, C.byref(nr), ext.ctypes.data, start.ctypes.data) == 0
    replay()
    assert nr.value == len(regs_ref) == cnt["extended"] and R.same_regions(regs[:nr.value], regs_ref) is None
    tp, tr = [], []
    for _ in range(reps):
        tp.append(timed(plan))
        tr.append(timed(replay))
    both = [a + b for a, b in zip(tp, tr)]
    return dict(read_len=read_len, reads=n_reads, chains=len(ch), seeds=n, seeds_bwa_extends=cnt["extended"],
                speculation=round(n / cnt["extended"], 3), skipped_share=round(1 - cnt["extended"] / n, 3), rescued=cnt["rescued"],
                plan=spread(tp, n), replay=spread(tr, n), plan_plus_replay=spread(both, n))


def gpu_row(host, read_len, n_reads, reps):
    wl = R.make_workload(n_reads, seed=100 + read_len, len_lo=read_len, len_hi=read_len)
    p = host.default_params()
    ch, sd, lens = R.arrays(host, wl)
    n = len(sd)
    L = host.lib()
    rdt, _ = host.chain2aln_plan(p, wl["l_pac"], ch, sd, lens)
    regs, ext, start = np.zeros(n, dtype=host.CREG), np.zeros(n, dtype=np.uint8), np.zeros(len(lens) + 1, dtype=np.uint64)
    nr = C.c_size_t(0)
    with host.BswContext(device=0, result_format=host.RESULT_PAIR) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        arena = host.HostArena(n * host.PAIR.itemsize + 64)
        out = arena.view(host.PAIR, n)
        try:
            def job():
                h = C.c_void_p()
                assert L.bsw_chain2aln_reads_start(c.handle, p.ctypes.data, None, ref, rd, ch.ctypes.data, len(ch), sd.ctypes.data, n, C.byref(h)) == 0
                assert L.bsw_chain2aln_finish(h, regs.ctypes.data, C.byref(nr), ext.ctypes.data, start.ctypes.data, None) == 0

            def bare():
                t = C.c_uint64(0)
                assert L.bsw_submit_reads_t(c.handle, p.ctypes.data, ref, rd, rdt.ctypes.data, n, out.ctypes.data, C.byref(t)) == 0
                assert L.bsw_wait_ticket(c.handle, t) == 0
            job()
            bare()
            tj, tb = [], []
            for _ in range(reps):
                tj.append(timed(job))
                tb.append(timed(bare))
        finally:
            del out
            arena.free()
            c.reads_free(rd)
            c.ref_free(ref)

    def rate(ts):
        ts = sorted(ts)
        return dict(median_seeds_per_s=round(n / ts[len(ts) // 2], 1), min_s=round(ts[0], 6), median_s=round(ts[len(ts) // 2], 6), max_s=round(ts[-1], 6), reps=len(ts))
    return dict(read_len=read_len, reads=n_reads, seeds=n, regions=int(nr.value), job_start_to_finish=rate(tj), bare_submit_reads_ticket=rate(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = graft.load_package().host
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    if a.gpu:
        rows = [gpu_row(host, rl, a.reads, a.reps) for rl in (150, 250)]
        doc["gpu"] = dict(rows=rows, note="one MI355X, pair records, chunk_tasks = 0; the C calls alone; alternating repetitions")
    else:
        oracle = graft.load_oracle()
        rows = [cpu_row(host, oracle, rl, a.reads, a.reps) for rl in (150, 250)]
        doc["cpu"] = dict(rows=rows, note="one thread of the CPU the tool ran on; median [min - max]; synthetic chains (tests/_chain2aln_ref.py)")
        doc.setdefault("gpu", "not measured")
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
