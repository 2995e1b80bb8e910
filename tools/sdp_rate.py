#!/usr/bin/env python3
"""What bsw_sdp costs: the speculation (pairs sent to the GPU over the alignments bwa runs), the host side (the engine alone), and
with --gpu the job against the bare patch ticket on the job's own round-1 tasks.

Two workloads, both synthetic (what share of pairs a merge makes stale is a property of the regions; real ones will differ):
  sdp_ref   the regions of tests/_sdp_ref.py scaled to --reads reads: 1 - 4 colinear segments per read and the hand-made cases
  chained   the chains of tests/_chain2aln_ref.py at 150 bases (the block of tools/chain2aln_rate.py) through mem_chain2aln: the
            regions bsw_chain2aln leaves, through bsw_sdp_from_cregs

  speculation   tasks sent in round 1 and in all rounds over the alignments bwa runs (the sequential restatement's count), and
                the histogram of rounds per read
  host cost     the engine alone with every result precomputed: open, needs / feed until nothing is needed, collect, close; one
                thread, ns per input region, median [min - max] of --reps repetitions
  --gpu         bsw_sdp_reads_start + bsw_sdp_finish against bsw_patch_reads_submit_t + bsw_wait_ticket on the job's round-1
                tasks (that baseline runs none of the job's code), alternating repetitions

    python3 tools/sdp_rate.py [--reads 4080] [--reps 7] [--gpu] [--out profiles/sdp_rate.json]
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
import _sdp_ref as S  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def chained_cpu(host, oracle, p, n_reads):
    """the regions mem_chain2aln leaves of the block of tools/chain2aln_rate.py (150 bases), the extensions from the CPU oracle"""
    wl = R.make_workload(n_reads, seed=250, len_lo=150, len_hi=150)
    ch, sd, lens = R.arrays(host, wl)
    rdt, _ = host.chain2aln_plan(p, wl["l_pac"], ch, sd, lens)
    items = [(int(t["read"]), int(t["seed"]["rbeg"]), int(t["seed"]["qbeg"]), int(t["seed"]["len"]), int(t["rmax0"]), int(t["rmax1"]), k) for k, t in enumerate(rdt)]
    tasks, keep = R.build_tasks(host, R.pen_of(p), wl["reads"], wl["both"], items)
    cregs, _, start = host.chain2aln_replay(p, ch, sd, lens, oracle.pair_batch(p, tasks, nthreads=8))
    return wl, host.sdp_from_cregs(cregs), start, lens


def with_regs(wl, sregs, start):
    wl = dict(wl)
    wl["regs"] = [[{f: int(sregs[k][f]) for f in S.FIELDS[:-1]} for k in range(int(start[r]), int(start[r + 1]))] for r in range(len(start) - 1)]
    return wl


def cpu_row(host, oracle, p, name, wl, sregs, start, lens, reps):
    patcher = S.Patcher(host, oracle, p, wl)
    want, want_start, cnt, rounds = S.sdp(wl, patcher)
    L = host.lib()
    n = len(sregs)
    # one run with the oracle answering, to learn every round's results
    answers = []
    with host.SdpEngine(p, wl["l_pac"], sregs, start, lens) as e:
        while len(t := e.needs()):
            res = np.zeros(len(t), dtype=host.PRESULT)
            for k, x in enumerate(t):
                a, b = ({f: int(x[nm][f]) for f in S.PREG} for nm in ("a", "b"))
                r = patcher(int(x["read"]), a, b)
                res[k] = (r["score"], r["w"], r["gscore"], r["status"])
            e.feed(res)
            answers.append(res)
        out, ostart, st = e.collect()
    assert S.same_regions(out, want) is None and S.same_stats(st, cnt, len(lens), n, len(want)) is None
    outb, startb, nout = np.zeros(max(n, 1), dtype=host.SREG), np.zeros(len(lens) + 1, dtype=np.uint64), C.c_size_t(0)

    def engine():
        h, t, k = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        assert L.bsw_sdp_open(p.ctypes.data, None, wl["l_pac"], sregs.ctypes.data, n, start.ctypes.data, lens.ctypes.data, len(lens), C.byref(h), None, 0) == 0
        for res in answers:
            assert L.bsw_sdp_needs(h, C.byref(t), C.byref(k)) == 0 and k.value == len(res)
            assert L.bsw_sdp_feed(h, res.ctypes.data, len(res)) == 0
        assert L.bsw_sdp_needs(h, C.byref(t), C.byref(k)) == 0 and k.value == 0
        assert L.bsw_sdp_collect(h, outb.ctypes.data, C.byref(nout), startb.ctypes.data, None) == 0
        L.bsw_sdp_close(h)
    engine()
    ts = sorted(timed(engine) for _ in range(reps))
    return dict(workload=name, reads=len(lens), regions_in=n, regions_out=len(want), merges=cnt["merges"], kills_p=cnt["kills_p"], kills_q=cnt["kills_q"],
                dups=cnt["dups"], alignments_bwa=cnt["alns"], tasks_round1=cnt["tasks_first"], tasks_total=cnt["tasks"],
                round1_over_bwa=round(cnt["tasks_first"] / max(cnt["alns"], 1), 3), total_over_bwa=round(cnt["tasks"] / max(cnt["alns"], 1), 3),
                rounds=cnt["rounds"], reads_by_rounds={str(k): rounds.count(k) for k in range(max(rounds) + 1)},
                engine=dict(median_ns_per_region=round(ts[len(ts) // 2] / n * 1e9, 2), min_ns_per_region=round(ts[0] / n * 1e9, 2),
                            max_ns_per_region=round(ts[-1] / n * 1e9, 2), reps=len(ts)))


def gpu_row(host, c, ref, p, name, wl, sregs, start, lens, reps):
    L = host.lib()
    n = len(sregs)
    with host.SdpEngine(p, wl["l_pac"], sregs, start, lens) as e:
        first = e.needs()
    rd = c.reads_upload(wl["reads"])
    arena = host.HostArena(len(first) * (host.RD_PTASK.itemsize + host.PRESULT.itemsize) + 128)
    tasks = arena.view(host.RD_PTASK, len(first))
    tasks[:] = first
    res = arena.view(host.PRESULT, len(first), offset=(len(first) * host.RD_PTASK.itemsize + 63) & ~63)
    out, ostart, nout, st = np.zeros(max(n, 1), dtype=host.SREG), np.zeros(len(lens) + 1, dtype=np.uint64), C.c_size_t(0), np.zeros(1, dtype=host.SDP_STATS)
    try:
        def job():
            h = C.c_void_p()
            assert L.bsw_sdp_reads_start(c.handle, p.ctypes.data, None, ref, rd, sregs.ctypes.data, n, start.ctypes.data, C.byref(h)) == 0
            assert L.bsw_sdp_finish(h, out.ctypes.data, C.byref(nout), ostart.ctypes.data, st.ctypes.data) == 0

        def bare():
            t = C.c_uint64(0)
            assert L.bsw_patch_reads_submit_t(c.handle, p.ctypes.data, ref, rd, tasks.ctypes.data, len(first), res.ctypes.data, C.byref(t)) == 0
            assert L.bsw_wait_ticket(c.handle, t) == 0
        job()
        bare()
        tj, tb = [], []
        for _ in range(reps):
            tj.append(timed(job))
            tb.append(timed(bare))
    finally:
        del tasks, res
        arena.free()
        c.reads_free(rd)

    def spread(ts):
        ts = sorted(ts)
        return dict(median_s=round(ts[len(ts) // 2], 6), min_s=round(ts[0], 6), max_s=round(ts[-1], 6), reps=len(ts))
    sj, sb = spread(tj), spread(tb)
    return dict(workload=name, reads=len(lens), regions_in=n, regions_out=int(nout.value), rounds=int(st["rounds"][0]), tasks_round1=len(first),
                tasks_total=int(st["tasks"][0]), job_start_to_finish=sj, bare_round1_patch_ticket=sb,
                job_over_bare=round(sj["median_s"] / sb["median_s"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = graft.load_package().host
    p = host.default_params()
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    wl_a = S.make_workload(a.reads)
    sregs_a, start_a, lens_a = S.arrays(host, wl_a)
    if a.gpu:
        rows = []
        with host.BswContext(device=0) as c:
            ref = c.ref_upload(wl_a["pac"], wl_a["l_pac"])
            try:
                rows.append(gpu_row(host, c, ref, p, "sdp_ref", wl_a, sregs_a, start_a, lens_a, a.reps))
                wl_b = R.make_workload(a.reads, seed=250, len_lo=150, len_hi=150)
                ch, sd, lens_b = R.arrays(host, wl_b)
                rd = c.reads_upload(wl_b["reads"])
                cregs, _, start_b, _ = c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()
                c.reads_free(rd)
                rows.append(gpu_row(host, c, ref, p, "chained", wl_b, host.sdp_from_cregs(cregs), start_b, lens_b, a.reps))
            finally:
                c.ref_free(ref)
        doc["gpu"] = dict(rows=rows, several_gpus="not measured",
                          note="one MI355X; the C calls alone; alternating repetitions; the bare ticket is round 1's tasks only")
    else:
        oracle = graft.load_oracle()
        rows = [cpu_row(host, oracle, p, "sdp_ref", wl_a, sregs_a, start_a, lens_a, a.reps)]
        wl_b, sregs_b, start_b, lens_b = chained_cpu(host, oracle, p, a.reads)
        rows.append(cpu_row(host, oracle, p, "chained", with_regs(wl_b, sregs_b, start_b), sregs_b, start_b, lens_b, a.reps))
        doc["cpu"] = dict(rows=rows, note="one thread of the CPU the tool ran on; median [min - max]; synthetic regions")
        doc.setdefault("gpu", "not measured")
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
