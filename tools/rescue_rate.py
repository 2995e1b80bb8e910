#!/usr/bin/env python3
"""What bsw_rescue costs: the speculation (windows sent to the GPU over the orientations that run in bwa's order), the host side
(the engine alone), and with --gpu the job against the bare rescue ticket on the job's own round-1 tasks.

Two blocks of the workload of tests/_rescue_ref.py, both synthetic (how often a rescue changes what a later anchor skips is a
property of the regions; real ones will differ): the test workload itself, and the same mix scaled to --pairs pairs.

  speculation   tasks sent in round 1 and in all rounds over the orientations that run (the sequential restatement's count), and
                the tasks first asked after round 1 (late)
  host cost     the engine alone with every result precomputed: open, needs / feed until nothing is needed, collect, close; one
                thread, ns per anchor and per input region, median [min - max] of --reps repetitions
  --gpu         bsw_rescue_reads_start + bsw_rescue_finish against bsw_matesw_reads_submit_t + bsw_wait_ticket on the job's round-1
                tasks (that baseline runs none of the job's code), alternating repetitions

    python3 tools/rescue_rate.py [--pairs 4080] [--reps 7] [--gpu] [--out profiles/rescue_rate.json]
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
import _rescue_ref as R  # noqa: E402
import _sdp_ref as S  # noqa: E402

HAND = 9             # the pairs make_workload builds by hand


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def blocks(pairs):
    n_long = pairs // 12
    return [("test", R.make_workload()), ("block", R.make_workload(n100=pairs - n_long - HAND, n_long=n_long))]


def spread(ts, per=1, unit="s", digits=6):
    ts = sorted(ts)
    return {"median_" + unit: round(ts[len(ts) // 2] / per, digits), "min_" + unit: round(ts[0] / per, digits), "max_" + unit: round(ts[-1] / per, digits),
            "reps": len(ts)}


def engine_args(host, wl):
    opt, contigs = R.options("fr")
    return host.rescue_opt(**opt), host.contig_table(contigs)


def cpu_row(host, oracle, p, name, wl, reps):
    regs, start, lens = S.arrays(host, wl)
    al = R.Aligner(oracle, p, wl)
    want, want_start, want_n_sw, cnt = R.rescue(wl, al)
    o, ct = engine_args(host, wl)
    L = host.lib()
    n = len(regs)
    answers = []                                     # one run with the oracle answering, to learn every round's results
    with host.RescueEngine(p, wl["l_pac"], regs, start, lens, contigs=ct, opt={k: o[k][0] for k in o.dtype.names}) as e:
        while len(t := e.needs()):
            res = R.answer(host, al, t)
            e.feed(res)
            answers.append(res)
        out, ostart, n_sw, st = e.collect()
        cap = e.out_capacity()
    assert S.same_regions(out, want) is None and list(n_sw) == want_n_sw and R.same_stats(st, cnt, n, len(want)) is None
    outb, startb, nout = np.zeros(max(cap, 1), dtype=host.SREG), np.zeros(len(lens) + 1, dtype=np.uint64), C.c_size_t(0)

    def engine():
        h, t, k = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        assert L.bsw_rescue_open(p.ctypes.data, o.ctypes.data, wl["l_pac"], ct.ctypes.data, len(ct), regs.ctypes.data, n, start.ctypes.data, lens.ctypes.data,
                                 len(lens), C.byref(h), None, 0) == 0
        for res in answers:
            assert L.bsw_rescue_needs(h, C.byref(t), C.byref(k)) == 0 and k.value == len(res)
            assert L.bsw_rescue_feed(h, res.ctypes.data, len(res)) == 0
        assert L.bsw_rescue_needs(h, C.byref(t), C.byref(k)) == 0 and k.value == 0
        assert L.bsw_rescue_collect(h, outb.ctypes.data, C.byref(nout), startb.ctypes.data, None, None) == 0
        L.bsw_rescue_close(h)
    engine()
    ts = [timed(engine) for _ in range(reps)]
    return dict(workload=name, pairs=len(lens) // 2, regions_in=n, regions_out=len(want), anchors=cnt["anchors"], pushed=cnt["pushed"],
                alignments_bwa=cnt["alns"], tasks_round1=cnt["tasks_first"], tasks_total=cnt["tasks"], late=cnt["late"], rounds=cnt["rounds"],
                round1_over_bwa=round(cnt["tasks_first"] / max(cnt["alns"], 1), 3), total_over_bwa=round(cnt["tasks"] / max(cnt["alns"], 1), 3),
                engine_ns_per_anchor=spread(ts, cnt["anchors"] * 1e-9, "ns", 2), engine_ns_per_region=spread(ts, n * 1e-9, "ns", 2))


def gpu_row(host, c, ref, p, name, wl, reps):
    L = host.lib()
    regs, start, lens = S.arrays(host, wl)
    o, ct = engine_args(host, wl)
    n = len(regs)
    with host.RescueEngine(p, wl["l_pac"], regs, start, lens, contigs=ct, opt={k: o[k][0] for k in o.dtype.names}) as e:
        first = e.needs()
        cap = e.out_capacity()
    rd = c.reads_upload(wl["reads"])
    arena = host.HostArena(len(first) * (host.RD_MTASK.itemsize + host.MRESULT.itemsize) + 128)
    tasks = arena.view(host.RD_MTASK, len(first))
    tasks[:] = first
    res = arena.view(host.MRESULT, len(first), offset=(len(first) * host.RD_MTASK.itemsize + 63) & ~63)
    out, ostart, nout = np.zeros(max(cap, 1), dtype=host.SREG), np.zeros(len(lens) + 1, dtype=np.uint64), C.c_size_t(0)
    st = np.zeros(1, dtype=host.RESCUE_STATS)
    try:
        def job():
            h = C.c_void_p()
            assert L.bsw_rescue_reads_start(c.handle, p.ctypes.data, o.ctypes.data, ref, rd, ct.ctypes.data, len(ct), regs.ctypes.data, n, start.ctypes.data,
                                            C.byref(h)) == 0
            assert L.bsw_rescue_finish(h, out.ctypes.data, len(out), C.byref(nout), ostart.ctypes.data, None, st.ctypes.data) == 0

        def bare():
            t = C.c_uint64(0)
            assert L.bsw_matesw_reads_submit_t(c.handle, p.ctypes.data, ref, rd, tasks.ctypes.data, len(first), res.ctypes.data, C.byref(t)) == 0
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
    sj, sb = spread(tj), spread(tb)
    return dict(workload=name, pairs=len(lens) // 2, regions_in=n, regions_out=int(nout.value), rounds=int(st["rounds"][0]), tasks_round1=len(first),
                tasks_total=int(st["tasks"][0]), late=int(st["late"][0]), alignments_bwa=int(st["alns_bwa"][0]), job_start_to_finish=sj,
                bare_round1_rescue_ticket=sb, job_over_bare=round(sj["median_s"] / sb["median_s"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = graft.load_package().host
    p = host.default_params()
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    work = blocks(a.pairs)
    if a.gpu:
        rows = []
        with host.BswContext(device=0) as c:
            ref = c.ref_upload(work[0][1]["pac"], work[0][1]["l_pac"])
            try:
                for name, wl in work:
                    rows.append(gpu_row(host, c, ref, p, name, wl, a.reps))
            finally:
                c.ref_free(ref)
        doc["gpu"] = dict(rows=rows, several_gpus="not measured",
                          note="one MI355X; the C calls alone; alternating repetitions; the bare ticket is round 1's tasks only")
    else:
        oracle = graft.load_oracle()
        rows = [cpu_row(host, oracle, p, name, wl, a.reps) for name, wl in work]
        doc["cpu"] = dict(rows=rows, note="one thread of the CPU the tool ran on; median [min - max]; synthetic regions")
        doc.setdefault("gpu", "not measured")
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
