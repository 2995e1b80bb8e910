#!/usr/bin/env python3
"""What the device replay of mem_chain2aln's seed loop costs against the host replay (needs a GPU; one process).

Blocks: the 150-base and 250-base blocks of tools/chain2aln_rate.py (--reads reads of tests/_chain2aln_ref.py each), and one block
of at least --big seeds made of copies of the 150-base block (the read indices shifted, the reads uploaded as often): the small
blocks leave the GPU idle either way.

Per block, --reps alternating repetitions, median [min - max]:
  job        bsw_chain2aln_reads_start .. bsw_chain2aln_finish with the switch off on a context with pack_threads 8 and one with
             pack_threads 1 (the parent's code path), and with the switch on
  replay     bsw_chain2aln_replay on one thread against bsw_chain2aln_replay_batch, on the pair records of the block
  caller CPU the calling thread's own clock around the job, and bsw_host_stats' slot and helper CPU time, per million seeds
  bytes      H2D and D2H bytes per seed of the device replay, reads_host

    python3 tools/c2a_device_rate.py [--reads 4000] [--big 1000000] [--reps 7] [--out profiles/c2a_device_rate.json]
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


def spread(ts, n, unit=1e3, name="ms"):
    ts = sorted(ts)
    return {"median_" + name: round(ts[len(ts) // 2] * unit, 4), "min_" + name: round(ts[0] * unit, 4), "max_" + name: round(ts[-1] * unit, 4),
            "median_seeds_per_s": round(n / ts[len(ts) // 2], 1), "reps": len(ts)}


def tiled(host, wl, ch, sd, lens, copies):
    """`copies` copies of a block laid end to end: read and seed indices shifted"""
    if copies == 1:
        return wl["reads"], ch, sd, lens
    chs, sds = [], []
    for k in range(copies):
        c = ch.copy()
        c["read"] += k * len(lens)
        c["first_seed"] += k * len(sd)
        chs.append(c)
        sds.append(sd)
    return list(wl["reads"]) * copies, np.concatenate(chs), np.concatenate(sds), np.tile(lens, copies)


def block(host, name, read_len, n_reads, copies, reps):
    wl = R.make_workload(n_reads, seed=100 + read_len, len_lo=read_len, len_hi=read_len)
    p = host.default_params()
    ch, sd, lens = R.arrays(host, wl)
    reads, ch, sd, lens = tiled(host, wl, ch, sd, lens, copies)
    n = len(sd)
    L = host.lib()
    rdt, _ = host.chain2aln_plan(p, wl["l_pac"], ch, sd, lens)
    regs, ext, start = np.zeros(n, dtype=host.CREG), np.zeros(n, dtype=np.uint8), np.zeros(len(lens) + 1, dtype=np.uint64)
    regs2, ext2, start2 = regs.copy(), ext.copy(), start.copy()
    nr, nr2 = C.c_size_t(0), C.c_size_t(0)
    dst = np.zeros(1, dtype=host.C2A_DEV_STATS)
    row = dict(block=name, read_len=read_len, reads=len(lens), chains=len(ch), seeds=n)
    ctxs = {k: host.BswContext(device=0, result_format=host.RESULT_PAIR, pack_threads=t) for k, t in (("off_pack8", 8), ("off_pack1", 1), ("on", 8))}
    try:
        refs = {k: c.ref_upload(wl["pac"], wl["l_pac"]) for k, c in ctxs.items()}
        rds = {k: c.reads_upload(reads) for k, c in ctxs.items()}

        def job(k):
            c = ctxs[k]
            host.set_c2a_device(1 if k == "on" else 0)
            h = C.c_void_p()
            t0, c0 = time.perf_counter(), time.thread_time()
            assert L.bsw_chain2aln_reads_start(c.handle, p.ctypes.data, None, refs[k], rds[k], ch.ctypes.data, len(ch), sd.ctypes.data, n, C.byref(h)) == 0
            assert L.bsw_chain2aln_finish(h, regs.ctypes.data, C.byref(nr), ext.ctypes.data, start.ctypes.data, None) == 0
            return time.perf_counter() - t0, time.thread_time() - c0

        # the records of the block once, for the replay alone
        c = ctxs["on"]
        arena = host.HostArena(n * host.PAIR.itemsize + 64)
        out = arena.view(host.PAIR, n)
        t = C.c_uint64(0)
        assert L.bsw_submit_reads_t(c.handle, p.ctypes.data, refs["on"], rds["on"], rdt.ctypes.data, n, out.ctypes.data, C.byref(t)) == 0
        assert L.bsw_wait_ticket(c.handle, t) == 0

        def replay_host():
            t0 = time.perf_counter()
            assert L.bsw_chain2aln_replay(p.ctypes.data, None, ch.ctypes.data, len(ch), sd.ctypes.data, n, lens.ctypes.data, len(lens), out.ctypes.data,
                                          host.RESULT_PAIR, regs.ctypes.data, C.byref(nr), ext.ctypes.data, start.ctypes.data) == 0
            return time.perf_counter() - t0

        def replay_dev():
            t0 = time.perf_counter()
            assert L.bsw_chain2aln_replay_batch(c.handle, p.ctypes.data, None, ch.ctypes.data, len(ch), sd.ctypes.data, n, lens.ctypes.data, len(lens),
                                                out.ctypes.data, host.RESULT_PAIR, regs2.ctypes.data, C.byref(nr2), ext2.ctypes.data, start2.ctypes.data,
                                                dst.ctypes.data) == 0
            return time.perf_counter() - t0

        replay_host()
        replay_dev()
        assert nr.value == nr2.value and regs[:nr.value].tobytes() == regs2[:nr2.value].tobytes() and ext.tobytes() == ext2.tobytes() and start.tobytes() == start2.tobytes()
        row["regions"] = int(nr.value)
        row["device_replay"] = dict(h2d_bytes_per_seed=round(int(dst["h2d_bytes"][0]) / n, 2), d2h_bytes_per_seed=round(int(dst["d2h_bytes"][0]) / n, 2),
                                    reads_host=int(dst["reads_host"][0]), reads_gpu=int(dst["reads_gpu"][0]), chunks=int(dst["chunks"][0]))
        th, td = [], []
        for _ in range(reps):
            th.append(replay_host())
            td.append(replay_dev())
        row["replay_alone"] = dict(host_one_thread=spread(th, n), device_batch=spread(td, n))
        del out
        arena.free()

        for k in ctxs:                               # warm-up: staging, the pipeline's threads
            job(k)
        wall = {k: [] for k in ctxs}
        cpu = {k: [] for k in ctxs}
        side = {}
        for k in ctxs:
            side[k] = ctxs[k].host_stats()
        for _ in range(reps):
            for k in ctxs:
                w, u = job(k)
                wall[k].append(w)
                cpu[k].append(u)
        jobs = {}
        for k in ctxs:
            s1 = ctxs[k].host_stats()
            jobs[k] = dict(start_to_finish=spread(wall[k], n),
                           caller_thread_cpu_ms_per_million_seeds=spread(cpu[k], n, unit=1e3 * 1e6 / n, name="ms"),
                           slot_cpu_ms_per_million_seeds=round((s1["slot_cpu_ns"] - side[k]["slot_cpu_ns"]) / reps / n, 4),
                           helper_cpu_ms_per_million_seeds=round((s1["helper_cpu_ns"] - side[k]["helper_cpu_ns"]) / reps / n, 4))
        row["job"] = jobs
    finally:
        host.set_c2a_device(0)
        for k, c in ctxs.items():
            c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--big", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = graft.load_package().host
    host.c2a_device_load()
    rows = [block(host, "150", 150, a.reads, 1, a.reps), block(host, "250", 250, a.reads, 1, a.reps)]
    copies = -(-a.big // rows[0]["seeds"])
    rows.append(block(host, "150 x %d" % copies, 150, a.reads, copies, a.reps))
    for r in rows:
        print(json.dumps(r), flush=True)
    doc = dict(rows=rows, note="one MI355X, pair records, chunk_tasks = 0; the C calls alone; alternating repetitions; median [min - max]. "
                               "On several GPUs: not measured.")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
