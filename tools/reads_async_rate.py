#!/usr/bin/env python3
"""What the asynchronous read-block upload (bsw_reads_upload_start) changes for a block, on one GPU.

The block is tools/reads_rate.py's (131 072 extension seeds, 65 536 rescue windows, 65 536 CIGAR tasks over 262 144 reads of 150
bases).  One process, the forms alternating, --reps times each (at least seven), median [min - max]:

  a  the three tickets, pointer forms
  b  bsw_reads_upload + the three _reads_ tickets + free                      (the parent's form)
  c  bsw_reads_upload_start + the three _reads_ tickets at once + collect + free
  d  a run of 8 blocks, block k+1's start issued beside block k's tickets, per block; against the same 8 blocks through (a)

The yardsticks are a and b.  The feature meets its purpose if c is not slower than a by more than a's own spread (max - min).
The same rows again with the reads in UNREGISTERED memory (copies of the arenas in pageable arrays): the pointer forms then gather
on the host, and so do the upload's pieces.  `sweep`: row c with BSW_READS_UP_BYTES over powers of two (the library reads the
variable at every start).  Several GPUs: not measured (one GPU visible).

    python3 tools/reads_async_rate.py [--reps 7] [--out profiles/reads_async_rate.json] [--no-sweep] [--only-c N]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402
import f4_stream_rate as F  # noqa: E402
import reads_rate as RR  # noqa: E402


class Block(RR.Block):
    def start(self):
        h = C.c_void_p()
        self.chk(self.L.bsw_reads_upload_start(self.ctx.handle, self.ptrs.ctypes.data, self.lens.ctypes.data, len(self.ptrs), C.byref(h)), "start")
        return h

    def free_h(self, h):
        self.chk(self.L.bsw_reads_wait(self.ctx.handle, h), "reads_wait")
        self.chk(self.L.bsw_reads_free(self.ctx.handle, h), "free")

    def tickets(self, k):
        self.ext(k); self.rescue(k); self.cigar(k)


def rows(b, reps):
    def a():
        b.tickets(0); b.wait()

    def bb():
        b.upload(); b.tickets(1); b.wait(); b.free()

    def c():
        b.rd = b.start(); b.tickets(1); b.wait(); b.free_h(b.rd); b.rd = None

    def d_async():
        nxt = b.start()
        for k in range(8):
            b.rd = nxt
            b.tickets(1)
            nxt = b.start() if k < 7 else None
            b.wait()
            b.free_h(b.rd)
        b.rd = None

    def d_ptr():
        for _ in range(8):
            a()
    a(); bb(); c()
    assert b.equal(), "the _reads_ tickets behind an asynchronous upload differ from the pointer forms"
    t = {k: [] for k in "abc"}
    td, tdp = [], []
    for _ in range(reps):
        for name, fn in (("a", a), ("b", bb), ("c", c)):
            t0 = time.perf_counter(); fn(); t[name].append(time.perf_counter() - t0)
        t0 = time.perf_counter(); d_ptr(); tdp.append((time.perf_counter() - t0) / 8)
        t0 = time.perf_counter(); d_async(); td.append((time.perf_counter() - t0) / 8)
    s = {k: RR.summarise(v) for k, v in t.items()}
    spread = s["a"]["max_s"] - s["a"]["min_s"]
    return {"a_pointer_forms": s["a"], "b_upload_reads_forms_free": s["b"], "c_start_reads_forms_collect_free": s["c"],
            "d_8_blocks_pipelined_per_block": RR.summarise(td), "d_8_blocks_pointer_forms_per_block": RR.summarise(tdp),
            "a_spread_s": round(spread, 5), "c_minus_a_median_s": round(s["c"]["median_s"] - s["a"]["median_s"], 5),
            "purpose_met_c_not_slower_than_a_by_more_than_a_spread": bool(s["c"]["median_s"] - s["a"]["median_s"] <= spread),
            "bit_equal": b.equal()}


def sweep(b, reps):
    out = {}
    for sh in range(16, 26):
        os.environ["BSW_READS_UP_BYTES"] = str(1 << sh)
        ts = []
        b.rd = b.start(); b.tickets(1); b.wait(); b.free_h(b.rd)
        for _ in range(reps):
            t0 = time.perf_counter()
            b.rd = b.start(); b.tickets(1); b.wait(); b.free_h(b.rd)
            ts.append(time.perf_counter() - t0)
        out[str(1 << sh)] = RR.summarise(ts)
        b.rd = None
    del os.environ["BSW_READS_UP_BYTES"]
    return out


def pageable(tasks, field, arena, keep):
    """the same task records with their sequences in a pageable copy of the arena"""
    copy = np.array(arena.u8[:arena.nbytes])
    keep.append(copy)
    t = tasks.copy()
    t[field] = t[field] - np.uint64(arena.ptr) + np.uint64(copy.ctypes.data)
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_async_rate.json"))
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--only-c", type=int, default=0, help="N runs of row c and nothing else (for a kernel trace)")
    a = ap.parse_args()
    host = graft.load_package().host
    pac, fwd, rt, arena_e = F.workloads(host)
    out = {"tool": "tools/reads_async_rate.py", "reps": a.reps, "cards_visible": int(host.lib().bsw_device_count()),
           "several_devices": "not measured: one GPU visible",
           "note": "C calls alone, one process, the forms alternate; reads of 150 bases; outputs in pageable arrays"}
    with host.BswContext(devices=[0]) as ctx:
        ref = ctx.ref_upload(pac, F.L_PAC)
        mt, a1 = F.rescue_tasks(host, fwd, F.N_READS, 9)
        ct, a2 = F.cigar_tasks(host, fwd, F.N_CIGAR, 8)
        b = Block(host, ctx, ref, rt, mt, ct, (arena_e, a1, a2))
        if a.only_c:
            for _ in range(a.only_c):
                b.rd = b.start(); b.tickets(1); b.wait(); b.free_h(b.rd)
            print("ran row c %d times" % a.only_c)
            return
        assert a.reps >= 7, "at least seven repetitions per form"
        info_rd = b.start()
        out["block"] = dict(ctx.reads_info(info_rd))
        b.free_h(info_rd)
        out["registered_memory"] = rows(b, a.reps)
        print(json.dumps(out["registered_memory"]), flush=True)
        if not a.no_sweep:
            out["piece_size_sweep_row_c"] = sweep(b, a.reps)
            print(json.dumps(out["piece_size_sweep_row_c"]), flush=True)
        keep = []
        b2 = Block(host, ctx, ref, pageable(rt, "query", arena_e, keep), pageable(mt, "mate", a1, keep), pageable(ct, "query", a2, keep), ())
        out["unregistered_memory"] = rows(b2, a.reps)
        print(json.dumps(out["unregistered_memory"]), flush=True)
        ctx.ref_free(ref)
        a1.free(); a2.free()
    arena_e.free()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
