#!/usr/bin/env python3
"""What a resident read block (bsw_reads_upload + the three *_reads_* submits) changes against the pointer forms, on one GPU.

The block is tools/f4_stream_rate.py's: 131 072 extension seeds, 65 536 rescue windows of 150 x 550 and 65 536 CIGAR tasks, all
from reads of 150 bases in registered memory.  Its generators make a sequence per task, so the resident block holds 262 144
reads (39 M bases) where a real block would hold the 65 536 reads its tasks share: the upload measured here is four times a real
one.

  per_stage   each stage alone, pointer form and _reads_ form: H2D bytes per task and slot-thread CPU ns per task from
              bsw_host_stats (counted, not timed: they must equal tests/test_reads_double_cpu.py's 76 / 112 / 144), and the
              upload's bytes and time.
  block       the three tickets in flight together: pointer forms against upload + _reads_ forms + free, alternated in one
              process, --reps times each (at least five); median and range of both.  No ratio is fixed in advance.  A third
              series, for the decomposition only: the _reads_ tickets with the block uploaded outside the timed region.
  bench       python bench.py on the parent commit's build and on this one, alternated, merged in with --merge-bench THIS PARENT
              (two files of bench.py result lines): this build's median must lie inside the parent's own range.
Several GPUs: not measured (one GPU visible).

    python3 tools/reads_rate.py [--reps 5] [--out profiles/reads_rate.json]
    python3 tools/reads_rate.py --merge-bench this.jsonl parent.jsonl [--out profiles/reads_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402
import f4_stream_rate as F  # noqa: E402

RL = 150


def summarise(ts):
    med = statistics.median(ts)
    return {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "reps_s": [round(t, 5) for t in ts]}


class Block:
    """the pointer forms' task arrays, the same tasks by read index, and the calls"""

    def __init__(self, host, ctx, ref, rt, mt, ct, arenas):
        self.host, self.ctx, self.ref, self.L, self.p = host, ctx, ref, host.lib(), host.default_params()
        self.rt, self.mt, self.ct = rt, mt, ct
        ne, nm, nc = len(rt), len(mt), len(ct)
        # read i of the block: the extension reads, then the mates, then the CIGAR reads (each RL bases, back to back in its arena)
        self.ptrs = np.concatenate([rt["query"], mt["mate"], ct["query"]]).astype(np.uint64)
        self.lens = np.full(len(self.ptrs), RL, dtype=np.int32)
        assert (rt["l_query"] == RL).all() and (mt["l_ms"] == RL).all() and (ct["l_query"] == RL).all()
        self.rd_e = np.zeros(ne, dtype=host.RD_TASK)
        self.rd_e["read"] = np.arange(ne)
        for f in ("init_score", "seed", "rmax0", "rmax1", "tag"):
            self.rd_e[f] = rt[f]
        self.rd_m = np.zeros(nm, dtype=host.RD_MTASK)
        self.rd_m["read"] = ne + np.arange(nm)
        for f in ("is_rev", "rb", "re", "xtra", "min_score"):
            self.rd_m[f] = mt[f]
        self.rd_c = np.zeros(nc, dtype=host.RD_CTASK)
        self.rd_c["read"], self.rd_c["qb"], self.rd_c["qe"] = ne + nm + np.arange(nc), 0, RL
        for f in ("w", "rb", "re", "w_cap", "min_score", "max_tries"):
            self.rd_c[f] = ct[f]
        self.out_e = [np.zeros(ne, dtype=ctx.out_dtype) for _ in range(2)]
        self.mres = [np.zeros(nm, dtype=host.MRESULT) for _ in range(2)]
        self.cres = [np.zeros(nc, dtype=host.CRESULT) for _ in range(2)]
        self.cig = [np.zeros((nc, F.MAX_CIGAR), dtype=np.uint32) for _ in range(2)]
        self.md = [np.zeros((nc, F.MAX_MD), dtype=np.uint8) for _ in range(2)]
        self.rd = None
        self.upload_s = []

    def chk(self, rc, what):
        if rc:
            raise self.host.BswError(rc, what + ": " + self.L.bsw_last_error(self.ctx.handle).decode())

    def upload(self):
        h = C.c_void_p()
        t0 = time.perf_counter()
        self.chk(self.L.bsw_reads_upload(self.ctx.handle, self.ptrs.ctypes.data, self.lens.ctypes.data, len(self.ptrs), C.byref(h)), "upload")
        self.upload_s.append(time.perf_counter() - t0)
        self.rd = h

    def free(self):
        self.chk(self.L.bsw_reads_free(self.ctx.handle, self.rd), "free")
        self.rd = None

    # one submit of each kind and form (k: 0 = pointer form, 1 = _reads_ form); returns the ticket
    def ext(self, k):
        t = C.c_uint64(0)
        h, p, L = self.ctx.handle, self.p.ctypes.data, self.L
        if k:
            self.chk(L.bsw_submit_reads_t(h, p, self.ref, self.rd, self.rd_e.ctypes.data, len(self.rd_e), self.out_e[1].ctypes.data, C.byref(t)), "ext reads")
        else:
            self.chk(L.bsw_submit_ref_t(h, p, self.ref, self.rt.ctypes.data, len(self.rt), self.out_e[0].ctypes.data, C.byref(t)), "ext ref")
        return t.value

    def rescue(self, k):
        t = C.c_uint64(0)
        h, p, L = self.ctx.handle, self.p.ctypes.data, self.L
        if k:
            self.chk(L.bsw_matesw_reads_submit_t(h, p, self.ref, self.rd, self.rd_m.ctypes.data, len(self.rd_m), self.mres[1].ctypes.data, C.byref(t)), "rescue reads")
        else:
            self.chk(L.bsw_matesw_ref_submit_t(h, p, self.ref, self.mt.ctypes.data, len(self.mt), self.mres[0].ctypes.data, C.byref(t)), "rescue ref")
        return t.value

    def cigar(self, k):
        t = C.c_uint64(0)
        h, p, L = self.ctx.handle, self.p.ctypes.data, self.L
        if k:
            self.chk(L.bsw_cigar_reads_submit_t(h, p, self.ref, self.rd, self.rd_c.ctypes.data, len(self.rd_c), F.MAX_CIGAR, self.cig[1].ctypes.data, F.MAX_MD,
                                                self.md[1].ctypes.data, self.cres[1].ctypes.data, C.byref(t)), "cigar reads")
        else:
            self.chk(L.bsw_cigar_ref_submit_t(h, p, self.ref, self.ct.ctypes.data, len(self.ct), F.MAX_CIGAR, self.cig[0].ctypes.data, F.MAX_MD,
                                              self.md[0].ctypes.data, self.cres[0].ctypes.data, C.byref(t)), "cigar ref")
        return t.value

    def wait(self):
        self.chk(self.L.bsw_wait(self.ctx.handle), "wait")

    def equal(self):
        n = np.clip(self.cres[0]["n_cigar"], 0, F.MAX_CIGAR)
        mask = np.arange(F.MAX_CIGAR)[None, :] < n[:, None]
        m = np.clip(self.cres[0]["md_len"], 0, F.MAX_MD)
        mmask = np.arange(F.MAX_MD)[None, :] < m[:, None]
        return bool(self.out_e[0].tobytes() == self.out_e[1].tobytes() and self.mres[0].tobytes() == self.mres[1].tobytes() and
                    self.cres[0].tobytes() == self.cres[1].tobytes() and (self.cig[0][mask] == self.cig[1][mask]).all() and
                    (self.md[0][mmask] == self.md[1][mmask]).all())


def per_stage(b, reps):
    out = {}
    b.upload()
    for name, fn, n in (("extension", b.ext, len(b.rt)), ("rescue", b.rescue, len(b.mt)), ("cigar", b.cigar, len(b.ct))):
        row = {"tasks": n}
        for k, form in ((0, "pointer_form"), (1, "reads_form")):
            fn(k); b.wait()                                  # warm-up: staging of this kind and form
            s0 = b.ctx.host_stats()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter(); fn(k); b.wait(); ts.append(time.perf_counter() - t0)
            s1 = b.ctx.host_stats()
            row[form] = dict(summarise(ts), h2d_bytes_per_task=round((s1["h2d_bytes"] - s0["h2d_bytes"]) / (reps * n), 2),
                             slot_cpu_ns_per_task=round((s1["slot_cpu_ns"] - s0["slot_cpu_ns"]) / (reps * n), 1),
                             helper_cpu_ns_per_task=round((s1["helper_cpu_ns"] - s0["helper_cpu_ns"]) / (reps * n), 1),
                             chunks=(s1["chunks"] - s0["chunks"]) // reps)
        out[name] = row
    info = b.ctx.reads_info(b.rd)
    b.free()
    for _ in range(reps):
        b.upload(); b.free()
    out["upload"] = dict(summarise(b.upload_s[1:]), reads=info["n_reads"], bases=info["bases"], device_bytes=info["device_bytes"],
                         note="host packing of every read and one copy to the device; a real block of this work holds a quarter of the reads")
    return out


def block(b, reps):
    def pointer():
        b.ext(0); b.rescue(0); b.cigar(0); b.wait()

    def reads():
        b.upload(); b.ext(1); b.rescue(1); b.cigar(1); b.wait(); b.free()
    pointer(); reads()
    tp, tr, ts = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); pointer(); tp.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); reads(); tr.append(time.perf_counter() - t0)
        # for the decomposition only: the three _reads_ tickets with the block uploaded outside the timed region (what a pipeline
        # that uploads block k + 1 while block k is on the GPU sees per block, if the upload hides completely)
        b.upload()
        t0 = time.perf_counter(); b.ext(1); b.rescue(1); b.cigar(1); b.wait(); ts.append(time.perf_counter() - t0)
        b.free()
    p, r = summarise(tp), summarise(tr)
    faster = r["max_s"] < p["min_s"]
    return {"three_tickets_pointer_forms": p, "upload_plus_three_tickets_reads_forms_plus_free": r,
            "three_tickets_reads_forms_block_already_resident": summarise(ts),
            "reads_over_pointer_median": round(r["median_s"] / p["median_s"], 4),
            "reads_form_faster_beyond_the_pointer_forms_own_range": bool(faster), "bit_equal": b.equal()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_rate.json"))
    ap.add_argument("--merge-bench", nargs=2, metavar=("THIS", "PARENT"))
    a = ap.parse_args()
    if a.merge_bench:
        F.merge_bench(a.out, *a.merge_bench)
        d = json.load(open(a.out))
        bb = d["bench_py_default_run"]
        bb["this_median_inside_parent_range"] = bool(min(bb["parent"]) <= bb["this_median"] <= max(bb["parent"]))
        with open(a.out, "w") as f:
            json.dump(d, f, indent=1)
            f.write("\n")
        return
    assert a.reps >= 5, "at least five repetitions per side"
    host = graft.load_package().host
    pac, fwd, rt, arena_e = F.workloads(host)
    out = {"tool": "tools/reads_rate.py", "reps": a.reps, "l_pac": F.L_PAC, "cards_visible": int(host.lib().bsw_device_count()),
           "several_devices": "not measured: one GPU visible",
           "note": "C calls alone, one process, the two forms alternate; reads of 150 bases in registered memory, outputs in pageable arrays"}
    with host.BswContext(devices=[0]) as ctx:
        ref = ctx.ref_upload(pac, F.L_PAC)
        mt, a1 = F.rescue_tasks(host, fwd, F.N_READS, 9)
        ct, a2 = F.cigar_tasks(host, fwd, F.N_CIGAR, 8)
        b = Block(host, ctx, ref, rt, mt, ct, (arena_e, a1, a2))
        out["per_stage"] = per_stage(b, a.reps)
        print(json.dumps(out["per_stage"]), flush=True)
        out["block"] = block(b, a.reps)
        print(json.dumps(out["block"]), flush=True)
        ctx.ref_free(ref)
        a1.free(); a2.free()
    arena_e.free()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
