#!/usr/bin/env python3
"""Rates of the ticketed CIGAR and mate-rescue submits (bsw_cigar_ref_submit_t / bsw_matesw_ref_submit_t) against the synchronous
calls, and of the three stages of a read block as three tickets in flight against the serial order.

Every comparison runs in one process, the two sides alternate, each side is repeated --reps times (at least five), and the spread
of each side ((max - min) / median of its repetitions) is recorded next to its median.  A side under test is ACCEPTED when its
median is not slower than the yardstick's median by more than the yardstick's own spread.

  row 1  one device, one call: m150_w550 x 262 144 rescue tasks (tools/matesw_rate.py's shape) and q150 x 65 536 CIGAR tasks
         (tools/cigar_rate.py's, a tenth of them in mem_reg2aln's loop); ticketed submit + wait against the synchronous call.
  row 2  pipeline: one block of reads of 150 bases — 131 072 extension seeds (bsw_synth_ref_generate, as bench.py's device-reference
         leg), 65 536 rescue windows and 65 536 CIGAR tasks: two seeds, one window and one CIGAR per read pair end; three tickets
         in flight together against submit + wait followed by the two synchronous calls.
  row 3  rows 1 and 2 over 2, 4 and 8 devices when the machine shows more than one card, else a note that says so;
         devices=[0, 0] (one ordinal twice: more slots on one card) is recorded and claims nothing.
  sweep  the work target of a chunk (BSW_F4_MATESW_WORK / BSW_F4_CIGAR_WORK, read once per process: one child process per value).
  row 4  bench.py's default run on this tree and on the parent commit's, alternated: merged in with --merge-bench THIS PARENT
         (two files of bench.py result lines, one per run).

    python3 tools/f4_stream_rate.py [--reps 5] [--no-sweep] [--out profiles/f4_stream_rate.json]
    python3 tools/f4_stream_rate.py --merge-bench this.jsonl parent.jsonl [--out profiles/f4_stream_rate.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402

L_PAC = 4_000_003
N_RESCUE, N_CIGAR, N_READS = 262144, 65536, 65536
MAX_CIGAR, MAX_MD = 64 + 150 // 8, 256 + 150 * 2          # tools/cigar_rate.py's room for q150
SWEEP_MATESW = [1 << k for k in range(27, 34)]
SWEEP_CIGAR = [1 << k for k in range(24, 31)]


def unpack_pac(pac, l_pac):
    x = np.arange(l_pac, dtype=np.int64)
    return ((pac[x >> 2] >> ((~x & 3) << 1)) & 3).astype(np.uint8)


def rescue_tasks(host, fwd, n, seed):
    """tools/matesw_rate.py's m150_w550: (MTASK array, the registered arena that holds the mates)"""
    import matesw_rate as mr
    mr.L_PAC = L_PAC
    rng = np.random.default_rng(seed)
    rb, re, is_rev, mates = mr.make(rng, fwd, 150, 550, n)
    arena = host.HostArena(n * 150 + 64)
    arena.u8[:n * 150] = mates.reshape(-1)
    mt = np.zeros(n, dtype=host.MTASK)
    mt["mate"] = arena.ptr + 150 * np.arange(n, dtype=np.uint64)
    mt["l_ms"], mt["is_rev"], mt["rb"], mt["re"], mt["xtra"], mt["min_score"] = 150, is_rev, rb, re, 0x40000 | 0x80000 | 0x10000 | 19, 19
    return mt, arena


def cigar_tasks(host, fwd, n, seed, retry_frac=0.1):
    """tools/cigar_rate.py's q150 (reads of 150 bases, intervals of 150 +- 3 %, w_ = 100; a tenth with w_ = 25, w_cap = 100, a
    min_score out of reach and up to 3 tries), generated with vector operations: (CTASK array, the registered arena of the reads)"""
    import matesw_rate as mr
    mr.L_PAC = L_PAC
    rng = np.random.default_rng(seed)
    rlen = 150 + rng.integers(-4, 5, n)
    strand = np.arange(n) & 1
    rb = strand * L_PAC + rng.integers(0, L_PAC - 160, n)
    rows = mr.gather(fwd, rb.astype(np.int64), np.full(n, 160, np.int64))
    reads = rows[:, :150].copy()
    sub = rng.random((n, 150)) < 0.02
    reads[sub] = (reads[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    gap = rng.random(n) < 0.4                                # one deleted base near the middle: the tail shifts by one
    reads[gap, 70:150] = rows[gap, 71:151]
    arena = host.HostArena(n * 150 + 64)
    arena.u8[:n * 150] = reads.reshape(-1)
    retry = rng.random(n) < retry_frac
    ct = np.zeros(n, dtype=host.CTASK)
    ct["query"] = arena.ptr + 150 * np.arange(n, dtype=np.uint64)
    ct["l_query"], ct["rb"], ct["re"] = 150, rb, rb + rlen
    ct["w"] = np.where(retry, 25, 100)
    ct["w_cap"] = np.where(retry, 100, 0)
    ct["min_score"] = np.where(retry, 1 << 30, -(1 << 31))
    ct["max_tries"] = np.where(retry, 3, 1)
    return ct, arena


def summarise(ts):
    med = statistics.median(ts)
    return {"median_s": round(med, 5), "spread": round((max(ts) - min(ts)) / med, 4), "reps_s": [round(t, 5) for t in ts]}


def compare(yard, test, reps):
    """alternate the two sides; -> (yardstick summary, test summary, verdict)"""
    ty, tt = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); yard(); ty.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); test(); tt.append(time.perf_counter() - t0)
    y, t = summarise(ty), summarise(tt)
    ok = t["median_s"] <= y["median_s"] * (1.0 + y["spread"])
    return y, t, {"test_over_yardstick": round(t["median_s"] / y["median_s"], 4), "accepted": bool(ok),
                  "rule": "test median <= yardstick median x (1 + yardstick spread)"}


class Calls:
    """the C calls alone, into output arrays allocated and touched once"""

    def __init__(self, host, ctx, ref, mt, ct):
        self.host, self.ctx, self.ref, self.mt, self.ct, self.L = host, ctx, ref, mt, ct, host.lib()
        self.p = host.default_params()
        self.mres = [np.zeros(len(mt), dtype=host.MRESULT) for _ in range(2)]
        self.cres = [np.zeros(len(ct), dtype=host.CRESULT) for _ in range(2)]
        self.cig = [np.zeros((len(ct), MAX_CIGAR), dtype=np.uint32) for _ in range(2)]
        self.md = [np.zeros((len(ct), MAX_MD), dtype=np.uint8) for _ in range(2)]

    def chk(self, rc, what):
        if rc:
            raise self.host.BswError(rc, what + ": " + self.L.bsw_last_error(self.ctx.handle).decode())

    def matesw_sync(self):
        self.chk(self.L.bsw_matesw_ref_batch(self.ctx.handle, self.p.ctypes.data, self.ref, self.mt.ctypes.data, len(self.mt), self.mres[0].ctypes.data), "matesw batch")

    def matesw_submit(self, wait=True):
        import ctypes as C
        t = C.c_uint64(0)
        self.chk(self.L.bsw_matesw_ref_submit_t(self.ctx.handle, self.p.ctypes.data, self.ref, self.mt.ctypes.data, len(self.mt), self.mres[1].ctypes.data, C.byref(t)), "matesw submit")
        if wait:
            self.chk(self.L.bsw_wait_ticket(self.ctx.handle, t.value), "matesw wait")
        return t.value

    def cigar_sync(self):
        self.chk(self.L.bsw_cigar_ref_batch(self.ctx.handle, self.p.ctypes.data, self.ref, self.ct.ctypes.data, len(self.ct), MAX_CIGAR, self.cig[0].ctypes.data, MAX_MD,
                                            self.md[0].ctypes.data, self.cres[0].ctypes.data), "cigar batch")

    def cigar_submit(self, wait=True):
        import ctypes as C
        t = C.c_uint64(0)
        self.chk(self.L.bsw_cigar_ref_submit_t(self.ctx.handle, self.p.ctypes.data, self.ref, self.ct.ctypes.data, len(self.ct), MAX_CIGAR, self.cig[1].ctypes.data, MAX_MD,
                                               self.md[1].ctypes.data, self.cres[1].ctypes.data, C.byref(t)), "cigar submit")
        if wait:
            self.chk(self.L.bsw_wait_ticket(self.ctx.handle, t.value), "cigar wait")
        return t.value

    def equal(self):
        n = np.clip(self.cres[0]["n_cigar"], 0, MAX_CIGAR)
        mask = np.arange(MAX_CIGAR)[None, :] < n[:, None]
        m = np.clip(self.cres[0]["md_len"], 0, MAX_MD)
        mmask = np.arange(MAX_MD)[None, :] < m[:, None]
        return bool(self.mres[0].tobytes() == self.mres[1].tobytes() and self.cres[0].tobytes() == self.cres[1].tobytes() and
                    (self.cig[0][mask] == self.cig[1][mask]).all() and (self.md[0][mmask] == self.md[1][mmask]).all())


def row1(host, ctx, ref, mt, ct, reps):
    c = Calls(host, ctx, ref, mt, ct)
    for f in (c.matesw_sync, c.matesw_submit, c.cigar_sync, c.cigar_submit):      # warm-up: allocations on both lanes
        f()
    out = {}
    base = ctx.host_stats()["chunks"]
    y, t, v = compare(c.matesw_sync, c.matesw_submit, reps)
    chunks = (ctx.host_stats()["chunks"] - base) // reps
    out["matesw_m150_w550"] = {"tasks": len(mt), "synchronous": dict(y, tasks_per_s=round(len(mt) / y["median_s"])),
                               "submit": dict(t, tasks_per_s=round(len(mt) / t["median_s"]), chunks=int(chunks)), "verdict": v}
    base = ctx.host_stats()["chunks"]
    y, t, v = compare(c.cigar_sync, c.cigar_submit, reps)
    chunks = (ctx.host_stats()["chunks"] - base) // reps
    out["cigar_q150"] = {"tasks": len(ct), "retried": 0.1, "synchronous": dict(y, tasks_per_s=round(len(ct) / y["median_s"])),
                         "submit": dict(t, tasks_per_s=round(len(ct) / t["median_s"]), chunks=int(chunks)), "verdict": v}
    out["bit_equal"] = c.equal()
    return out


def row2(host, ctx, ref, rt, mt, ct, reps):
    c = Calls(host, ctx, ref, mt, ct)
    p = c.p
    out_e = [np.zeros(len(rt), dtype=ctx.out_dtype) for _ in range(2)]

    def serial():
        ctx.submit_ref(p, ref, rt, out=out_e[0])
        ctx.wait()
        c.matesw_sync()
        c.cigar_sync()

    def piped():
        ctx.submit_ref(p, ref, rt, out=out_e[1])
        c.matesw_submit(wait=False)
        c.cigar_submit(wait=False)
        ctx.wait()
    serial()
    piped()
    y, t, v = compare(serial, piped, reps)
    return {"reads": N_READS, "extension_seeds": len(rt), "rescue_windows": len(mt), "cigar_tasks": len(ct),
            "serial_submit_wait_then_two_batch_calls": y, "three_tickets_in_flight": t, "verdict": v,
            "bit_equal": bool(c.equal() and out_e[0].tobytes() == out_e[1].tobytes())}


def workloads(host):
    p = host.default_params()
    arena_e = host.HostArena(2 * N_READS * 150 + 64)
    pac, rt, _ = host.synth_ref_tasks(2 * N_READS, L_PAC, p, arena=arena_e.u8, seed=11, read_len=150, seed_len_min=19, seed_len_max=60,
                                      seed_at_start=0, sub_rate=0.02, indel_rate=0.004, n_rate=0.002, junk_frac=0.05)
    fwd = unpack_pac(pac, L_PAC)
    return pac, fwd, rt, arena_e


def measure_on(host, devices, pac, fwd, rt, reps):
    out = {}
    with host.BswContext(devices=devices) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        mt, a1 = rescue_tasks(host, fwd, N_RESCUE, 7)
        ct, a2 = cigar_tasks(host, fwd, N_CIGAR, 8)
        out["one_call"] = row1(host, ctx, ref, mt, ct, reps)
        mt2, a3 = rescue_tasks(host, fwd, N_READS, 9)
        out["pipeline"] = row2(host, ctx, ref, rt, mt2, ct, reps)
        ctx.ref_free(ref)
        for a in (a1, a2, a3):
            a.free()
    return out


def child_sweep(kind, reps):
    """one value of the work target (taken from the environment by the library): submit + wait, median of reps"""
    host = graft.load_package().host
    rng = np.random.default_rng(2026)
    fwd = rng.integers(0, 4, L_PAC).astype(np.uint8)
    import _gencigar_ref as gc
    pac = gc.pack_pac(fwd)
    with host.BswContext(device=0) as ctx:
        ref = ctx.ref_upload(pac, L_PAC)
        mt, a1 = rescue_tasks(host, fwd, N_RESCUE if kind == "matesw" else 1024, 7)
        ct, a2 = cigar_tasks(host, fwd, N_CIGAR if kind == "cigar" else 1024, 8)
        c = Calls(host, ctx, ref, mt, ct)
        f = c.matesw_submit if kind == "matesw" else c.cigar_submit
        f()
        base = ctx.host_stats()["chunks"]
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
        chunks = (ctx.host_stats()["chunks"] - base) // reps
        ctx.ref_free(ref)
        a1.free(); a2.free()
    n = len(mt) if kind == "matesw" else len(ct)
    print("SWEEP " + json.dumps(dict(summarise(ts), chunks=int(chunks), tasks_per_s=round(n / statistics.median(ts)))), flush=True)


def sweep(reps):
    out = {}
    for kind, var, values in (("matesw", "BSW_F4_MATESW_WORK", SWEEP_MATESW), ("cigar", "BSW_F4_CIGAR_WORK", SWEEP_CIGAR)):
        rows = []
        for v in values:
            env = dict(os.environ)
            env[var] = str(v)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-sweep", kind, "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("SWEEP ")]
            if r.returncode != 0 or not line:
                raise RuntimeError("sweep child %s=%d failed: %s" % (var, v, r.stderr[-2000:]))
            row = dict(json.loads(line[0][6:]), work_target=v, log2=int(v).bit_length() - 1)
            print(kind, json.dumps(row), flush=True)
            rows.append(row)
        out["sweep_" + kind] = {"variable": var, "shape": "m150_w550 x 262144" if kind == "matesw" else "q150 x 65536, a tenth retried",
                                "one_device_four_slots": rows}
    return out


def merge_bench(out_path, this_path, parent_path):
    def values(path):
        vals = []
        for line in open(path):
            line = line.strip()
            if line.startswith("{"):
                d = json.loads(line)
                if "value" in d:
                    vals.append({"value": d["value"], "metric": d.get("metric"), "unit": d.get("unit")})
        return vals
    d = json.load(open(out_path))
    this, parent = values(this_path), values(parent_path)
    tv, pv = [x["value"] for x in this], [x["value"] for x in parent]
    d["bench_py_default_run"] = {
        "how": "python bench.py, this tree and the parent commit's alternated, one process each",
        "metric": this[0]["metric"] if this else None, "unit": this[0]["unit"] if this else None,
        "this_tree": tv, "parent": pv,
        "this_median": statistics.median(tv), "parent_median": statistics.median(pv),
        "parent_spread": round((max(pv) - min(pv)) / statistics.median(pv), 4),
        "this_over_parent": round(statistics.median(tv) / statistics.median(pv), 4),
        "within_parent_spread": bool(statistics.median(tv) >= statistics.median(pv) - (max(pv) - min(pv)))}
    with open(out_path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f4_stream_rate.json"))
    ap.add_argument("--child-sweep", default=None, choices=["matesw", "cigar"])
    ap.add_argument("--merge-bench", nargs=2, metavar=("THIS", "PARENT"))
    a = ap.parse_args()
    if a.merge_bench:
        return merge_bench(a.out, *a.merge_bench)
    if a.child_sweep:
        return child_sweep(a.child_sweep, a.reps)
    assert a.reps >= 5, "at least five repetitions per side"
    host = graft.load_package().host
    ncards = int(host.lib().bsw_device_count())
    pac, fwd, rt, arena_e = workloads(host)
    out = {"tool": "tools/f4_stream_rate.py", "reps": a.reps, "l_pac": L_PAC, "cards_visible": ncards,
           "note": "C calls alone; the two sides of a comparison alternate in one process; spread = (max - min) / median of a side's repetitions; "
                   "reads in registered memory, outputs in pageable arrays"}
    out["one_device"] = measure_on(host, [0], pac, fwd, rt, a.reps)
    print(json.dumps(out["one_device"]), flush=True)
    if ncards > 1:
        out["several_devices"] = {}
        for g in (2, 4, 8):
            if g <= ncards:
                out["several_devices"][str(g)] = measure_on(host, list(range(g)), pac, fwd, rt, a.reps)
                print(g, json.dumps(out["several_devices"][str(g)]), flush=True)
    else:
        out["several_devices"] = "not measured: one GPU visible"
    out["devices_0_0_claims_nothing"] = measure_on(host, [0, 0], pac, fwd, rt, a.reps)
    arena_e.free()
    if not a.no_sweep:
        out.update(sweep(a.reps))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
