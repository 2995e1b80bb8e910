#!/usr/bin/env python3
"""What the upload encodings of a read block (bsw_reads_upload_start_enc: codes, FASTQ letters, 4-bit words) change, on one GPU.

The block is tools/reads_async_rate.py's (131 072 extension seeds, 65 536 rescue windows, 65 536 CIGAR tasks over 262 144 reads of
150 bases); for the uploads its reads lie once more back to back in ONE array per encoding: 150 bytes per read as codes and as
letters, 10 words per read as 4-bit words.  One process, the rows alternating, --reps times each (at least seven), median
[min - max], with that array in registered memory and again in pageable memory:

  pointer          the three tickets, pointer forms (the baseline)
  <enc>_upload     start + wait alone
  <enc>_block      start + the three _reads_ tickets at once + collect + free
  h2d_bytes_per_read of each encoding, counted by bsw_host_stats over one upload

No threshold: the rows say whether letters or words go up faster than codes, whichever way it falls.  --codes-only uses
bsw_reads_upload_start alone, so that the same rows can be taken on a build from before the encodings (--tree PATH: the checkout
whose build is measured); --merge-parent FILE puts such a run's rows beside this build's and says whether the codes rows of this
build lie inside the parent's own spread.  Several GPUs: not measured (one GPU visible).

    python3 tools/reads_enc_rate.py [--reps 7] [--out profiles/reads_enc_rate.json]
    python3 tools/reads_enc_rate.py --codes-only --tree ../parent --out parent.json
    python3 tools/reads_enc_rate.py --merge-parent parent.json [--out profiles/reads_enc_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if "--tree" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402
import f4_stream_rate as F  # noqa: E402
import reads_rate as RR  # noqa: E402

CODES, ASCII, PACKED = 0, 1, 2
NAMES = {CODES: "codes", ASCII: "letters", PACKED: "words"}
RL = RR.RL


class Block(RR.Block):
    """RR.Block with the reads once more in one array per encoding: src[enc] = (pointer table, array kept alive)"""

    def forms(self, host, registered, encs):
        n = len(self.ptrs)
        codes = np.frombuffer(b"".join(C.string_at(int(p), RL) for p in self.ptrs), dtype=np.uint8).reshape(n, RL)
        made = {CODES: codes}
        if ASCII in encs:
            made[ASCII] = np.frombuffer(b"ACGTN", dtype=np.uint8)[np.minimum(codes, 4)]
        if PACKED in encs:
            nw = (RL + 15) // 16
            nib = np.zeros((n, nw * 16), dtype=np.uint64)
            nib[:, :RL] = np.minimum(codes, 4)
            made[PACKED] = (nib.reshape(n, nw, 16) << (4 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint64)
        self.src, self.keep = {}, []
        for enc in encs:
            a = np.ascontiguousarray(made[enc])
            if registered:
                ar = host.HostArena(a.nbytes + 64)
                ar.u8[:a.nbytes] = a.reshape(-1).view(np.uint8)
                base, keep = ar.ptr, ar
            else:
                base, keep = a.ctypes.data, a
            self.keep.append(keep)
            self.src[enc] = (np.uint64(base) + np.arange(n, dtype=np.uint64) * np.uint64(a.nbytes // n)).astype(np.uint64)

    def release(self):
        for k in self.keep:
            if hasattr(k, "free"):
                k.free()
        self.keep = []

    def start(self, enc, old_call):
        h = C.c_void_p()
        p = self.src[enc]
        if old_call:
            self.chk(self.L.bsw_reads_upload_start(self.ctx.handle, p.ctypes.data, self.lens.ctypes.data, len(p), C.byref(h)), "start")
        else:
            self.chk(self.L.bsw_reads_upload_start_enc(self.ctx.handle, p.ctypes.data, self.lens.ctypes.data, len(p), enc, C.byref(h)), "start_enc")
        return h

    def free_h(self, h):
        self.chk(self.L.bsw_reads_wait(self.ctx.handle, h), "reads_wait")
        self.chk(self.L.bsw_reads_free(self.ctx.handle, h), "free")

    def tickets(self, k):
        self.ext(k); self.rescue(k); self.cigar(k)


def rows(b, reps, encs, old_call):
    def pointer():
        b.tickets(0); b.wait()

    def upload(enc):
        b.free_h(b.start(enc, old_call))

    def block(enc):
        b.rd = b.start(enc, old_call); b.tickets(1); b.wait(); b.free_h(b.rd); b.rd = None
    out, n = {}, len(b.ptrs)
    pointer()
    for enc in encs:                                          # warm-up, parity and the counted bytes
        block(enc)
        assert b.equal(), "the _reads_ tickets behind an upload of %s differ from the pointer forms" % NAMES[enc]
        h0 = b.ctx.host_stats()["h2d_bytes"]
        upload(enc)
        out["h2d_bytes_per_read_" + NAMES[enc]] = round((b.ctx.host_stats()["h2d_bytes"] - h0) / n, 3)
    t = {"pointer": []}
    for enc in encs:
        t[NAMES[enc] + "_upload"], t[NAMES[enc] + "_block"] = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); pointer(); t["pointer"].append(time.perf_counter() - t0)
        for enc in encs:
            t0 = time.perf_counter(); upload(enc); t[NAMES[enc] + "_upload"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); block(enc); t[NAMES[enc] + "_block"].append(time.perf_counter() - t0)
    out.update({k: RR.summarise(v) for k, v in t.items()})
    for enc in encs[1:]:
        for row in ("_upload", "_block"):
            a, c = out[NAMES[enc] + row], out["codes" + row]
            out[NAMES[enc] + row + "_faster_than_codes_beyond_both_ranges"] = bool(a["max_s"] < c["min_s"])
            out[NAMES[enc] + row + "_over_codes_median"] = round(a["median_s"] / c["median_s"], 4)
    out["bit_equal"] = b.equal()
    return out


def merge_parent(path, parent_path):
    d, p = json.load(open(path)), json.load(open(parent_path))
    d["parent_build_codes_rows"] = {k: p[k] for k in ("registered_memory", "unregistered_memory")}
    verdict = {}
    for mem in ("registered_memory", "unregistered_memory"):
        for row in ("codes_upload", "codes_block", "pointer"):
            mine, theirs = d[mem][row], p[mem][row]
            inside = theirs["min_s"] <= mine["median_s"] <= theirs["max_s"]
            off = 0.0 if inside else (mine["median_s"] - theirs["max_s"] if mine["median_s"] > theirs["max_s"] else mine["median_s"] - theirs["min_s"])
            verdict[mem + "." + row] = {"this_median_s": mine["median_s"], "parent_min_s": theirs["min_s"], "parent_median_s": theirs["median_s"],
                                        "parent_max_s": theirs["max_s"], "inside_parent_spread": bool(inside), "outside_by_s": round(off, 5)}
    d["codes_rows_against_parent_build"] = verdict
    with open(path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "reads_enc_rate.json"))
    ap.add_argument("--tree", default=None, help="the checkout whose build is measured (default: this one)")
    ap.add_argument("--codes-only", action="store_true", help="the codes rows through bsw_reads_upload_start (any build)")
    ap.add_argument("--merge-parent", metavar="FILE")
    a = ap.parse_args()
    if a.merge_parent:
        merge_parent(a.out, a.merge_parent)
        return
    assert a.reps >= 7, "at least seven repetitions per row"
    encs = [CODES] if a.codes_only else [CODES, ASCII, PACKED]
    host = graft.load_package().host
    pac, fwd, rt, arena_e = F.workloads(host)
    out = {"tool": "tools/reads_enc_rate.py", "reps": a.reps, "cards_visible": int(host.lib().bsw_device_count()),
           "codes_through": "bsw_reads_upload_start" if a.codes_only else "bsw_reads_upload_start_enc",
           "several_devices": "not measured: one GPU visible",
           "note": "C calls alone, one process, the rows alternate; reads of 150 bases back to back in one array per encoding; outputs in pageable arrays"}
    with host.BswContext(devices=[0]) as ctx:
        ref = ctx.ref_upload(pac, F.L_PAC)
        mt, a1 = F.rescue_tasks(host, fwd, F.N_READS, 9)
        ct, a2 = F.cigar_tasks(host, fwd, F.N_CIGAR, 8)
        b = Block(host, ctx, ref, rt, mt, ct, (arena_e, a1, a2))
        out["reads"] = len(b.ptrs)
        for registered, name in ((True, "registered_memory"), (False, "unregistered_memory")):
            b.forms(host, registered, encs)
            out[name] = rows(b, a.reps, encs, a.codes_only)
            print(name, json.dumps(out[name]), flush=True)
            b.release()
        ctx.ref_free(ref)
        a1.free(); a2.free()
    arena_e.free()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
