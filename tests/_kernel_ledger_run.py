"""Runs one group of the kernel ledger (tests/_kernel_ledger.py) on cuda:0 and compares every result with its reference, bit for
bit.  The group's switches must already be in the environment (tests/test_gpu_kernel_ledger.py starts this under a kernel
trace, one group at a time).  Prints `case <name> seeds <n>` per case and `ok` at the end."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import _kernel_ledger as L  # noqa: E402
from test_gpu_parity import assert_same, FIELDS  # noqa: E402


def run_ext(host, orc, case):
    import _rtl_ref
    sd = L.workload(case)
    tasks, arena = host.make_tasks(sd)
    p = L.make_params(host, case)
    if case["params"].get("variant") == L.RTL:
        want = _rtl_ref.pair_batch(p, tasks)
    else:
        want = orc.pair_batch(p, tasks, nthreads=8)
    cx = dict(case["ctx"])
    entry = case["entry"]
    if entry == "wire":
        words, n = host.refbatch_encode(p, tasks)
        assert n == len(tasks)
        with host.BswContext(device=0, **cx) as c:
            out, nres = c.refbatch_run(words, variant=int(p["variant"][0]), zdrop=int(p["zdrop"][0]))
        assert nres == n
        got = host.refbatch_decode_results(out, n)
        for f in FIELDS:
            bad = np.nonzero(got[f] != want[f])[0]
            assert bad.size == 0, (case["name"], f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
        return len(tasks)
    with host.BswContext(device=0, **cx) as c:
        if entry == "extend_pairs":
            got = c.extend_pairs(p, tasks)
        elif entry == "upload_run":
            b = c.upload(p, tasks)
            c.run(b)
            c.sync()
            got = c.download(b)
            b.free()
        elif entry == "packed_registered":
            need = int(host.lib().bsw_pack_tasks_bound(tasks.ctypes.data, len(tasks)))
            ha = host.HostArena(need + 64)
            try:
                pt, words = host.pack_tasks(tasks, ha.view(np.uint64, need // 8 + 1))
                got = c.extend_pairs_packed(p, pt)
            finally:
                ha.free()
        else:
            raise ValueError(entry)
    if cx.get("result_format") == L.PAIR:
        for f in FIELDS:
            bad = np.nonzero(got[f] != want[f])[0]
            assert bad.size == 0, (case["name"], f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    else:
        assert_same(got, want, tasks)
    return len(tasks)


def run_other(host, orc, case):
    p = L.make_params(host, case)
    with host.BswContext(device=0, **case["ctx"]) as c:
        if case["entry"] == "global_batch":
            import test_gpu_global as T
            pairs, ws = L.workload(case)
            T.check(host, orc, c, p, pairs, ws, max_cigar=max(len(q) for q, t in pairs) // 2 + 96)
            return len(pairs)
        if case["entry"] == "align_batch":
            import test_gpu_align as T
            pairs, xt = L.workload(case)
            at, keep = T.make(host, pairs, xt)
            T.check(host, orc, c, p, at)
            return len(pairs)
        if case["entry"] == "cigar_ref_batch":
            import test_gpu_cigar_ref as T
            specs = L.workload(case)
            pac = L.cigar_genome()
            ref = c.ref_upload(pac, T.L_PAC)
            try:
                T.check(host, orc, c, p, (pac, ref), specs, max_cigar=1024, max_md=8192)
            finally:
                c.ref_free(ref)
            return len(specs)
        if case["entry"] == "reads_upload_async":
            raw, lens, offs = L.workload(case)
            reads = [raw[o:o + n] for o, n in zip(offs, lens)]
            rd = c.reads_upload_start(reads)
            try:
                c.reads_wait(rd)
                got = c.reads_image(rd)
            finally:
                c.reads_free(rd)
            rd = c.reads_upload(reads)
            try:
                sync = c.reads_image(rd)
            finally:
                c.reads_free(rd)
            slack = (len(got) - sum((int(n) + 15) // 16 for n in lens)) // 2
            want = L.reads_image(raw, lens, offs, slack)
            assert slack > 0 and got.tobytes() == sync.tobytes(), np.nonzero(got != sync)[0][:5]
            assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:5]
            return len(reads)
    raise ValueError(case["entry"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", required=True)
    args = ap.parse_args()
    cases = L.groups()[args.group]
    for c in cases:
        for k, v in c["env"].items():
            assert os.environ.get(k) == v, "group %s needs %s=%s in the environment" % (args.group, k, v)
    host, orc = graft.load_package().host, graft.load_oracle()
    for c in cases:
        t0 = time.time()
        ext = c["entry"] in ("extend_pairs", "upload_run", "packed_registered", "wire")
        n = run_ext(host, orc, c) if ext else run_other(host, orc, c)
        print("case %s seeds %d seconds %.1f" % (c["name"], n, time.time() - t0), flush=True)
    print("ok")


if __name__ == "__main__":
    main()
