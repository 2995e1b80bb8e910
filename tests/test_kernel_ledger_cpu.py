"""The kernel ledger (tests/_kernel_ledger.py) against the build: the kernels compiled into libbwasw_mi355.so — the .kd symbols of
its gfx950 code objects, demangled — are exactly the ledger's targets plus UNREACHED.  A new instantiation without a case fails,
and so does a case naming a kernel the build no longer has.  Every extension workload is checked on the CPU reference for the
edges it claims: a side at its class's last column, a band retry, a z-drop, Ns in queries and targets, 8-bit seeds at the
255 bound and 16-bit seeds near the 65 000 bound."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _kernel_ledger as L

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def compiled_kernels(so_path, arch="gfx950"):
    """normalised names of the kernels in the .hip_fatbin section of `so_path`, for `arch`"""
    with tempfile.TemporaryDirectory(prefix="ledger_") as tmp:
        fb = os.path.join(tmp, "fatbin")
        subprocess.check_call(["objcopy", "--dump-section", ".hip_fatbin=" + fb, so_path, os.path.join(tmp, "copy.so")])
        data = open(fb, "rb").read()
        syms = []
        at, k = data.find(BUNDLE), 0
        while at >= 0:
            n = struct.unpack_from("<Q", data, at + 24)[0]
            p = at + 32
            for _ in range(n):
                off, size, idlen = struct.unpack_from("<QQQ", data, p)
                triple = data[p + 24:p + 24 + idlen].decode()
                p += 24 + idlen
                if triple.endswith("-" + arch) and size:
                    co = os.path.join(tmp, "co%d" % k)
                    k += 1
                    with open(co, "wb") as f:
                        f.write(data[at + off:at + off + size])
                    out = subprocess.run([READELF, "--syms", "--wide", co], capture_output=True, text=True, check=True).stdout
                    syms += [ln.split()[-1][:-3] for ln in out.splitlines() if ln.split() and ln.split()[-1].endswith(".kd")]
            at = data.find(BUNDLE, at + 1)
        assert k > 0, "no %s code object in %s" % (arch, so_path)
    dm = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    return set(L.normalise(x) for x in dm if x.strip())


@pytest.fixture(scope="module")
def build_kernels(built):
    return compiled_kernels(built.lib_path())


def test_ledger_covers_the_build(build_kernels):
    ledger = L.targets()
    missing = sorted(build_kernels - ledger - set(L.UNREACHED))
    stale = sorted((ledger | set(L.UNREACHED)) - build_kernels)
    print("compiled kernels: %d, ledger targets: %d, unreached: %d" % (len(build_kernels), len(ledger), len(L.UNREACHED)))
    assert not missing, "compiled kernels without a ledger case: %s" % missing
    assert not stale, "ledger names kernels the build does not have: %s" % stale
    assert not (ledger & set(L.UNREACHED)), "a kernel both reached and UNREACHED"
    for name, why in L.UNREACHED.items():
        assert why.strip(), name


def test_cases_are_well_formed():
    names = [c["name"] for c in L.CASES]
    assert len(names) == len(set(names)), "case names must be unique"
    entries = {"extend_pairs", "upload_run", "packed_registered", "wire", "global_batch", "align_batch", "cigar_ref_batch",
               "reads_upload_async"}
    for c in L.CASES:
        assert c["targets"] and c["ref"] and callable(c["gen"]), c["name"]
        assert c["entry"] in entries, c["name"]
        assert all(k.startswith("BSW_") for k in c["env"]), c["name"]
        assert all(t == L.normalise(t) and t.startswith(L.NS) for t in c["targets"]), c["name"]


EXT_CASES = [c for c in L.CASES if c["entry"] in ("extend_pairs", "upload_run", "packed_registered", "wire")]


@pytest.mark.parametrize("case", EXT_CASES, ids=[c["name"] for c in EXT_CASES])
def test_workload_is_non_vacuous(host, oracle, case):
    import _rtl_ref
    sd = L.workload(case)
    tasks, arena = host.make_tasks(sd)
    p = L.make_params(host, case)
    ref = (lambda q: _rtl_ref.pair_batch(q, tasks)) if case["params"].get("variant") == L.RTL else \
        (lambda q: oracle.pair_batch(q, tasks, nthreads=8))
    want = ref(p)
    lq, rq = tasks["lqlen"].astype(np.int64), tasks["rqlen"].astype(np.int64)
    qm = np.maximum(lq, rq)
    a, b = int(p["mat"][0][0]), max(0, -int(p["mat"][0][1]))
    top = tasks["h0"].astype(np.int64) + (lq + rq) * a
    got = {}
    edges = case["edges"]
    if "last_col" in edges:
        for lo, hi in case["bands"]:
            got["last_col %d" % (hi + 1)] = int((qm == hi).sum())
    if "retry" in edges:
        w = int(p["w"][0])
        got["retry"] = int(((want["left"]["aw"] > w) | (want["right"]["aw"] > w)).sum())
    if "zdrop" in edges:
        q0 = p.copy()
        q0["zdrop"] = 0
        nz = ref(q0)
        got["zdrop"] = int(((want["left"]["cells"] != nz["left"]["cells"]) | (want["right"]["cells"] != nz["right"]["cells"])).sum())
    if "qn" in edges:
        got["qn"] = sum(int((np.asarray(s.get(k, ()), np.uint8) >= 4).any()) for s in sd for k in ("lq", "rq"))
    if "tn" in edges:
        got["tn"] = sum(int((np.asarray(s.get(k, ()), np.uint8) >= 4).any()) for s in sd for k in ("lt", "rt"))
    if "bound8" in edges:
        e8 = (top + b == 255) & (qm > 0)
        got["bound8"] = int(e8.sum())
        got["score_at_bound"] = int((want["score"][e8] == 255 - b).sum())      # perfect matches to the end of both sides
    if "bound16" in edges:
        got["bound16"] = int(((top >= 64936) & (top < 65000) & (qm + 1 <= L.L16_COLS)).sum())
    print(case["name"], len(tasks), got)
    assert all(v > 0 for v in got.values()), (case["name"], sorted(got.items()))


def test_reads_block_is_what_it_claims(host):
    """every length the case names, Ns, a read at every offset modulo 16 of the raw buffer; and the numpy image is the device
    sequence format as bsw_pack_bases makes it, read by read"""
    case, = [c for c in L.CASES if c["entry"] == "reads_upload_async"]
    raw, lens, offs = L.workload(case)
    assert 290 <= len(lens) <= 310 and set(L.READS_LENS) <= set(lens.tolist()) and 250 < lens.max() <= 400
    assert set((offs & 15).tolist()) == set(range(16))
    assert 0.01 < (raw == 4).mean() < 0.03
    img = L.reads_image(raw, lens, offs, 2)
    assert len(img) == sum((int(n) + 15) // 16 for n in lens) + 4 and not img[:2].any() and not img[-2:].any()
    at = 2
    for n, o in zip(lens, offs):
        w = np.full((int(n) + 15) // 16, 0xdeadbeef, dtype=np.uint64)
        r = np.ascontiguousarray(raw[o:o + n])
        host.lib().bsw_pack_bases(r.ctypes.data, int(n), w.ctypes.data)
        assert (img[at:at + len(w)] == w).all(), (n, o)
        at += len(w)
