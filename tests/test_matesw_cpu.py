"""CPU checks of mate rescue on the resident reference (bsw_matesw_ref_batch): the ABI of bsw_mtask / bsw_mresult, the glue
(bsw_infer_dir, bsw_matesw_windows) against the restatement in tests/_matesw_ref.py, known answers of the restatement's is_rev
mapping (what the GPU tests compare against), and a build audit: the kernels in the library are the ledger's, and no
bsw_align_kernel uses more scratch, or more register allocation blocks, than before it learnt to read a reverse-complemented
query."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _kernel_ledger
import _matesw_ref as mr
from test_kernel_ledger_cpu import compiled_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {c: i for i, c in enumerate("ACGTN")}
PEN = (6, 1, 6, 1)

GENOME = "AATCGGGACACTGAGATTTGTCAGCGTCTACTAGCGTTTG"
L_PAC = len(GENOME)


def enc(s):
    return np.array([CODE[c] for c in s], dtype=np.uint8)


def test_mtask_and_mresult_layout_match_the_header(host, tmp_path):
    fields = [("bsw_mtask", host.MTASK), ("bsw_mresult", host.MRESULT)]
    body = []
    for name, dt in fields:
        body.append('printf("%%zu\\n", sizeof(%s));' % name)
        for f in dt.names:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (name, f))
    for f in host.KSWR.names:
        body.append('printf("%%zu\\n", offsetof(bsw_mresult, aln.%s));' % f)
    src = tmp_path / "lay.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bwa_sw_mi355.h"\nint main(void){%s return 0;}\n' % "".join(body))
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, dt in fields:
        want.append(dt.itemsize)
        want.extend(dt.fields[f][1] for f in dt.names)
    want.extend(host.KSWR.fields[f][1] for f in host.KSWR.names)
    assert got == want
    assert (host.MTASK.itemsize, host.MRESULT.itemsize) == (40, 72)


def test_infer_dir_matches_the_restatement(host):
    assert host.infer_dir(100, 10, 50) == mr.infer_dir(100, 10, 50) == (0, 40)      # same strand, mate to the right
    assert host.infer_dir(100, 50, 10) == mr.infer_dir(100, 50, 10) == (3, 40)      # same strand, mate to the left
    assert host.infer_dir(100, 10, 150) == mr.infer_dir(100, 10, 150) == (1, 39)    # p2 = 199 - 150 = 49
    assert host.infer_dir(100, 60, 150) == mr.infer_dir(100, 60, 150) == (2, 11)
    rng = np.random.default_rng(3)
    for _ in range(20000):
        l_pac = int(rng.integers(1, 1 << 40)) if rng.random() < 0.5 else int(rng.integers(1, 2000))
        pick = lambda: int(rng.choice([0, l_pac - 1, l_pac, 2 * l_pac - 1, int(rng.integers(0, 2 * l_pac))]))
        b1, b2 = pick(), pick()
        assert host.infer_dir(l_pac, b1, b2) == mr.infer_dir(l_pac, b1, b2), (l_pac, b1, b2)


def test_windows_match_the_restatement(host):
    rng = np.random.default_rng(4)
    for it in range(5000):
        l_pac = int(rng.integers(1, 5000)) if it % 3 else int(rng.integers(1, 1 << 36))
        l_ms = int(rng.integers(0, 1025))
        anchor = int(rng.choice([0, 1, l_pac - 1, l_pac, l_pac + 1, 2 * l_pac - 1, int(rng.integers(0, 2 * l_pac))]))
        low = rng.integers(-200, 800, 4).astype(np.int32)
        high = (low + rng.integers(0, 1200, 4)).astype(np.int32)
        failed = (rng.random(4) < 0.3).astype(np.int32)
        got = host.matesw_windows(anchor, l_ms, l_pac, low, high, failed)
        want = mr.windows(anchor, l_ms, l_pac, low.tolist(), high.tolist(), failed.tolist())
        for r in range(4):
            assert (int(got["rb"][r]), int(got["re"][r]), int(got["is_rev"][r]), int(got["skip"][r])) == want[r], (it, r)
            assert 0 <= got["rb"][r] and got["re"][r] <= 2 * l_pac
    # a 500 +- 50 insert, 150 bp mates, anchor at 10 000 on the forward strand: FR (r = 1) looks 300 .. 400 bases on, reversed
    w = host.matesw_windows(10_000, 150, 1_000_000, [300] * 4, [700] * 4, [1, 0, 1, 1])
    assert (int(w["rb"][1]), int(w["re"][1]), int(w["is_rev"][1])) == (10_150, 10_700, 1)
    assert list(w["is_rev"]) == [0, 1, 1, 0] and list(w["skip"]) == [1, 0, 1, 1]
    # clamps at 0 and 2 * l_pac
    w = host.matesw_windows(5, 150, 1000, [0] * 4, [100] * 4, [0] * 4)
    assert int(w["rb"][3]) == 0 and int(w["rb"][2]) == 0
    w = host.matesw_windows(1990, 150, 1000, [0] * 4, [100] * 4, [0] * 4)
    assert int(w["re"][0]) == 2000 and int(w["re"][1]) == 2000


def test_glue_rejects_bad_arguments(host):
    import ctypes as C
    z = np.zeros(4, np.int32)
    out64, out32 = np.zeros(4, np.int64), np.zeros(4, np.int32)
    L = host.lib()
    assert L.bsw_matesw_windows(0, -1, 100, z.ctypes.data, z.ctypes.data, z.ctypes.data, out64.ctypes.data, out64.ctypes.data,
                                out32.ctypes.data, out32.ctypes.data) == -2
    assert L.bsw_matesw_windows(0, 10, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, out64.ctypes.data, out64.ctypes.data,
                                out32.ctypes.data, out32.ctypes.data) == -2
    assert L.bsw_matesw_windows(0, 10, 100, None, z.ctypes.data, z.ctypes.data, out64.ctypes.data, out64.ctypes.data,
                                out32.ctypes.data, out32.ctypes.data) == -2
    assert L.bsw_infer_dir(100, 10, 50, None) == 0
    d = C.c_int64(0)
    assert L.bsw_infer_dir(100, 10, 50, C.byref(d)) == 0 and d.value == 40


# ---- known answers of the restatement's mapping (a 40-base genome, l_pac = 40; forward [5, 30) = GGACACTGAGATTTGTCAGCGTCTA) ----

@pytest.fixture(scope="module")
def pac():
    import _gencigar_ref as gc
    return gc.pack_pac(enc(GENOME))


def rescue(oracle, host, pac, mate, is_rev, rb, re, min_score=5):
    return mr.matesw(oracle, host.bwa_matrix(), PEN, L_PAC, pac, mate, is_rev, rb, re, mr.xtra_of(len(mate), 1, 5), min_score)


def test_forward_mate_on_the_forward_strand(oracle, host, pac):
    b = rescue(oracle, host, pac, enc(GENOME[12:22]), 0, 5, 30)      # GAGATTTGTC at window offset 7
    assert (b["aln"]["score"], b["aln"]["tb"], b["aln"]["te"], b["aln"]["qb"], b["aln"]["qe"]) == (10, 7, 16, 0, 9)
    assert (b["status"], b["rb"], b["re"], b["qb"], b["qe"], b["score"], b["seedcov"]) == (0, 12, 22, 0, 10, 10, 5)


def test_reversed_mate_lands_on_the_reverse_strand(oracle, host, pac):
    # the mate is revcomp(forward [12, 22)): aligned as that forward stretch, reported at [80 - 22, 80 - 12) = [58, 68)
    b = rescue(oracle, host, pac, mr.revcomp(enc(GENOME[12:22])), 1, 5, 30)
    assert (b["aln"]["tb"], b["aln"]["te"], b["aln"]["qb"], b["aln"]["qe"]) == (7, 16, 0, 9)
    assert (b["status"], b["rb"], b["re"], b["qb"], b["qe"], b["seedcov"]) == (0, 80 - (5 + 16 + 1), 80 - (5 + 7), 0, 10, 5)
    assert (b["rb"], b["re"]) == (58, 68)


def test_reversed_mate_in_a_reverse_strand_window_lands_forward(oracle, host, pac):
    # window [45, 70) of the reverse strand; revcomp(mate) = its bases [48, 58): the mate is forward [22, 32) = AGCGTCTACT
    b = rescue(oracle, host, pac, enc(GENOME[22:32]), 1, 45, 70)
    assert (b["aln"]["tb"], b["aln"]["te"], b["aln"]["qb"], b["aln"]["qe"]) == (3, 12, 0, 9)
    assert (b["status"], b["rb"], b["re"], b["qb"], b["qe"]) == (0, 80 - (45 + 12 + 1), 80 - (45 + 3), 0, 10)
    assert (b["rb"], b["re"]) == (22, 32)


def test_reversed_mate_with_a_clipped_end_flips_qb_and_qe(oracle, host, pac):
    # aligned query = TGA + GAGATTTGTC (TGA mismatches forward [9, 12) = ACT): qb = 3, qe = 12 of 13 in the aligned frame;
    # in read order the mate's first 10 bases align and its last 3 are clipped: qb = 13 - 13 = 0, qe = 13 - 3 = 10
    mate = mr.revcomp(enc("TGA" + GENOME[12:22]))
    b = rescue(oracle, host, pac, mate, 1, 5, 30)
    assert (b["aln"]["score"], b["aln"]["tb"], b["aln"]["te"], b["aln"]["qb"], b["aln"]["qe"]) == (10, 7, 16, 3, 12)
    assert (b["status"], b["rb"], b["re"], b["qb"], b["qe"], b["seedcov"]) == (0, 58, 68, 0, 10, 5)
    # the same query forwards keeps the aligned frame
    f = rescue(oracle, host, pac, enc("TGA" + GENOME[12:22]), 0, 5, 30)
    assert (f["rb"], f["re"], f["qb"], f["qe"]) == (12, 22, 3, 13)


def test_keep_decision_and_status_cases(oracle, host, pac):
    b = rescue(oracle, host, pac, enc(GENOME[12:22]), 0, 5, 30, min_score=11)        # score 10 < min_score: run, not kept
    assert b["status"] == 2 and b["aln"]["score"] == 10 and (b["rb"], b["re"], b["score"]) == (0, 0, 0)
    for rb, re in [(30, 30), (31, 30), (35, 45), (-1, 10), (70, 81)]:
        b = rescue(oracle, host, pac, enc(GENOME[12:22]), 0, rb, re)
        assert b["status"] == 1 and b["aln"] == mr.NOT_RUN
    assert rescue(oracle, host, pac, enc(""), 0, 5, 30)["status"] == 1


# ---- build audit ----

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"
# bsw_align_kernel<SLEN, BYTE> in the parent build: (vgpr_count, sgpr_count, private_segment_fixed_size) per the code object
# metadata of libbwasw_mi355.so before the kernel learnt BSW_AD_QRC
ALIGN_BEFORE = {(8, True): (57, 100, 0), (10, True): (65, 106, 0), (16, True): (92, 106, 0), (32, True): (161, 106, 68),
                (64, True): (385, 106, 68), (16, False): (92, 106, 0), (20, False): (123, 106, 0), (32, False): (141, 106, 68),
                (64, False): (365, 106, 68), (128, False): (512, 108, 512)}


def align_kernel_metadata(so_path):
    """{(SLEN, BYTE): (vgpr_count, sgpr_count, private_segment_fixed_size)} of the gfx950 bsw_align_kernel instantiations"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="matesw_") as tmp:
        fb = os.path.join(tmp, "fatbin")
        subprocess.check_call(["objcopy", "--dump-section", ".hip_fatbin=" + fb, so_path, os.path.join(tmp, "copy.so")])
        data = open(fb, "rb").read()
        at, k = data.find(BUNDLE), 0
        while at >= 0:
            n = struct.unpack_from("<Q", data, at + 24)[0]
            p = at + 32
            for _ in range(n):
                off, size, idlen = struct.unpack_from("<QQQ", data, p)
                triple = data[p + 24:p + 24 + idlen].decode()
                p += 24 + idlen
                if triple.endswith("-gfx950") and size:
                    co = os.path.join(tmp, "co%d" % k)
                    k += 1
                    with open(co, "wb") as f:
                        f.write(data[at + off:at + off + size])
                    notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
                    for block in re.split(r"\n\s+- \.", notes):
                        m = re.search(r"\.?name:\s+_ZN3bsw16bsw_align_kernelILi(\d+)ELb([01])E", block)
                        if not m:
                            continue
                        f = dict((a, int(b)) for a, b in re.findall(r"\.?(vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\d+)",
                                                                    block))
                        out[(int(m.group(1)), m.group(2) == "1")] = (f["vgpr_count"], f["sgpr_count"], f["private_segment_fixed_size"])
            at = data.find(BUNDLE, at + 1)
    return out


def test_build_has_the_ledgers_kernels(built):
    ks = compiled_kernels(built.lib_path())
    assert ks == _kernel_ledger.targets() | set(_kernel_ledger.UNREACHED)
    assert sum(1 for x in ks if x.startswith("bsw::bsw_align_kernel<")) == len(ALIGN_BEFORE)


def blocks(n, granule):
    return -(-n // granule)


def test_align_kernels_use_no_more_register_blocks_or_scratch(built):
    """The reverse-complement read costs one or two VGPRs in some instantiations (the counts are printed); occupancy follows
    the allocation blocks (8 VGPRs, 16 SGPRs on gfx950), and those, like the scratch size, must not grow."""
    got = align_kernel_metadata(built.lib_path())
    assert set(got) == set(ALIGN_BEFORE)
    for key, (v0, s0, p0) in sorted(ALIGN_BEFORE.items()):
        v, s, p = got[key]
        print("bsw_align_kernel<%d, %s>: vgpr %d -> %d, sgpr %d -> %d, scratch %d -> %d" % (key + (v0, v, s0, s, p0, p)))
        assert blocks(v, 8) <= blocks(v0, 8) and blocks(s, 16) <= blocks(s0, 16) and p <= p0, (key, got[key], ALIGN_BEFORE[key])
