"""Build audit of ksw_align2's long-query route: libbwasw_mi355.so (whose kernel set is pinned by test_reads_build_cpu.py and
test_kernel_ledger_cpu.py) holds the two instantiations of bsw_align_long_kernel without scratch, exports the three calls and
needs no second library, and the ABI version is unchanged."""
import os
import re
import subprocess

from test_reads_build_cpu import ALIGN_LONG_KERNEL, assert_no_second_library, kernel_metadata, kernels_matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bsw_set_align_long", "bsw_align_long", "bsw_align_long_stats")


def class_geometry(so):
    """[(byte mode, slen bound, alignments per workgroup, LDS bytes per alignment, LDS bytes per workgroup)] per class, as the
    built library's launcher computes them (bsw_alnl_class_geometry)"""
    import ctypes as C
    lib = C.CDLL(so)
    fn = lib.bsw_alnl_class_geometry
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    out, cls = [], 0
    while True:
        byte, slen, apb, per, wg = C.c_int(), C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        if fn(cls, C.byref(byte), C.byref(slen), C.byref(apb), C.byref(per), C.byref(wg)) != 0:
            return out
        out.append((byte.value, slen.value, apb.value, per.value, wg.value))
        cls += 1


def test_library_holds_the_two_long_kernels_without_scratch(built):
    meta = kernels_matching(kernel_metadata(built.lib_path()), ALIGN_LONG_KERNEL)
    assert len(meta) == 2, sorted(meta)                              # 8-bit and 16-bit mode
    for name, (vgpr, sgpr, scratch) in sorted(meta.items()):
        print("%s: vgpr_count %d sgpr_count %d scratch %d" % (name, vgpr, sgpr, scratch))
        assert scratch == 0
        assert vgpr <= 64                                            # the rows live in LDS, not in registers: eight waves per SIMD fit
    geo = class_geometry(built.lib_path())
    assert [(g[0], g[1]) for g in geo] == [(1, b) for b in (16, 32, 64, 128, 256, 512)] + [(0, b) for b in (32, 64, 128, 256, 512, 1024)]
    for byte, slen, apb, per, wg in geo:
        lanes = 16 if byte else 8
        print("%s mode, slen bound %4d: %2d alignments per workgroup (%3d lanes), dynamic LDS %6d bytes per alignment, %6d per workgroup" % (
            "8-bit" if byte else "16-bit", slen, apb, apb * lanes, per, wg))
        assert per >= 7 * slen * lanes                               # H and E in a dword, Hmax, the query code: 7 bytes a position
        assert (per // 4) % 32 == lanes                              # neighbouring alignments on different banks (32 banks of a dword)
        assert wg == apb * per and wg <= 160 << 10 and 1 <= apb * lanes <= 256
        assert apb * lanes >= 64 or 2 * wg > 160 << 10               # less than a wavefront only where LDS leaves no room for more
    assert [g[2] for g in geo if g[1] * (16 if g[0] else 8) == 8192] == [2, 2]      # the largest class of each mode: two alignments


def test_main_library_exports_the_three_calls_and_stands_alone(built):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    for f in NEW:
        assert re.search(r" T %s$" % f, syms, re.M), f
        assert f in built.host.EXPORTS, f
        assert hasattr(built.host.lib(), f)
    assert_no_second_library(built)


def test_abi_version_stays_6_and_the_header_declares_the_calls(built):
    text = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    assert re.search(r"#define BSW_ABI_VERSION 6\b", text)
    assert built.host.lib().bsw_abi_version() == 6
    assert re.search(r"#define BSW_ALIGN_LONG_MAX_QLEN 8191\b", text) and re.search(r"#define BSW_ALIGN_MAX_QLEN 1024\b", text)
    assert re.search(r"\bvoid\s+bsw_set_align_long\(int mode\);", text)
    assert re.search(r"\bint\s+bsw_align_long\(void\);", text)
    assert re.search(r"\bint\s+bsw_align_long_stats\(uint64_t \*launches, int cap\);", text)
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")]
    assert "bsw_set_align_long" in threads


def test_switch_and_counters_without_a_gpu(built):
    """the switch is process-wide state of the host library: no device is opened by these three calls"""
    host = built.host
    was = host.align_long()
    try:
        for mode, want in ((1, 1), (2, 2), (0, 0), (3, 0), (-1, 0)):
            host.set_align_long(mode)
            assert host.align_long() == want
    finally:
        host.set_align_long(was)
    st = host.align_long_stats()
    assert len(st) == 12 and host.lib().bsw_align_long_stats(None, 0) == 12
    assert host.ALIGN_LONG_MAX_QLEN == 8191
