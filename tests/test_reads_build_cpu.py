"""Build audit of the resident-read source of bsw_pack_kernel: the kernel may not need more register allocation blocks or
scratch than before it learnt BSW_PACK_STORE, and no other kernel of the library may have changed at all.  The numbers of the
parent build are code object metadata (vgpr_count, sgpr_count, private_segment_fixed_size) of its libbwasw_mi355.so:
bsw_pack_kernel's below, every kernel's in tests/golden/kernel_resources_before_reads.json.

This file is also the build pin of the library's kernel set: the golden kernels plus ADDED, the kernels that came after the
golden file, each a mangled-name pattern with the exact number of instantiations (added_kernels).  A new kernel gets a line in
ADDED (and a case in tests/_kernel_ledger.py); the audits of the features that brought the kernels import the pin from here."""
import glob
import json
import os
import re
import struct
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"
PACK = "_ZN3bsw15bsw_pack_kernelEPKhPK9bsw_dtaskPK10bsw_rawoffjjiS1_lPK8bsw_refxPmPh"
PACK_BEFORE = (34, 43, 0)          # vgpr_count, sgpr_count, private_segment_fixed_size in the parent build
# the kernels that are not in the golden file: (mangled-name pattern, number of instantiations)
RTL2_KERNEL = r"_ZN3bsw20bsw_lane2_rtl_kernelILi(9|17)ELi(3|2)ELb[01]EEE"
READS_PACK_KERNEL = r"_ZN3bsw21bsw_reads_pack_kernelE"
ALIGN_LONG_KERNEL = r"_ZN3bsw21bsw_align_long_kernelILb[01]EEE"
ADDED = ((RTL2_KERNEL, 4), (READS_PACK_KERNEL, 1), (ALIGN_LONG_KERNEL, 2))


def kernel_metadata(so_path):
    """{mangled kernel name: (vgpr_count, sgpr_count, private_segment_fixed_size)} of the gfx950 code objects"""
    out = {}
    with tempfile.TemporaryDirectory(prefix="reads_audit_") as tmp:
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
                        m = re.search(r"\.?name:\s+(\S+)", block)
                        f = dict((a, int(b)) for a, b in re.findall(r"\.?(vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\d+)", block))
                        if m and len(f) == 3:
                            out[m.group(1)] = (f["vgpr_count"], f["sgpr_count"], f["private_segment_fixed_size"])
            at = data.find(BUNDLE, at + 1)
    return out


def golden():
    """read, not rewritten: the kernels of the build before the resident read store"""
    return {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_reads.json"))).items()}


def kernels_matching(meta, pattern):
    return {k: v for k, v in meta.items() if re.match(pattern, k)}


def added_kernels(meta):
    """the names in meta that ADDED's patterns match, each pattern with exactly its count"""
    out = set()
    for pattern, count in ADDED:
        names = set(kernels_matching(meta, pattern))
        assert len(names) == count, (pattern, sorted(names))
        out |= names
    return out


def assert_kernel_set_is_pinned(got):
    """the library's kernels are the golden ones plus ADDED, and bsw_pack_kernel alone may differ from the golden file"""
    before = golden()
    assert set(got) == set(before) | added_kernels(got)      # no kernel added or removed, instantiations included
    changed = {k: (before[k], got[k]) for k in before if k != PACK and got[k] != before[k]}
    assert not changed, changed


def assert_no_second_library(built):
    """every kernel is in libbwasw_mi355.so: it needs no library of the project's, none is built next to it, and `make clean`
    removes the ones a build from before the single library left there"""
    dyn = subprocess.check_output([READELF, "-d", built.lib_path()], text=True)
    assert not re.search(r"NEEDED.*libbwasw_mi355_", dyn), dyn
    here = os.path.dirname(built.lib_path())
    assert glob.glob(os.path.join(here, "libbwasw_mi355*.so")) == [built.lib_path()]
    dry = subprocess.check_output(["make", "-n", "-C", os.path.join(here, "csrc"), "clean"], text=True)
    assert "../libbwasw_mi355_*.so" in dry


def blocks(n, granule):
    return -(-n // granule)


def test_pack_kernel_needs_no_more_blocks_and_nothing_else_changed(built):
    got = kernel_metadata(built.lib_path())
    assert golden()[PACK] == PACK_BEFORE
    assert_kernel_set_is_pinned(got)
    v, s, p = got[PACK]
    print("bsw_pack_kernel: vgpr %d -> %d, sgpr %d -> %d, scratch %d -> %d" % (PACK_BEFORE[0], v, PACK_BEFORE[1], s, PACK_BEFORE[2], p))
    # occupancy follows the allocation blocks (8 VGPRs, 16 SGPRs on gfx950)
    assert blocks(v, 8) <= blocks(PACK_BEFORE[0], 8) and blocks(s, 16) <= blocks(PACK_BEFORE[1], 16) and p <= PACK_BEFORE[2]


def test_the_library_stands_alone(built):
    assert_no_second_library(built)


def test_the_library_has_the_store_source(built):
    """fails on a build without the feature: the flag and the fetch are what the pack kernel was given"""
    src = open(os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_stage_kernel.hip")).read()
    assert "BSW_PACK_STORE" in src and "bsw_reads_word(" in src
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    assert " T bsw_reads_upload" in syms
