"""Build audit of the upload encodings: libbwasw_mi355.so exports bsw_reads_upload_enc and bsw_reads_upload_start_enc, the header
and host.EXPORTS know them, the ABI version is unchanged, and the device code went INTO bsw_reads_pack_kernel: there is still
exactly one, without scratch and within the registers of eight waves per SIMD (the kernel set itself is pinned by
test_reads_build_cpu.py and test_kernel_ledger_cpu.py)."""
import os
import re
import subprocess

from test_reads_build_cpu import READS_PACK_KERNEL, kernel_metadata, kernels_matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bsw_reads_upload_enc", "bsw_reads_upload_start_enc")


def test_library_exports_the_two_calls(built):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    for f in NEW:
        assert re.search(r" T %s$" % f, syms, re.M), f
        assert f in built.host.EXPORTS, f
        assert hasattr(built.host.lib(), f)
    assert (built.host.READS_CODES, built.host.READS_ASCII, built.host.READS_PACKED) == (0, 1, 2)


def test_header_declares_the_calls_and_the_abi_version_stays_6(built):
    text = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    assert re.search(r"#define BSW_ABI_VERSION 6\b", text)
    assert built.host.lib().bsw_abi_version() == 6
    for f in NEW:
        assert re.search(r"\bint\s+%s\(bsw_ctx \*ctx, const void \*const \*reads, const int32_t \*lens, size_t n_reads, int encoding, bsw_reads \*\*out\);" % f, text), f
    for name, value in (("CODES", 0), ("ASCII", 1), ("PACKED", 2)):
        assert re.search(r"#define BSW_READS_%s\s+%d\b" % (name, value), text)
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")]
    for f in NEW:
        assert f in threads.split("every other call")[0], f


def test_one_pack_kernel_without_scratch_within_64_vgprs(built):
    meta = kernels_matching(kernel_metadata(built.lib_path()), READS_PACK_KERNEL)
    assert len(meta) == 1, sorted(meta)
    (name, (vgpr, sgpr, scratch)), = meta.items()
    print("bsw_reads_pack_kernel with three encodings: vgpr_count %d sgpr_count %d scratch %d" % (vgpr, sgpr, scratch))
    assert scratch == 0
    assert vgpr <= 64
