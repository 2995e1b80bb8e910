"""Build audit of the asynchronous read-block upload: libbwasw_mi355.so (whose kernel set is pinned by test_reads_build_cpu.py
and test_kernel_ledger_cpu.py) holds bsw_reads_pack_kernel without scratch, exports the four entry points and needs no second
library, and the ABI version is unchanged."""
import os
import re
import subprocess

from test_reads_build_cpu import READS_PACK_KERNEL, assert_no_second_library, kernel_metadata, kernels_matching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bsw_reads_upload_start", "bsw_reads_test", "bsw_reads_wait", "bsw_reads_image")


def test_library_holds_exactly_one_pack_kernel_without_scratch(built):
    meta = kernels_matching(kernel_metadata(built.lib_path()), READS_PACK_KERNEL)
    assert len(meta) == 1, sorted(meta)
    (name, (vgpr, sgpr, scratch)), = meta.items()
    print("bsw_reads_pack_kernel: vgpr_count %d sgpr_count %d scratch %d" % (vgpr, sgpr, scratch))
    assert scratch == 0
    assert vgpr <= 64                                    # eight waves per SIMD: the kernel hides its loads behind other waves


def test_main_library_exports_the_four_calls_and_stands_alone(built):
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
    for f in NEW:
        assert re.search(r"\bint\s+%s\(bsw_ctx \*ctx" % f, text), f
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")]
    for f in NEW[:3]:
        assert f in threads.split("every other call")[0], f
    assert "bsw_reads_image" in threads.split("every other call")[1]
