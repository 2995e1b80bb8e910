"""Build audit of the asynchronous read-block upload: bsw_reads_pack_kernel lives in a companion library of its own next to
libbwasw_mi355.so (whose kernel set is pinned by test_reads_build_cpu.py and test_kernel_ledger_cpu.py), the main library exports
the four entry points, lists the companion as needed and finds it next to itself, the ABI version is unchanged, and no kernel of
the main library changed."""
import json
import os
import re
import subprocess

from test_reads_build_cpu import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
COMPANION = "libbwasw_mi355_rdpack.so"
NEW = ("bsw_reads_upload_start", "bsw_reads_test", "bsw_reads_wait", "bsw_reads_image")


def test_companion_holds_exactly_the_pack_kernel_without_scratch(built):
    so = os.path.join(os.path.dirname(built.lib_path()), COMPANION)
    assert os.path.exists(so)
    meta = kernel_metadata(so)
    assert len(meta) == 1, sorted(meta)
    (name, (vgpr, sgpr, scratch)), = meta.items()
    print("bsw_reads_pack_kernel: vgpr_count %d sgpr_count %d scratch %d" % (vgpr, sgpr, scratch))
    assert re.match(r"_ZN3bsw21bsw_reads_pack_kernelE", name), name
    assert scratch == 0
    assert vgpr <= 64                                    # eight waves per SIMD: the kernel hides its loads behind other waves
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert re.search(r" T _ZN3bsw17launch_reads_packE", syms)


def test_main_library_exports_the_four_calls_and_needs_the_companion(built):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    for f in NEW:
        assert re.search(r" T %s$" % f, syms, re.M), f
        assert f in built.host.EXPORTS, f
        assert hasattr(built.host.lib(), f)
    dyn = subprocess.check_output([READELF, "-d", built.lib_path()], text=True)
    assert re.search(r"NEEDED.*\[%s\]" % re.escape(COMPANION), dyn)
    assert re.search(r"R(UN)?PATH.*\$ORIGIN", dyn)
    assert not [k for k in kernel_metadata(built.lib_path()) if "bsw_reads_pack_kernel" in k]


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


def test_main_librarys_kernels_are_the_ones_from_before_the_read_store(built):
    """read, not rewritten: tests/golden/kernel_resources_before_reads.json.  bsw_pack_kernel is the one kernel the read store
    changed (test_reads_build_cpu.py bounds it); every other kernel's register metadata is what it was."""
    from test_reads_build_cpu import PACK
    before = {k: tuple(v) for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_reads.json"))).items()}
    got = kernel_metadata(built.lib_path())
    assert set(got) == set(before)
    assert {k for k in before if got[k] != before[k]} <= {PACK}
