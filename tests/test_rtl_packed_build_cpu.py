"""Build audit of the packed variant-RTL kernels: libbwasw_mi355.so — whose kernel set is pinned by test_reads_build_cpu.py and
test_kernel_ledger_cpu.py — holds exactly the four instantiations of bsw_lane2_rtl_kernel at the occupancy their launch bounds
ask for, exports the switch and needs no second library."""
import os
import re
import subprocess

from test_reads_build_cpu import RTL2_KERNEL, assert_no_second_library, kernel_metadata, kernels_matching

# bsw_lane2_rtl_kernel<QB, WPS, SYM>: 72 columns at three waves per SIMD, 136 at two; shared / separate gap penalties
WANT = {(9, 3, True), (9, 3, False), (17, 2, True), (17, 2, False)}


def test_library_holds_exactly_the_four_rtl_instantiations(built):
    meta = kernels_matching(kernel_metadata(built.lib_path()), RTL2_KERNEL)
    got = set()
    for name, (vgpr, sgpr, scratch) in sorted(meta.items()):
        m = re.match(r"_ZN3bsw20bsw_lane2_rtl_kernelILi(\d+)ELi(\d+)ELb([01])EEEv", name)
        assert m, "unexpected instantiation: %s" % name
        got.add((int(m.group(1)), int(m.group(2)), m.group(3) == "1"))
        print("bsw_lane2_rtl_kernel<%s, %s, %s>: vgpr_count %d sgpr_count %d scratch %d" % (m.group(1), m.group(2), m.group(3), vgpr, sgpr, scratch))
        # the occupancy the launch bounds ask for: 512 VGPRs per SIMD lane in allocation blocks of 8, nothing in scratch
        assert vgpr <= (512 // int(m.group(2))) // 8 * 8 and scratch == 0
    assert got == WANT and len(meta) == 4


def test_main_library_exports_the_switch_and_stands_alone(built):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    for f in ("bsw_set_rtl_packed", "bsw_rtl_packed", "bsw_rtl_packed_stats"):
        assert re.search(r" T %s$" % f, syms, re.M), f
    assert_no_second_library(built)


def test_switch_defaults_off_and_counts_nothing_without_launches(built):
    """host-only: no GPU is touched.  (BSW_RTL_PACKED=1 in the environment turns the initial value on: a fresh process shows it.)"""
    import sys
    code = ("import __graft_entry__ as g; h = g.load_package().host; a = h.rtl_packed(); h.set_rtl_packed(1); b = h.rtl_packed(); h.set_rtl_packed(0); "
            "print(int(a), int(b), int(h.rtl_packed()), sum(h.rtl_packed_stats()))")
    env = {k: v for k, v in os.environ.items() if k != "BSW_RTL_PACKED"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    assert subprocess.check_output([sys.executable, "-c", code], env=env, text=True).split() == ["0", "1", "0", "0"]
    env["BSW_RTL_PACKED"] = "1"
    assert subprocess.check_output([sys.executable, "-c", code], env=env, text=True).split() == ["1", "1", "0", "0"]
