"""CPU checks of the long-query global alignment (bsw_global_long_kernel.hip): the public limit and a build audit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bwa_sw_mi355.h")
SRC = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_global_long_kernel.hip")


def header_define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(HDR).read(), re.M)
    assert m, name
    return int(m.group(1))


def test_global_limit_equals_extension_limit():
    assert header_define("BSW_GLOBAL_MAX_QLEN") == header_define("BSW_MAX_QLEN") == 8191


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernel_builds_for_gfx950_without_scratch():
    out = subprocess.check_output(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function",
                                   "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", SRC, "-o", "-"],
                                  stderr=subprocess.DEVNULL, text=True)
    assert "bsw_global_long_kernel" in out
    sizes = [int(x) for x in re.findall(r"ScratchSize: (\d+)", out)]
    assert sizes and all(x == 0 for x in sizes), sizes
    spills = [int(x) for x in re.findall(r"\.(?:s|v)gpr_spill_count:\s+(\d+)", out)]
    assert all(x == 0 for x in spills), spills
