"""Builds tests/hip_double/host_align_long.cpp: the objects of tests/_host_double_build.py (the library's host units, the HIP
stand-in, the stand-in launchers, the oracle), plus the unit that owns the switch of ksw_align2's long-query route
(csrc/bsw_align_long.hip) and a stand-in for its launcher (tests/hip_double/launchers_align_long.cpp: the oracle, and a check of
every task's class).  A stand-alone program per sanitizer.  Test infrastructure."""
import os

import _host_double_build as B

_exe = {}


def program(san):
    if san in _exe:
        return _exe[san]
    b = B.build(san)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + B.SAN[san]
    hip = [B.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + ["-I", os.path.join(B.ROOT, "include"), "-I", B.DBL]

    def obj(name):
        return os.path.join(b["dir"], name + ".o")
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_align_long.hip"), "-o", obj("bsw_align_long")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_align_long.cpp"), "-o", obj("launchers_align_long")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_align_long.cpp"), "-o", obj("host_align_long")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "launchers", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_align_long")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] + [obj("host_align_long"), obj("bsw_align_long"), obj("launchers_align_long")] + shared + ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe


if __name__ == "__main__":
    import sys
    print(program(sys.argv[1]))
