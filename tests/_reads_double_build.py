"""Builds tests/hip_double/host_reads.cpp: the objects tests/_host_double_build.py makes (the library's host-side translation
units, the stand-in runtime, the oracles), plus the read store's translation unit, plus a launch_pack stand-in that understands
BSW_PACK_STORE (tests/hip_double/launchers_reads.cpp) in front of launchers.cpp compiled with its own launch_pack renamed.
Test infrastructure."""
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
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_reads.hip"), "-o", obj("bsw_reads")])
    B._cc(hip + ["-Dlaunch_pack=launch_pack_bytes", "-c", os.path.join(B.DBL, "launchers.cpp"), "-o", obj("launchers_bytes")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_reads.cpp"), "-o", obj("launchers_reads")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_reads.cpp"), "-o", obj("host_reads")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_reads")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] + [obj("host_reads"), obj("bsw_reads"), obj("launchers_bytes"), obj("launchers_reads")] + shared +
          ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe
