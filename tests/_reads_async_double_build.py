"""Builds tests/hip_double/host_reads_async.cpp: what tests/_reads_double_build.py links for host_reads, plus the asynchronous
upload's translation unit and a stand-in for its launcher (tests/hip_double/launchers_reads_pack.cpp: the word function restated
as a nibble loop).  A stand-alone program per sanitizer.  Test infrastructure."""
import os

import _host_double_build as B
import _reads_double_build as R

_exe = {}


def program(san):
    if san in _exe:
        return _exe[san]
    R.program(san)                                   # its objects: bsw_reads, launchers_bytes, launchers_reads
    b = B.build(san)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + B.SAN[san]
    hip = [B.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + ["-I", os.path.join(B.ROOT, "include"), "-I", B.DBL]

    def obj(name):
        return os.path.join(b["dir"], name + ".o")
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_reads_async.hip"), "-o", obj("bsw_reads_async")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_reads_pack.cpp"), "-o", obj("launchers_reads_pack")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_reads_async.cpp"), "-o", obj("host_reads_async")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_reads_async")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] + [obj("host_reads_async"), obj("bsw_reads_async"), obj("launchers_reads_pack"), obj("bsw_reads"),
                                                         obj("launchers_bytes"), obj("launchers_reads")] + shared + ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe
