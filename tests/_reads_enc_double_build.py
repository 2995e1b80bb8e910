"""Builds tests/hip_double/host_reads_enc.cpp: what tests/_reads_async_double_build.py links for host_reads_async, with the
program replaced and with a stand-in for launch_reads_pack that honours every record's encoding
(tests/hip_double/launchers_reads_pack_enc.cpp: the word function restated per base for codes, letters and 4-bit words).  A
stand-alone program per sanitizer.  Test infrastructure."""
import os

import _host_double_build as B
import _reads_async_double_build as A

_exe = {}


def program(san):
    if san in _exe:
        return _exe[san]
    A.program(san)                                   # its objects: bsw_reads, bsw_reads_async, launchers_bytes, launchers_reads
    b = B.build(san)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + B.SAN[san]
    hip = [B.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + ["-I", os.path.join(B.ROOT, "include"), "-I", B.DBL]

    def obj(name):
        return os.path.join(b["dir"], name + ".o")
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_reads_pack_enc.cpp"), "-o", obj("launchers_reads_pack_enc")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_reads_enc.cpp"), "-o", obj("host_reads_enc")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_reads_enc")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] + [obj("host_reads_enc"), obj("bsw_reads_async"), obj("launchers_reads_pack_enc"), obj("bsw_reads"),
                                                         obj("launchers_bytes"), obj("launchers_reads")] + shared + ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe
