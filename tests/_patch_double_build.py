"""Builds tests/hip_double/host_patch.cpp: the objects of tests/_host_double_build.py (the library's host units, the HIP stand-in,
the oracles), plus the read store's translation unit and the launch_pack stand-in that understands BSW_PACK_STORE
(tests/hip_double/launchers_reads.cpp in front of launchers.cpp compiled with its own launch_pack renamed), as
tests/_reads_double_build.py does.  A stand-alone program per sanitizer, and one without ("plain").  Test infrastructure."""
import os

import _host_double_build as B

B.SAN.setdefault("plain", [])
_exe = {}


def program(san):
    if san in _exe:
        return _exe[san]
    b = B.build(san)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + B.SAN[san]
    hip = [B.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + ["-I", os.path.join(B.ROOT, "include"), "-I", B.DBL]

    def obj(name):
        return os.path.join(b["dir"], name + ".o")
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_reads.hip"), "-o", obj("bsw_reads_p")])
    B._cc(hip + ["-Dlaunch_pack=launch_pack_bytes", "-c", os.path.join(B.DBL, "launchers.cpp"), "-o", obj("launchers_bytes_p")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_reads.cpp"), "-o", obj("launchers_reads_p")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_patch.cpp"), "-o", obj("host_patch")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_patch")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] + [obj("host_patch"), obj("bsw_reads_p"), obj("launchers_bytes_p"), obj("launchers_reads_p")] + shared +
          ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe


if __name__ == "__main__":
    import sys
    print(program(sys.argv[1]))
