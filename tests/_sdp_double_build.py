"""Builds tests/hip_double/host_sdp.cpp exactly as tests/_chain2aln_double_build.py builds host_chain2aln: the objects of
tests/_host_double_build.py (the library's host units, the HIP stand-in, the oracles), the read store's translation unit and the
launch_pack stand-in that understands BSW_PACK_STORE, plus the two units of the feature under test: bsw_sdp.c (the engine) and
bsw_sdp_job.hip (the job).  A stand-alone program per sanitizer, and one without ("plain").  Test infrastructure."""
import os

import _host_double_build as B

B.SAN.setdefault("plain", [])
_exe = {}


def program(san):
    if san in _exe:
        return _exe[san]
    b = B.build(san)
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + B.SAN[san]
    inc = ["-I", os.path.join(B.ROOT, "include")]
    hip = [B.HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + inc + ["-I", B.DBL]

    def obj(name):
        return os.path.join(b["dir"], name + ".o")
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_reads.hip"), "-o", obj("bsw_reads_sdp")])
    B._cc(hip + ["-Dlaunch_pack=launch_pack_bytes", "-c", os.path.join(B.DBL, "launchers.cpp"), "-o", obj("launchers_bytes_sdp")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "launchers_reads.cpp"), "-o", obj("launchers_reads_sdp")])
    B._cc(hip + ["-c", os.path.join(B.CSRC, "bsw_sdp_job.hip"), "-o", obj("bsw_sdp_job")])
    B._cc([B.CLANG, "-std=gnu11"] + flags + inc + ["-c", os.path.join(B.CSRC, "bsw_sdp.c"), "-o", obj("bsw_sdp")])
    B._cc(hip + ["-c", os.path.join(B.DBL, "host_sdp.cpp"), "-o", obj("host_sdp")])
    shared = [b["objs"][n] for n in B.HOST_HIP + B.HOST_C + ["hip_double", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    exe = os.path.join(b["dir"], "host_sdp")
    B._cc([B.HIPCC, "-fno-gpu-sanitize"] + B.SAN[san] +
          [obj(n) for n in ("host_sdp", "bsw_sdp_job", "bsw_sdp", "bsw_reads_sdp", "launchers_bytes_sdp", "launchers_reads_sdp")] + shared +
          ["-o", exe, "-lpthread"])
    _exe[san] = exe
    return exe


if __name__ == "__main__":
    import sys
    print(program(sys.argv[1]))
