"""Builds the host-double test programs (tests/hip_double/): the library's host-side translation units compiled host-only with a
sanitizer, linked against the host-memory HIP stand-in and the CPU stand-ins of the kernel launchers.  Test infrastructure."""
import atexit
import concurrent.futures
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc")
DBL = os.path.join(ROOT, "tests", "hip_double")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"

SAN = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}
HOST_HIP = ["bsw_ctx", "bsw_batch", "bsw_scalar", "bsw_wire", "bsw_f4", "bsw_cigar", "bsw_matesw"]
HOST_C = ["bsw_synth", "bsw_glue", "bsw_refbatch"]
PROGRAMS = ["host_parity", "host_f4", "host_faults", "host_watchdog", "host_tickets", "asan_plan"]

_built = {}


def _cc(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr[-6000:]))


def build(san):
    """-> {"dir": ..., "objs": {name: path}, program name: path}; built once per process and sanitizer."""
    if san in _built:
        return _built[san]
    out = tempfile.mkdtemp(prefix="host_double_%s_" % san)
    atexit.register(shutil.rmtree, out, True)
    inc = ["-I", os.path.join(ROOT, "include")]
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + SAN[san]
    hip = [HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + inc
    jobs, objs = [], {}

    def obj(name):
        objs[name] = os.path.join(out, name + ".o")
        return objs[name]
    for n in HOST_HIP:
        jobs.append(hip + ["-c", os.path.join(CSRC, n + ".hip"), "-o", obj(n)])
    for n in HOST_C:
        jobs.append([CLANG, "-std=gnu11"] + flags + inc + ["-c", os.path.join(CSRC, n + ".c"), "-o", obj(n)])
    for n in ("hip_double", "launchers"):
        jobs.append(hip + ["-c", os.path.join(DBL, n + ".cpp"), "-o", obj(n)])
    for n in PROGRAMS:
        src = os.path.join(ROOT, "tests", "asan_plan.cpp") if n == "asan_plan" else os.path.join(DBL, n + ".cpp")
        jobs.append(hip + ["-I", DBL, "-c", src, "-o", obj(n)])
    # the oracle is the yardstick, not the code under test: optimised, not instrumented (tests/asan_host.c runs it under ASan)
    for src, name in (("ksw_extend_ref.c", "oracle_extend"), ("ksw_global_ref.c", "oracle_global"), ("ksw_align_ref.c", "oracle_align")):
        jobs.append([CLANG, "-O2", "-std=gnu11"] + inc + ["-c", os.path.join(ROOT, "oracle", src), "-o", obj(name)])
    jobs.append([CLANG, "-O2", "-std=gnu11"] + inc + ["-c", os.path.join(ROOT, "tests", "ksw_extend_rtl_ref.c"), "-o", obj("oracle_rtl")])
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(_cc, jobs))
    shared = [objs[n] for n in HOST_HIP + HOST_C + ["hip_double", "launchers", "oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]]
    res = {"dir": out, "objs": objs}
    for n in PROGRAMS:
        exe = os.path.join(out, n)
        _cc([HIPCC, "-fno-gpu-sanitize"] + SAN[san] + [objs[n]] + shared + ["-o", exe, "-lpthread"])
        res[n] = exe
    _built[san] = res
    return res


def env(san, **extra):
    e = dict(os.environ)
    e["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    e["LSAN_OPTIONS"] = "suppressions=" + os.path.join(DBL, "lsan.supp") + ":print_suppressions=0"
    e["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    e["TSAN_OPTIONS"] = "halt_on_error=1:second_deadlock_stack=1"
    e.update(extra)
    return e


if __name__ == "__main__":
    import sys
    b = build(sys.argv[1])
    print(b["dir"])
    if len(sys.argv) > 2:
        keep = sys.argv[2]
        shutil.rmtree(keep, True)
        shutil.copytree(b["dir"], keep)
