"""Builds and runs the host-double test programs (tests/hip_double/): the library's host-side translation units compiled host-only
with a sanitizer (or without: "plain"), linked against the host-memory HIP stand-in and the CPU stand-ins of the kernel launchers.
TABLE has one row per program; build() makes what every program shares and the base programs, program() one program of the
table, run() runs one and collects the sanitizers' reports.  Test infrastructure."""
import atexit
import concurrent.futures
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc")
DBL = os.path.join(ROOT, "tests", "hip_double")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"

SAN = {
    "plain": [],
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}
HOST_HIP = ["bsw_ctx", "bsw_batch", "bsw_scalar", "bsw_wire", "bsw_f4", "bsw_cigar", "bsw_matesw"]
HOST_C = ["bsw_synth", "bsw_glue", "bsw_refbatch"]
ORACLES = ["oracle_extend", "oracle_global", "oracle_align", "oracle_rtl"]
PROGRAMS = ["host_parity", "host_f4", "host_faults", "host_watchdog", "host_tickets", "asan_plan"]      # the base programs: build() links them

# The launch_pack stand-in a program links: plain launchers.cpp, or (PACK) launchers_reads.cpp, which understands BSW_PACK_STORE,
# in front of launchers.cpp compiled with its own launch_pack renamed.
PACK = True
# program: (library units on top of HOST_HIP + HOST_C: csrc/NAME.hip, or csrc/NAME.c where written so,
#           stand-in units on top of hip_double: tests/hip_double/NAME.cpp,
#           PACK or not)
# A program's link set is part of what it tests (a program linked without bsw_align_long sees no long-route table): a new
# program gets a row of its own, never a wider row of another's.
TABLE = {n: ([], [], not PACK) for n in PROGRAMS}
TABLE.update({
    "host_f4_stream": ([], [], not PACK),
    "host_reads": (["bsw_reads"], [], PACK),
    "host_reads_async": (["bsw_reads_async", "bsw_reads"], ["launchers_reads_pack"], PACK),
    "host_reads_enc": (["bsw_reads_async", "bsw_reads"], ["launchers_reads_pack_enc"], PACK),
    "host_align_long": (["bsw_align_long"], ["launchers_align_long"], not PACK),
    "host_patch": (["bsw_reads"], [], PACK),
    "host_chain2aln": (["bsw_chain2aln_job", "bsw_chain2aln.c", "bsw_reads"], [], PACK),
    "host_sdp": (["bsw_sdp_job", "bsw_sdp.c", "bsw_reads"], [], PACK),
})

_built = {}
_extra = {}          # (san, object name) -> path: what program() compiled on top of build(), each once


def _cc(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr[-6000:]))


def _cc_all(jobs):
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(_cc, jobs))


def _compilers(san):
    """-> (flags, include path, the hipcc line for a host-only C++ unit, the clang line for a C unit)"""
    inc = ["-I", os.path.join(ROOT, "include")]
    flags = ["-O1", "-g", "-fno-omit-frame-pointer"] + SAN[san]
    hip = [HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-fno-gpu-sanitize"] + flags + inc
    return flags, inc, hip, [CLANG, "-std=gnu11"] + flags + inc


def _link(san, exe, objs):
    _cc([HIPCC, "-fno-gpu-sanitize"] + SAN[san] + objs + ["-o", exe, "-lpthread"])
    return exe


def build(san):
    """-> {"dir": ..., "objs": {name: path}, base program name: path}; built once per process and sanitizer."""
    if san in _built:
        return _built[san]
    out = tempfile.mkdtemp(prefix="host_double_%s_" % san)
    atexit.register(shutil.rmtree, out, True)
    _, inc, hip, cc = _compilers(san)
    jobs, objs = [], {}

    def obj(name):
        objs[name] = os.path.join(out, name + ".o")
        return objs[name]
    for n in HOST_HIP:
        jobs.append(hip + ["-c", os.path.join(CSRC, n + ".hip"), "-o", obj(n)])
    for n in HOST_C:
        jobs.append(cc + ["-c", os.path.join(CSRC, n + ".c"), "-o", obj(n)])
    for n in ("hip_double", "launchers"):
        jobs.append(hip + ["-c", os.path.join(DBL, n + ".cpp"), "-o", obj(n)])
    for n in PROGRAMS:
        src = os.path.join(ROOT, "tests", "asan_plan.cpp") if n == "asan_plan" else os.path.join(DBL, n + ".cpp")
        jobs.append(hip + ["-I", DBL, "-c", src, "-o", obj(n)])
    # the oracle is the yardstick, not the code under test: optimised, not instrumented (tests/asan_host.c runs it under ASan)
    for src, name in (("ksw_extend_ref.c", "oracle_extend"), ("ksw_global_ref.c", "oracle_global"), ("ksw_align_ref.c", "oracle_align")):
        jobs.append([CLANG, "-O2", "-std=gnu11"] + inc + ["-c", os.path.join(ROOT, "oracle", src), "-o", obj(name)])
    jobs.append([CLANG, "-O2", "-std=gnu11"] + inc + ["-c", os.path.join(ROOT, "tests", "ksw_extend_rtl_ref.c"), "-o", obj("oracle_rtl")])
    _cc_all(jobs)
    shared = [objs[n] for n in HOST_HIP + HOST_C + ["hip_double", "launchers"] + ORACLES]
    res = {"dir": out, "objs": objs}
    for n in PROGRAMS:
        res[n] = _link(san, os.path.join(out, n), [objs[n]] + shared)
    _built[san] = res
    return res


def program(name, san):
    """-> the path of one program of TABLE: its row's units compiled on top of build(san), each distinct (source, defines) pair
    once per process and sanitizer whichever program asks first, and linked with exactly its row."""
    b = build(san)
    if name in b:
        return b[name]
    lib, standin, pack = TABLE[name]
    _, _, hip, cc = _compilers(san)
    hip = hip + ["-I", DBL]
    want = {name: hip + ["-c", os.path.join(DBL, name + ".cpp")]}
    for n in lib:
        want[n] = cc + ["-c", os.path.join(CSRC, n)] if n.endswith(".c") else hip + ["-c", os.path.join(CSRC, n + ".hip")]
    for n in standin + (["launchers_reads"] if pack else []):
        want[n] = hip + ["-c", os.path.join(DBL, n + ".cpp")]
    if pack:
        want["launchers_bytes"] = hip + ["-Dlaunch_pack=launch_pack_bytes", "-c", os.path.join(DBL, "launchers.cpp")]
    jobs = []
    for n, cmd in want.items():
        if (san, n) not in _extra:
            _extra[san, n] = os.path.join(b["dir"], n + ".o")
            jobs.append(cmd + ["-o", _extra[san, n]])
    _cc_all(jobs)
    shared = [b["objs"][n] for n in HOST_HIP + HOST_C + ["hip_double"] + ([] if pack else ["launchers"]) + ORACLES]
    b[name] = _link(san, os.path.join(b["dir"], name), [_extra[san, n] for n in want] + shared)
    return b[name]


def env(san, **extra):
    e = dict(os.environ)
    e["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    e["LSAN_OPTIONS"] = "suppressions=" + os.path.join(DBL, "lsan.supp") + ":print_suppressions=0"
    e["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    e["TSAN_OPTIONS"] = "halt_on_error=1:second_deadlock_stack=1"
    e.update(extra)
    return e


_env = env           # run() has a parameter of that name


def run(name, san, *args, limit, env=None, quiet_stderr=False, expect_ok=True):
    """Runs program `name` of TABLE, built for `san`, under a time limit of `limit` seconds: a hang is a failure.  `env` adds
    variables (None: unset).  -> the CompletedProcess, with the sanitizers' reports as .reports; unless expect_ok is False, an
    exit status other than 0 or any report fails the caller's test."""
    exe = program(name, san)
    log = os.path.join(os.path.dirname(exe), "san_" + re.sub(r"\W+", "_", "_".join((name,) + args)))
    e = _env(san)
    for k, v in (env or {}).items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log                   # reports survive a discarded stderr
    try:
        out = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL if quiet_stderr else subprocess.PIPE,
                             text=True, timeout=limit, env=e)
    except subprocess.TimeoutExpired as ex:
        raise AssertionError("%s %s (%s) hit the time limit of %d s; last output: %r" % (name, " ".join(args), san, limit, (ex.stdout or b"")[-600:]))
    out.reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            out.reports += open(os.path.join(d, f)).read()[-6000:]
    if expect_ok:
        assert out.returncode == 0 and not out.reports, (name, args, san, out.returncode, out.stdout[-1500:], (out.stderr or "")[-4000:], out.reports[-6000:])
    return out


if __name__ == "__main__":
    # SAN [KEEP_DIR] [PROGRAM | all]: the base build, and one program of TABLE or all of them on top of it
    import sys
    b = build(sys.argv[1])
    rest = sys.argv[2:]
    names = [a for a in rest if a in TABLE or a == "all"]
    for n in TABLE if "all" in names else names:
        print(program(n, sys.argv[1]))
    print(b["dir"])
    for keep in [a for a in rest if a not in names][:1]:
        shutil.rmtree(keep, True)
        shutil.copytree(b["dir"], keep)
