"""The device replay of mem_chain2aln's seed loop, without a GPU: the generator of tests/_c2a_device_gen.py is not vacuous,
bsw_c2a_core.h under the host compiler (tests/c2a_core_model.cpp, ASan + UBSan) equals bsw_chain2aln_replay byte for byte on the
generator's sets and on the hand cases, the main library's new unit runs on the HIP stand-in with a CPU launcher built from the
same header (tests/hip_double/host_c2a_device.cpp: plain, ASan, TSan), and the pair of libraries has the shape the ABI promises."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _c2a_device_gen as G
import _host_double_build as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc")
READELF = "/opt/rocm/llvm/bin/llvm-readelf"

# the program of this module: the new unit and the job on top of the base units, the CPU launcher registered by launchers_c2a.cpp
hb.TABLE["host_c2a_device"] = (["bsw_c2a_device", "bsw_chain2aln_job", "bsw_chain2aln.c", "bsw_reads"], ["launchers_c2a"], hb.PACK)

NEW = ["bsw_c2a_device_register", "bsw_c2a_device_load", "bsw_c2a_device_error", "bsw_set_c2a_device", "bsw_c2a_device",
       "bsw_chain2aln_replay_batch", "bsw_chain2aln_replay_submit_t"]


# ---- the generator ----
def flips(a, b):
    return int((a != b).sum())


def test_generator_is_non_vacuous(host):
    """conditions on the HOST replay alone, so that a later edit of the generator cannot hollow the GPU tests out"""
    p = host.default_params()
    for sizes in (G.SMALL, G.MIDDLE, G.LARGE):
        s = G.make(host, 200, sizes, seed=11)
        regs, ext, start = G.host_replay(host, p, s)
        share = ext.mean()
        n = len(ext)
        off = flips(ext, G.host_replay(host, p, s, opt=dict(ovl_len_frac=1e9))[1])
        f0 = flips(ext, G.host_replay(host, p, s, opt=dict(seedlen0_frac=-1.0))[1])
        fr = flips(ext, G.host_replay(host, p, s, opt=dict(seedlen0_frac=1.0 / 3, ovl_len_frac=2.0 / 3))[1])
        per_read = np.diff(start.astype(np.int64))
        print("%s: %d seeds, extended %.2f; un-skip off flips %d, seedlen0_frac = -1 %d, fractions 1/3 and 2/3 %d; reads with > 16 regions %d, > 64 %d"
              % (sizes, n, share, off, f0, fr, (per_read > 16).sum(), (per_read > 64).sum()))
        assert 0.3 <= share <= 0.8
        assert off >= 0.005 * n and f0 >= 0.005 * n and fr >= 0.005 * n
        if sizes is G.MIDDLE:
            assert (per_read > 16).any() and (per_read > 64).any()


# ---- bsw_c2a_core.h under the host compiler ----
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    out = tmp_path_factory.mktemp("c2a_model")
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    objs = []
    for n in ("bsw_chain2aln", "bsw_glue"):
        objs.append(str(out / (n + ".o")))
        subprocess.check_call(["gcc", "-std=gnu11"] + san + ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(CSRC, n + ".c"), "-o", objs[-1]])
    exe = str(out / "c2a_core_model")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + san + [os.path.join(ROOT, "tests", "c2a_core_model.cpp")] + objs + ["-lpthread", "-o", exe])
    return exe


def run_model(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "all equal" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_core_model_hand_cases(model):
    out = run_model(model, "hand")
    assert out.count("hand/") == 23


def test_core_model_equals_the_host_replay_on_the_generators_sets(host, model, tmp_path):
    files = []
    cases = [
        ("small", G.SMALL, {}, host.default_params(), 0, {}, False),
        ("middle", G.MIDDLE, {}, host.default_params(), 0, {}, True),
        ("large", G.LARGE, {}, host.default_params(), 0, {}, False),
        ("no_seedlen0", G.MIDDLE, dict(seedlen0_frac=-1.0), host.default_params(), 0, {}, False),
        ("thirds", G.MIDDLE, dict(seedlen0_frac=1.0 / 3, ovl_len_frac=2.0 / 3), host.default_params(), 0, {}, False),
        ("penalties", G.MIDDLE, {}, G.params(host, **G.PENALTIES[1]), 0, {}, False),
        ("asymmetric", G.MIDDLE, {}, G.params(host, **G.PENALTIES[2]), 0, {}, False),
        ("far", G.MIDDLE, {}, host.default_params(), 1 << 33, {}, False),
        ("cap", G.SMALL, {}, host.default_params(), 0, {1: [host.C2A_DEV_MAX_CHAIN - 1, 3], 3: [host.C2A_DEV_MAX_CHAIN], 4: [2, host.C2A_DEV_MAX_CHAIN + 1, 5]}, False),
    ]
    for name, sizes, opt, p, base, fixed, full in cases:
        s = G.make(host, 60 if fixed else 200, sizes, seed=11, d0_base=base, empty=(0, 7, 59) if fixed else (), chain_sizes=fixed)
        res = G.full_records(host, s["pairs"]) if full else s["pairs"]
        path = str(tmp_path / (name + ".bin"))
        G.dump(path, p, host.c2a_opt(**opt), s, res, res.dtype.itemsize)
        files.append(path)
    out = run_model(model, *files)
    assert out.count(" reads (") == len(cases)
    assert "cap.bin: 57 reads (1 for the host)" in out   # the set around the cap: only the read with a chain of cap + 1 seeds is the host's


# ---- the pair of libraries ----
def test_new_functions_are_exported_and_bound(host):
    L = C.CDLL(host.lib_path())
    hdr = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    for n in NEW:
        assert hasattr(L, n) and n in host.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
        assert getattr(host.lib(), n).argtypes is not None
    assert host.lib().bsw_abi_version() == 6


def test_the_companion_needs_the_main_library_and_never_the_reverse(host):
    here = os.path.dirname(host.lib_path())
    comp = os.path.join(here, "libbwasw_c2a.so")
    assert os.path.exists(comp)
    dyn = subprocess.check_output([READELF, "-d", comp], text=True)
    assert re.search(r"NEEDED.*\[libbwasw_mi355\.so\]", dyn) and "$ORIGIN" in dyn
    main = subprocess.check_output([READELF, "-d", host.lib_path()], text=True)
    assert not re.search(r"NEEDED.*libbwasw", main), main
    dry = subprocess.check_output(["make", "-n", "-C", CSRC, "clean"], text=True)
    assert "libbwasw_c2a.so" in dry and "../libbwasw_mi355_*.so" in dry


def test_the_replay_kernels_are_the_companions_alone(host):
    """the main library's kernel set is pinned elsewhere (tests/test_reads_build_cpu.py); here: the companion holds the three kernels
    of a launch and nothing of the main library's"""
    import test_reads_build_cpu as pin
    here = os.path.dirname(host.lib_path())
    got = pin.kernel_metadata(os.path.join(here, "libbwasw_c2a.so"))
    assert sorted(re.sub(r"^_ZN3bsw\d+", "", k)[:18] for k in got) == ["bsw_c2a_move_kerne", "bsw_c2a_replay_ker", "bsw_c2a_scan_kerne"]
    assert all(v[2] == 0 for v in got.values()), got     # no scratch
    assert not [k for k in pin.kernel_metadata(host.lib_path()) if "c2a" in k]


def test_the_switch_is_refused_without_the_companion():
    """in a fresh process that never loads the companion: bsw_set_c2a_device(1) answers BSW_E_INVAL and leaves the switch off; after
    bsw_c2a_device_load it is accepted; a path without the file is BSW_E_INVAL with a text"""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g\n"
        "h = g.load_package().host\n"
        "L = h.lib()\n"
        "assert L.bsw_c2a_device() == 0\n"
        "assert L.bsw_set_c2a_device(1) == -2 and L.bsw_c2a_device() == 0\n"
        "assert L.bsw_c2a_device_load(b'/nonexistent/libbwasw_c2a.so') == -2 and b'libbwasw_c2a' in L.bsw_c2a_device_error()\n"
        "assert L.bsw_set_c2a_device(1) == -2 and L.bsw_c2a_device() == 0\n"
        "h.c2a_device_load()\n"
        "h.set_c2a_device(1); assert h.c2a_device() == 1\n"
        "h.set_c2a_device(0); assert h.c2a_device() == 0\n"
        "print('ok')\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "BSW_C2A_DEVICE"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr[-3000:])


def test_the_environment_switch_loads_the_companion_on_first_use():
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g\n"
        "h = g.load_package().host\n"
        "assert h.c2a_device() == 1\n"
        "print('ok')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, BSW_C2A_DEVICE="1"))
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr[-3000:])


# ---- the main library's unit on the HIP stand-in ----
@pytest.mark.parametrize("san", ["plain", "asan", "tsan"])
@pytest.mark.parametrize("what", ["calls", "job", "faults", "busy"])
def test_host_double(san, what):
    out = hb.run("host_c2a_device", san, what, limit=600)
    assert what + " ok" in out.stdout, out.stdout[-2000:]


# ---- the Python job object when finish meets BSW_E_BUSY (the C side: host_c2a_device busy) ----
def test_the_job_object_keeps_its_handle_over_busy(host, monkeypatch):
    """Chain2alnJob.finish raises BSW_E_BUSY and keeps the handle and the arrays, then succeeds; release() keeps a job that answers BUSY"""
    class Lib:
        def __init__(self, answers):
            self.answers, self.calls = list(answers), []

        def bsw_chain2aln_finish(self, h, regs, n, ext, start, st):
            self.calls.append((h, regs))
            return self.answers.pop(0)

    class Ctx:
        handle = 1

        def _chk(self, rc, what):
            if rc:
                raise host.BswError(rc, what)

    fake = Lib([-6, -6, 0])
    monkeypatch.setattr(host, "lib", lambda: fake)
    keep = [object()]
    job = host.Chain2alnJob(Ctx(), 1234, 10, 3, keep)
    for _ in range(2):
        with pytest.raises(host.BswError) as ei:
            job.finish()
        assert ei.value.code == -6 and job.handle == 1234 and job._keep is keep
    regs, ext, start, st = job.finish()
    assert job.handle is None and job._keep is None and len(regs) == 0 and len(ext) == 10 and len(start) == 4
    assert [h for h, _ in fake.calls] == [1234] * 3
    # a failure other than BUSY frees the job
    fake.answers = [-4]
    job = host.Chain2alnJob(Ctx(), 77, 10, 3, keep)
    with pytest.raises(host.BswError):
        job.finish()
    assert job.handle is None and job._keep is None
    # release: BUSY keeps the job, anything else lets it go
    fake.answers = [-6, -2]
    job = host.Chain2alnJob(Ctx(), 88, 10, 3, keep)
    job.release()
    assert job.handle == 88 and job._keep is keep
    job.release()
    assert job.handle is None and job._keep is None
