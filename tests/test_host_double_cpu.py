"""The library's host side (batch manager, context, scalar queue, wire format: the threaded C++ that otherwise only runs with a
GPU behind it) on a HIP runtime made of host memory, under ASan + UBSan and under TSan.  tests/hip_double/ holds the stand-in
runtime, CPU stand-ins of the kernel launchers that compute real results with the oracle, and the test programs; none of it is
part of the library, and nothing here opens a GPU.  Every program runs under a time limit: a deadlock is a failure.

Not covered: launch_global, launch_global_long, launch_align and launch_cigar_md have no stand-in (they answer
hipErrorNotSupported in these programs), so bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch and bsw_matesw_ref_batch are
not swept.  The ticket-lifetime hazard in slot_main's BSW_DEBUG_TIMING print (id read after chunk_done) was closed by inspection:
neither the ticket storm nor a failure sweep with the switch set made the old code fault."""
import os
import re
import subprocess

import numpy as np
import pytest

import _host_double_build as B

LIMIT = 300          # seconds per program, as tests/test_sanitizers_cpu.py gives asan_plan: the deadlock detector


def run(san, prog, *args, env=None, quiet_stderr=False, expect_ok=True):
    b = B.build(san)
    log = os.path.join(b["dir"], "san_%s_%s" % (prog, "_".join(args)))
    e = B.env(san, **(env or {}))
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log                   # reports survive a discarded stderr
    try:
        out = subprocess.run([b[prog]] + list(args), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL if quiet_stderr else subprocess.PIPE,
                             text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired as ex:
        tail = (ex.stdout or b"")[-600:]
        raise AssertionError("%s %s (%s) hit the time limit of %d s; last output: %r" % (prog, " ".join(args), san, LIMIT, tail))
    reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            reports += open(os.path.join(d, f)).read()[-6000:]
    if expect_ok:
        assert out.returncode == 0 and not reports, (prog, args, san, out.returncode, out.stdout[-1500:], (out.stderr or "")[-4000:], reports[-6000:])
    return out, reports


SANS = ["asan", "tsan"]


# ---- the double stands alone -----------------------------------------------------------------------------------------------
def test_no_hip_symbol_is_left_to_the_runtime_library():
    """Every hip* symbol the host-side objects, the stand-in launchers and the test programs leave undefined is defined by
    tests/hip_double/hip_double.cpp: an entry point the double lacks would be resolved by libamdhip64 at run time."""
    b = B.build("asan")
    defined = set()
    for line in subprocess.check_output(["nm", "--defined-only", b["objs"]["hip_double"]], text=True).splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[1] in "TW":
            defined.add(parts[2])
    assert "hipMalloc" in defined and "hipStreamWaitEvent" in defined
    used = set()
    for name, path in b["objs"].items():
        if name == "hip_double":
            continue
        for line in subprocess.check_output(["nm", "-u", path], text=True).splitlines():
            sym = line.split()[-1]
            if re.match(r"^_?hip[A-Z]", sym):
                used.add(sym)
    assert len(used) >= 25, sorted(used)
    assert used <= defined, "left to libamdhip64: %s" % sorted(used - defined)


def test_standin_class_tables_equal_the_librarys(host):
    """The stand-ins restate the kernels' class tables.  One probe seed per query length through bsw_plan_batch: the program (its
    own tables) and the built library (the kernels' tables) must put every probe into the same segment."""
    out, _ = run("asan", "host_parity", "tables")
    rows = [tuple(int(x) for x in l.split()[1:]) for l in out.stdout.splitlines() if l.startswith("table ")]
    assert len(rows) > 800
    bases = np.ones(16384, dtype=np.uint8)
    p = host.default_params()
    segs_seen = set()
    for kernel, q, at in rows:
        t = np.zeros(1, dtype=host.TASK)
        t["rquery"] = bases.ctypes.data
        t["rtarget"] = bases.ctypes.data
        t["rqlen"], t["rtlen"], t["h0"], t["init_score"] = q, q + 5, 20, -1
        _, seg, _ = host.plan_batch(p, t, kernel=kernel)
        mine = -1
        for s in range(host.PLAN_SEGS - 1):
            if s != 8 and seg[s + 1] > seg[s]:
                mine = s
                break
        assert mine == at, "kernel %d, query of %d bases: the library plans segment %d, the stand-ins' tables %d" % (kernel, q, mine, at)
        segs_seen.add(mine)
    assert set(range(8)) <= segs_seen and {18, 19} & segs_seen, sorted(segs_seen)     # every wave class, lane classes too


# ---- a. parity through the whole host path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("mode", ["cross", "ref", "wire", "scalar"])
def test_parity_through_the_host_path(san, mode):
    """bsw_upload + bsw_run + bsw_download, bsw_submit, bsw_submit_packed, bsw_extend_batch (cross), bsw_extend_ref / bsw_submit_ref
    (ref), bsw_refbatch_* (wire), ksw_extend2 from 8 threads (scalar): equal to the oracle byte for byte, n in {0, 1, 63, 64, 65,
    5 000}, kernel AUTO / LANE / WAVE, 150 and 250 bp reads with Ns and junk, registered and pageable memory, variants H, M, RTL;
    chunk_tasks = 256, so 5 000 seeds are 20 chunks."""
    out, _ = run(san, "host_parity", mode)
    assert (mode + ":") in out.stdout


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_large_resident_batch_reaches_the_n_list(kernel):
    """120 000 two-sided 250 bp seeds as one resident batch.  Under AUTO such a chunk is what nsplit_candidate admits: the launch_bin
    stand-in must have seen an N list that ends behind order[4n+16), the capacity the header used to document."""
    out, _ = run("asan", "host_parity", "big", str(kernel))
    m = re.search(r"big: kernel (\d+), n (\d+), N list ends at (\d+), 4n\+16 = (\d+), beyond (\d+)", out.stdout)
    assert m, out.stdout
    if kernel == 0:
        assert int(m.group(5)) >= 1 and int(m.group(3)) > int(m.group(4)), out.stdout


# ---- b. devices --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", SANS)
def test_parity_on_2_3_and_8_devices(san, tmp_path):
    """2, 3 and 8 devices and one ordinal listed twice: parity, every device computes a disjoint set of seeds and together all of
    them, the reference copy a chunk fetches from lives on the chunk's device; BSW_SYSFS_PCI points at made-up numa_node /
    local_cpulist files (pin_this_thread, bsw_device_placement)."""
    for d in range(8):
        dd = tmp_path / ("0000:%02x:00.0" % (0xA1 + 0x0B * d))
        dd.mkdir()
        (dd / "numa_node").write_text("%d\n" % (d % 2))
        (dd / "local_cpulist").write_text("%d\n" % min(os.sched_getaffinity(0)))      # one CPU this process may run on
    out, _ = run(san, "host_parity", "devices", env={"BSW_SYSFS_PCI": str(tmp_path)})
    assert "devices: ok" in out.stdout


# ---- c. every single HIP failure ---------------------------------------------------------------------------------------------
PARTS = 4


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("part", range(PARTS))
def test_every_single_hip_failure_in_three_submits(san, part):
    """Two devices, three submits in flight (host sequences, packed, resident reference) of 4 chunks each, then a further submit and
    the release: call k of the clean run's C fails, for every k (this case: k = part mod 4).  Every wait returns, the ticket that
    met the failure answers BSW_E_NOMEM / BSW_E_HIP with a text that names the step, every other ticket is bit-exact, nothing stays
    in flight, the context stays usable (a return code never kills it; only the watchdog does), bsw_destroy returns, nothing leaks."""
    out, _ = run(san, "host_faults", "sweep", str(part), str(PARTS))
    m = re.search(r"C = (\d+), injection points visited = (\d+), fired = (\d+) .* skipped 0", out.stdout)
    assert m, out.stdout[-1500:]
    C, visited, fired = (int(x) for x in m.groups())
    assert C > 200 and fired >= (C - 16) // PARTS and visited >= fired, out.stdout[-800:]


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("mode", ["create", "ref_upload"])
def test_every_single_hip_failure_in_construction(san, mode):
    """bsw_create on three devices / bsw_ref_upload on three devices with call k failing, k = 1 .. C: a refused construction unwinds
    completely; a context created without its optional part (fork events, chain flags, placement) computes bit-exact results."""
    out, _ = run(san, "host_faults", mode)
    m = re.search(r"C = (\d+), injection points visited = (\d+)", out.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) > (20 if mode == "create" else 5), out.stdout[-800:]


# ---- d. the watchdog ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", SANS)
def test_watchdog_marks_only_its_context_dead(san):
    """timeout_ms = 300 and a stalled stream: the waiting call (resident upload; ticket wait) answers BSW_E_HIP "timeout", later
    calls say the context is dead, a third context of the process computes bit-exact results, bsw_destroy returns."""
    out, _ = run(san, "host_watchdog", "stall")
    assert "watchdog: ok" in out.stdout


@pytest.mark.parametrize("selftest", [False, True])
def test_chain_timeouts_counts_expired_waits(selftest):
    """bsw_chain_timeouts: with BSW_CHAIN_SELFTEST=1 (a target no count reaches) exactly the number of waits the chain queued,
    otherwise at most that (a stand-in raises its flag when its launch is done, which may be later than the wait's 20 ms).
    Results do not change."""
    out, _ = run("asan", "host_watchdog", "chain", env={"BSW_CHAIN_SELFTEST": "1"} if selftest else None)
    m = re.search(r"chain: (\d+) waits queued, (\d+) expired", out.stdout)
    assert m and int(m.group(1)) > 0 and (int(m.group(2)) == int(m.group(1)) if selftest else int(m.group(2)) <= int(m.group(1))), out.stdout


# ---- e. tickets from many threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", ["tsan", "asan"])
@pytest.mark.parametrize("mode", ["storm", "collide"])
@pytest.mark.parametrize("debug_timing", [False, True])
def test_tickets_from_many_threads(san, mode, debug_timing):
    """The threading contract of include/bwa_sw_mi355.h: 8 threads submit / bsw_test / bsw_wait_ticket on one context while a ninth
    calls bsw_wait and bsw_inflight (storm); a ticket collected by bsw_wait while another thread waits on it answers BSW_E_INVAL
    or its own code and never touches freed memory (collide).  Once more with BSW_DEBUG_TIMING=1 and stderr discarded."""
    out, _ = run(san, "host_tickets", mode, env={"BSW_DEBUG_TIMING": "1"} if debug_timing else None, quiet_stderr=debug_timing)
    assert (mode + ":") in out.stdout


# ---- f. the documented order[] size ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switches", [{}, {"BSW_LANE_FUSE": "0"}, {"BSW_NSPLIT": "1"}, {"BSW_LANE_FUSE": "0", "BSW_NSPLIT": "1"}])
def test_plan_batch_stays_inside_the_documented_order_capacity(switches):
    """bsw_plan_batch under AUTO with more than 100 000 two-sided 250 bp seeds and order[] malloc'ed with exactly the capacity the
    header documents; ASan is the witness (seg[] does not describe the N list).  The switches are read once per process."""
    out, _ = run("asan", "asan_plan", "big", env=switches)
    assert "asan_plan big ok" in out.stdout
    lens = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"n (\d+), order_len (\d+), 4n\+16 = (\d+)", out.stdout)]
    assert len(lens) == 3
    if switches.get("BSW_NSPLIT") == "1" or not switches:
        assert any(ol > old for _, ol, old in lens), "no plan exceeded 4n+16: the run did not reach what it is for: %s" % lens
