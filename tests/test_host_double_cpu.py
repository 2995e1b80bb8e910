"""The library's host side (batch manager, context, scalar queue, wire format: the threaded C++ that otherwise only runs with a
GPU behind it) on a HIP runtime made of host memory, under ASan + UBSan and under TSan.  tests/hip_double/ holds the stand-in
runtime, CPU stand-ins of the kernel launchers that compute real results with the oracle, and the test programs; none of it is
part of the library, and nothing here opens a GPU.  Every program runs under a time limit: a deadlock is a failure.

The global, align, CIGAR and mate-rescue hosts (bsw_f4.hip, bsw_cigar.hip, bsw_matesw.hip) run here too: launch_global,
launch_global_long, launch_align and launch_cigar_md have stand-ins that compute with the oracle from the staged words and check
every list, class and scratch slice.  bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch and bsw_matesw_ref_batch are
compared over every class, strand, status, retry count and memory kind (f4), across the task-count, backtrack-byte and
sub-optimal-list bounds of their sub-batch loops (f4split; the 2^31 sequence-byte bound is not reached here), from many threads
through the scalar queue (f4scalar), and with every single HIP call failing in turn.  The ticket-lifetime hazard in slot_main's BSW_DEBUG_TIMING print (id read after chunk_done) was closed by inspection:
neither the ticket storm nor a failure sweep with the switch set made the old code fault."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _gencigar_ref as gc
import _host_double_build as B
import _matesw_ref as ms

LIMIT = 300          # seconds per program, as tests/test_sanitizers_cpu.py gives asan_plan: the deadlock detector
run = functools.partial(B.run, limit=LIMIT)


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
    out = run("host_parity", "asan", "tables")
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


def test_standin_align_and_global_class_tables_equal_the_kernel_sources():
    """The stand-ins restate kAlignClasses, kGlobalClasses and the ring of the long global classes.  The initialisers are parsed
    from the kernel sources: a class added or changed there without the stand-ins fails here."""
    out = run("host_parity", "asan", "tables")
    lines = [l.split() for l in out.stdout.splitlines()]

    def src(name):
        return open(os.path.join(B.CSRC, name)).read()
    m = re.search(r"kAlignClasses\[\]\s*=\s*\{(.*?)\};", src("bsw_align_kernel.hip"), re.S)
    align = [(int(a), int(b)) for a, b in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1))]
    assert len(align) >= 10
    m = re.search(r"kGlobalClasses\[\]\s*=\s*\{(.*?)\};", src("bsw_global_kernel.hip"), re.S)
    glob = [int(x) for x in re.findall(r"\d+", m.group(1))]
    assert len(glob) >= 5
    nlong = int(re.search(r"GLOBAL_LONG_CLASSES\s*=\s*(\d+)", src("bsw_stage.h")).group(1))
    ring = re.search(r"const int ring = (\d+) << cls;", src("bsw_global_long_kernel.hip"))
    assert ring, "the ring size of a long global class is no longer written as N << cls"

    def class_of(q, byte):
        for c, (b, slen) in enumerate(align):
            if b == byte and q <= slen * (16 if byte else 8):
                return c
        return -1
    assert [int(l[1]) for l in lines if l[0] == "alignclasses"] == [len(align)]
    got = {(int(l[1]), int(l[2])): int(l[3]) for l in lines if l[0] == "alignclass"}
    assert len(got) == 2 * 1026
    for (byte, q), c in got.items():
        assert c == class_of(q, byte), (byte, q, c, class_of(q, byte))
    assert set(got.values()) == set(range(len(align))) | {-1}
    assert [int(l[1]) for l in lines if l[0] == "globalclasses"] == [len(glob)]
    assert [(int(l[1]), int(l[2])) for l in lines if l[0] == "globalclass"] == [(c, 64 * v) for c, v in enumerate(glob)]
    assert [int(l[1]) for l in lines if l[0] == "globallongclasses"] == [nlong]
    assert [(int(l[1]), int(l[2])) for l in lines if l[0] == "globallong"] == [(c, int(ring.group(1)) << c) for c in range(nlong)]


# ---- a. parity through the whole host path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("mode", ["cross", "ref", "wire", "scalar"])
def test_parity_through_the_host_path(san, mode):
    """bsw_upload + bsw_run + bsw_download, bsw_submit, bsw_submit_packed, bsw_extend_batch (cross), bsw_extend_ref / bsw_submit_ref
    (ref), bsw_refbatch_* (wire), ksw_extend2 from 8 threads (scalar): equal to the oracle byte for byte, n in {0, 1, 63, 64, 65,
    5 000}, kernel AUTO / LANE / WAVE, 150 and 250 bp reads with Ns and junk, registered and pageable memory, variants H, M, RTL;
    chunk_tasks = 256, so 5 000 seeds are 20 chunks."""
    out = run("host_parity", san, mode)
    assert (mode + ":") in out.stdout


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_large_resident_batch_reaches_the_n_list(kernel):
    """120 000 two-sided 250 bp seeds as one resident batch.  Under AUTO such a chunk is what nsplit_candidate admits: the launch_bin
    stand-in must have seen an N list that ends behind order[4n+16), the capacity the header used to document."""
    out = run("host_parity", "asan", "big", str(kernel))
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
    out = run("host_parity", san, "devices", env={"BSW_SYSFS_PCI": str(tmp_path)})
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
    out = run("host_faults", san, "sweep", str(part), str(PARTS))
    m = re.search(r"C = (\d+), injection points visited = (\d+), fired = (\d+) .* skipped 0", out.stdout)
    assert m, out.stdout[-1500:]
    C, visited, fired = (int(x) for x in m.groups())
    assert C > 200 and fired >= (C - 16) // PARTS and visited >= fired, out.stdout[-800:]


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("mode", ["create", "ref_upload"])
def test_every_single_hip_failure_in_construction(san, mode):
    """bsw_create on three devices / bsw_ref_upload on three devices with call k failing, k = 1 .. C: a refused construction unwinds
    completely; a context created without its optional part (fork events, chain flags, placement) computes bit-exact results."""
    out = run("host_faults", san, mode)
    m = re.search(r"C = (\d+), injection points visited = (\d+)", out.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) > (20 if mode == "create" else 5), out.stdout[-800:]


# ---- d. the watchdog ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", SANS)
def test_watchdog_marks_only_its_context_dead(san):
    """timeout_ms = 300 and a stalled stream: the waiting call (resident upload; ticket wait) answers BSW_E_HIP "timeout", later
    calls say the context is dead, a third context of the process computes bit-exact results, bsw_destroy returns."""
    out = run("host_watchdog", san, "stall")
    assert "watchdog: ok" in out.stdout


@pytest.mark.parametrize("selftest", [False, True])
def test_chain_timeouts_counts_expired_waits(selftest):
    """bsw_chain_timeouts: with BSW_CHAIN_SELFTEST=1 (a target no count reaches) exactly the number of waits the chain queued,
    otherwise at most that (a stand-in raises its flag when its launch is done, which may be later than the wait's 20 ms).
    Results do not change."""
    out = run("host_watchdog", "asan", "chain", env={"BSW_CHAIN_SELFTEST": "1"} if selftest else None)
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
    out = run("host_tickets", san, mode, env={"BSW_DEBUG_TIMING": "1"} if debug_timing else None, quiet_stderr=debug_timing)
    assert (mode + ":") in out.stdout


# ---- f. the documented order[] size ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switches", [{}, {"BSW_LANE_FUSE": "0"}, {"BSW_NSPLIT": "1"}, {"BSW_LANE_FUSE": "0", "BSW_NSPLIT": "1"}])
def test_plan_batch_stays_inside_the_documented_order_capacity(switches):
    """bsw_plan_batch under AUTO with more than 100 000 two-sided 250 bp seeds and order[] malloc'ed with exactly the capacity the
    header documents; ASan is the witness (seg[] does not describe the N list).  The switches are read once per process."""
    out = run("asan_plan", "asan", "big", env=switches)
    assert "asan_plan big ok" in out.stdout
    lens = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"n (\d+), order_len (\d+), 4n\+16 = (\d+)", out.stdout)]
    assert len(lens) == 3
    if switches.get("BSW_NSPLIT") == "1" or not switches:
        assert any(ol > old for _, ol, old in lens), "no plan exceeded 4n+16: the run did not reach what it is for: %s" % lens


# ---- g. the global, align, CIGAR and mate-rescue hosts ----------------------------------------------------------------------------
class F4File:
    """What host_f4 wrote: the genome, the scoring, and per batch call the caller's inputs next to the library's results."""

    def __init__(self, path):
        self.cigar, self.mate = [], []
        for line in open(path):
            w = line.split()
            if w[0] == "genome":
                self.l_pac = int(w[1])
                self.pac = np.frombuffer(bytes.fromhex(w[2]), dtype=np.uint8).copy()
            elif w[0] == "params":
                v = [int(x) for x in w[1:]]
                self.mat, self.pen = np.array(v[:25], dtype=np.int8), tuple(v[25:29])
            elif w[0] == "cigarcase":
                self.cigar.append(dict(max_cigar=int(w[2]), max_md=int(w[3]), want_cigar=int(w[4]), want_md=int(w[5]), what=w[6], rows=[]))
            elif w[0] == "matecase":
                self.mate.append(dict(what=w[2], rows=[]))
            elif w[0] == "c":
                a, b, c, d = line[2:].split("|")
                a = a.split()
                self.cigar[-1]["rows"].append(dict(read=seq_of(a[0]), rb=int(a[1]), re=int(a[2]), w=int(a[3]), w_cap=int(a[4]), min_score=int(a[5]),
                                                   max_tries=int(a[6]), res=[int(x) for x in b.split()], cig=[int(x) for x in c.split()],
                                                   md=d.strip()))
            elif w[0] == "m":
                a, b, c = line[2:].split("|")
                a = a.split()
                self.mate[-1]["rows"].append(dict(mate=seq_of(a[0]), is_rev=int(a[1]), rb=int(a[2]), re=int(a[3]), xtra=int(a[4]), min_score=int(a[5]),
                                                  aln=[int(x) for x in b.split()], res=[int(x) for x in c.split()]))


def seq_of(digits):
    return np.zeros(0, np.uint8) if digits == "-" else np.frombuffer(digits.encode(), dtype=np.uint8) - ord("0")


def compare_cigar_case(oracle, f, case):
    """-> the expectations (tests/_gencigar_ref.reg2aln on the caller's bytes), after comparing every field with them."""
    wants = []
    mc, mm = case["max_cigar"], case["max_md"]
    for i, r in enumerate(case["rows"]):
        w = gc.reg2aln(oracle, f.mat, f.pen, f.l_pac, f.pac, r["read"], r["rb"], r["re"], r["w"], r["w_cap"], r["min_score"], r["max_tries"])
        wants.append(w)
        score, n_cigar, nm, md_len, bw, tries, status, pad = r["res"]
        md = "" if r["md"] in ("-", "?") else r["md"]
        ctxt = (case["what"], mc, mm, i, len(r["read"]), r["rb"], r["re"], w.get("runs"), r["res"])
        assert (status, tries, bw, pad) == (w["status"], w["tries"], w["w"], 0), ctxt
        if w["status"]:
            assert (score, n_cigar, nm, md_len, md) == (0, 0, -1, 0, ""), ctxt
            continue
        assert score == w["score"], ctxt
        n = len(w["cigar"])
        if n > mc:
            assert (n_cigar, nm, md_len, md) == (-n, -1, 0, ""), ctxt
            continue
        assert n_cigar == n and nm == w["nm"], ctxt
        if case["want_cigar"]:
            assert [(x & 0xf, x >> 4) for x in r["cig"]] == w["cigar"], ctxt
        if not case["want_md"]:
            assert md_len == len(w["md"]), ctxt
        elif len(w["md"]) + 1 <= mm:
            assert (md_len, md) == (len(w["md"]), w["md"]), ctxt
        else:
            assert (md_len, md) == (-(len(w["md"]) + 1), ""), ctxt
    return wants


def compare_mate_case(oracle, f, case):
    wants = []
    for i, r in enumerate(case["rows"]):
        w = ms.matesw(oracle, f.mat, f.pen, f.l_pac, f.pac, r["mate"], r["is_rev"], r["rb"], r["re"], r["xtra"], r["min_score"])
        wants.append(w)
        ctxt = (case["what"], i, len(r["mate"]), r["is_rev"], r["rb"], r["re"], hex(r["xtra"]), r["aln"], r["res"], w)
        assert r["aln"] == [w["aln"][k] for k in ms.ALN], ctxt
        assert r["res"] == [w["status"], w["rb"], w["re"], w["qb"], w["qe"], w["score"], w["csub"], w["seedcov"], 0], ctxt
    return wants


@pytest.mark.parametrize("san", SANS)
def test_f4_hosts_parity(san, oracle, tmp_path):
    """bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch, bsw_matesw_ref_batch: n in {0, 1, 63, 64, 65, 2 600}, registered and
    pageable reads (the direct and the gather branch of every host).  Global and local alignment are compared with the oracle by
    the program; CIGAR / NM / MD / w / tries / status and the mate-rescue mapping here, with reg2aln and matesw on the caller's
    bytes.  The workload's reach is asserted on the expectations: status 1, both strands, the no-gap shortcut with one and two
    tries, retry loops of 1, 2 and 3 tries, CIGAR and MD overflow, cigars == NULL, md == NULL."""
    path = str(tmp_path / "f4.txt")
    out = run("host_f4", san, "f4", path)
    assert re.search(r"f4: 12 cases", out.stdout), out.stdout
    f = F4File(path)
    assert len(f.cigar) == 2 * (6 + 4) and len(f.mate) == 12
    assert {(c["max_cigar"], c["max_md"], c["want_cigar"], c["want_md"]) for c in f.cigar} == {(64, 512, 1, 1), (3, 512, 1, 1), (64, 6, 1, 1), (64, 512, 0, 1),
                                                                                              (64, 512, 1, 0)}
    for case in f.cigar:
        wants = compare_cigar_case(oracle, f, case)
        rows = case["rows"]
        if len(rows) >= 2600:
            live = [(r, w) for r, w in zip(rows, wants) if not w["status"]]
            assert sum(1 for w in wants if w["status"]) >= 100
            assert {r["rb"] >= f.l_pac for r, _ in live} == {False, True}
            nogap = [w for _, w in live if w["band"] is None]
            assert {w["tries"] for w in nogap} == {1, 2}, "the no-gap shortcut with and without a second try"
            assert {w["tries"] for _, w in live if w["band"] is not None} == {1, 2, 3}
            by_round = [sum(1 for _, w in live if w["band"] is not None and len(set(w["runs"])) >= k) for k in (1, 2, 3)]
            assert by_round[0] > by_round[1] > by_round[2] > 0, by_round          # survivors thin out per round
        if len(rows) == 65 and case["max_cigar"] == 3:
            assert sum(1 for w in wants if not w["status"] and len(w["cigar"]) > 3) >= 5
        if len(rows) == 65 and case["max_md"] == 6:
            assert sum(1 for w in wants if not w["status"] and len(w["md"]) + 1 > 6) >= 5
    for case in f.mate:
        wants = compare_mate_case(oracle, f, case)
        if len(wants) >= 2600:
            assert {w["status"] for w in wants} == {0, 1, 2}
            assert sum(1 for w in wants if w["status"] == 0 and w["csub"] > 0) >= 20


@pytest.mark.parametrize("which", ["count", "z", "b"])
def test_f4_hosts_across_a_sub_batch_bound(which, oracle, tmp_path):
    """One bound of the hosts' sub-batch loops per case (ASan): 2^20 + 37 tiny tasks through each of the four calls (count);
    a bsw_global_batch and a bsw_cigar_ref_batch of 141 alignments of 8 000 bases that need more than 4 GiB of backtrack bytes
    (z); a bsw_align_batch and a bsw_matesw_ref_batch of 4 651 windows of 65 535 bases, more than 2^28 target bases under KSW_XSUBO
    (b).  The tasks cycle through D distinct ones (D odd): the program compares result k with result k mod D byte for byte and
    the first D with the oracle (global, align) or hands them over (CIGAR, mate rescue: compared here).  Every call must have
    made at least two sub-batches."""
    path = str(tmp_path / "split.txt")
    out = run("host_f4", "asan", "f4split", which, path)
    m = re.search(r"f4split %s: sub-batches global (\d+) align (\d+) cigar (\d+) matesw (\d+)" % which, out.stdout)
    assert m, out.stdout[-800:]
    assert all(int(x) >= 2 for x in m.groups()), out.stdout[-300:]
    f = F4File(path)
    assert len(f.cigar) == (0 if which == "b" else 1) and len(f.mate) == (0 if which == "z" else 1)
    for case in f.cigar:
        wants = compare_cigar_case(oracle, f, case)
        assert len(wants) >= 5
        if which == "count":
            assert sum(1 for w in wants if not w["status"] and re.search(r"[ACGT^]", w["md"])) * 4 >= len(wants)
        else:
            assert all(not w["status"] and 3 <= len(w["cigar"]) <= case["max_cigar"] for w in wants)
    for case in f.mate:
        wants = compare_mate_case(oracle, f, case)
        subo = [w for w, r in zip(wants, case["rows"]) if r["xtra"] & 0x40000 and w["status"] != 1]
        assert len(subo) >= 5 and len(subo) < len(wants) or which == "count"
        assert sum(1 for w in subo if w["aln"]["score2"] >= 0) * 4 >= len(subo), [w["aln"] for w in subo]
        assert sum(1 for w in subo if w["aln"]["tb"] >= 0) * 4 >= len(subo), [w["aln"] for w in subo]


@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_scalar_queue_groups_of_three_kinds(san):
    """12 threads call ksw_global2, ksw_global, ksw_align2, ksw_align and ksw_extend2 at once under three scorings (one trip holds
    several groups of each kind); a 13th keeps calling ksw_align2 with a 2 000-base query.  Everyone but the offender gets the
    oracle's answer every time, the offender gets score -1, and bsw_scalar_stats shows fewer trips than calls."""
    out = run("host_f4", san, "f4scalar", quiet_stderr=True)
    m = re.search(r"f4scalar: (\d+) calls in (\d+) trips, offender calls (\d+)", out.stdout)
    assert m and int(m.group(2)) < int(m.group(1)) and int(m.group(3)) >= 3, out.stdout


def test_byte_mode_tasks_the_align_hosts_reject():
    """KSW_XBYTE with a matrix whose smallest entry is 1 or 2 (BSW_E_INVAL) or with a gap open + extend of 256 (BSW_E_LIMIT) through
    bsw_align_batch, bsw_matesw_ref_batch, ksw_align2 and ksw_align: the code, a text that names KSW_XBYTE, the reason and the
    task; the scalar calls answer score -1.  The same batches in 16-bit mode, a smallest entry of 0 and sums of 255 in 8-bit mode
    run and equal the oracle (ASan)."""
    out = run("host_f4", "asan", "rejects", quiet_stderr=True)
    assert re.search(r"rejects: 4 cases refused, 4 ran", out.stdout), out.stdout


@pytest.mark.parametrize("san", SANS)
@pytest.mark.parametrize("call", ["global", "align", "cigar", "matesw"])
def test_every_single_hip_failure_in_an_f4_batch_call(san, call):
    """Call k of the C counted HIP calls of a clean batch call fails, for every k in 1..C, with pageable and with registered reads:
    the call answers BSW_E_NOMEM / BSW_E_HIP with a text (a release whose code is ignored by design: success and exact results),
    the same call repeated on the same context is bit-exact, bsw_destroy returns, nothing leaks.  The cigar batch runs up to three
    tries, so failures inside the retry loop are reached."""
    out = run("host_f4", san, "faults", call)
    m = re.search(r"faults %s: C = (\d+), injection points visited = (\d+), failed calls (\d+), ignored releases (\d+), skipped 0" % call, out.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) >= 40 and int(m.group(3)) >= 36, out.stdout[-800:]


@pytest.mark.parametrize("san", SANS)
def test_the_sub_batch_cutter_on_made_up_costs(san):
    """cut_spans (csrc/bsw_f4_host.h), which cuts all four batch calls and both ticketed submits, called directly with small caps
    on made-up costs: the spans are contiguous and cover [0, n); no span exceeds a hard cap unless it is a single task; a span
    under a work target closes at the first task boundary at or past the target and not before; each of the five hard bounds
    (tasks, backtrack bytes, sequence bytes, list entries, output bytes) and the work target closes spans on its own — the
    sequence-byte bound too, which no batch of the other programs reaches; n = 0 yields no span, one task over every cap one."""
    out = run("host_f4", san, "cuts")
    m = re.search(r"cuts: ok, (\d+) spans, closed by tasks (\d+) z (\d+) seq (\d+) bl (\d+) out (\d+) work (\d+)", out.stdout)
    assert m and all(int(x) >= 20 for x in m.groups()), out.stdout[-600:]
