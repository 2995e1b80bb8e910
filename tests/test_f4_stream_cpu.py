"""bsw_cigar_ref_submit_t / bsw_matesw_ref_submit_t — the CIGAR and mate-rescue jobs of the slot pipeline — on the host-memory HIP
stand-in (tests/hip_double/), under ASan + UBSan and under TSan.  No GPU is opened.

tests/hip_double/host_f4_stream.cpp is a row of tests/_host_double_build.py's table, linked against the objects of the base
programs (the library's host-side translation units, the stand-in runtime and launchers, the oracles).  Its workloads are those of host_f4.cpp;
its expected values are the synchronous calls' results on a one-device context, which tests/test_host_double_cpu.py compares with
the restatements of bwa on the same workloads.  Every run has a time limit: a ticket that hangs is a failure.

The ABI side (header, host.EXPORTS, the Python bindings) is checked at the end of the file without a GPU."""
import functools
import os
import re

import pytest

import _host_double_build as B

LIMIT = 900          # seconds per program run: the fault sweep rebuilds its scenario once per injection point
SANS = ["asan", "tsan"]
run = functools.partial(B.run, "host_f4_stream", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_submits_equal_the_synchronous_calls_on_1_2_3_and_8_devices(san):
    """Rescue and CIGAR submits on 1, 2, 3 and 8 devices, registered and pageable reads, cut into more chunks than the contexts
    have slots: byte for byte what bsw_cigar_ref_batch / bsw_matesw_ref_batch return on a one-device context.  The workloads hold
    all statuses, both strands, is_rev 0 and 1, 1 / 2 / 3 tries and the no-gap shortcut (checked by the program).  The stand-in
    pack launch dies when a chunk's reference copy does not live on its stream's device: the runs on 2, 3 and 8 devices used each
    device's own copy.  Malformed tasks are refused with the synchronous calls' code and text and make no ticket."""
    out = run(san, "parity").stdout
    m = re.search(r"parity: (\d+) cases, (\d+) chunks", out)
    assert m and int(m.group(1)) == 8 and int(m.group(2)) > 8 * 40, out[-400:]


@pytest.mark.parametrize("san", SANS)
def test_a_submit_reaches_every_device(san):
    """Every stream of device 1 of a two-device context stalled: a multi-chunk submit completes device 0's chunks and no more,
    bsw_test stays 0; released, it completes with the right results."""
    assert "reach: ok" in run(san, "reach").stdout


@pytest.mark.parametrize("san", SANS)
def test_four_mixed_submits_in_flight_and_busy_for_the_fifth(san):
    """Extension, rescue, CIGAR and extension again in flight on one context: a fifth submit of any kind and the synchronous calls
    answer BSW_E_BUSY and change nothing; every ticket gets its own results; the synchronous calls work again afterwards."""
    assert "mixed: ok" in run(san, "mixed").stdout


@pytest.mark.parametrize("san", SANS)
def test_nine_threads_submit_and_collect_mixed_tickets(san):
    """The scenario of host_tickets.cpp with three kinds of tickets: eight threads submit, poll and collect, a ninth keeps calling
    bsw_wait and bsw_inflight."""
    out = run(san, "storm").stdout
    assert re.search(r"storm: 40 submits", out), out[-400:]


@pytest.mark.parametrize("san", SANS)
def test_every_hip_call_of_a_three_ticket_scenario_fails_in_turn(san):
    """One extension, one rescue and one CIGAR submit in flight; call k of the scenario fails, for every k until none fires.  Every
    ticket completes; a failing ticket carries the failure itself (code and text); tickets that report success have correct
    results; a context that is not dead completes a further submit of every kind bit-exactly; nothing is left alive after
    bsw_destroy; ASan sees no read of a freed host vector."""
    out = run(san, "faults").stdout
    m = re.search(r"injection points visited = (\d+), a ticket failed (\d+) times", out)
    assert m and int(m.group(1)) >= 150 and int(m.group(2)) >= 100, out[-600:]


@pytest.mark.parametrize("san", SANS)
def test_the_watchdog_fails_the_ticket_and_marks_the_context_dead(san):
    """A stalled stream under timeout_ms = 300: the wait answers BSW_E_HIP with a timeout text, later submits and the synchronous
    call answer BSW_E_HIP on the dead context."""
    assert "watchdog: ok" in run(san, "watchdog").stdout


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_name_both_submits(host):
    hdr = open(os.path.join(B.ROOT, "include", "bwa_sw_mi355.h")).read()
    for name in ("bsw_cigar_ref_submit_t", "bsw_matesw_ref_submit_t"):
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert name in host.EXPORTS
    assert re.search(r"#define BSW_ABI_VERSION 6\b", hdr)
    assert callable(host.BswContext.submit_cigar_ref) and callable(host.BswContext.submit_matesw_ref)
    thr = hdr[hdr.index("THREADS."):]
    thr = thr[:thr.index("every other call")]
    assert "bsw_cigar_ref_submit_t" in thr and "bsw_matesw_ref_submit_t" in thr
