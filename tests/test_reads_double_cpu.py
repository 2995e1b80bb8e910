"""Resident read blocks on the host-memory HIP stand-in (tests/hip_double/), under ASan + UBSan and under TSan: bsw_reads_upload /
bsw_reads_free and the three *_reads_* submits.  No GPU is opened.

tests/hip_double/host_reads.cpp is built by its row in tests/_host_double_build.py: the objects of the base programs, the read
store's translation unit, and a launch_pack stand-in that understands BSW_PACK_STORE (launchers_reads.cpp: a nibble loop over the
store, ASan watching every position) in front of the unchanged launchers.cpp.  Expected values are the pointer forms' results for
the same read bytes.  Every run has a time limit: a ticket that hangs is a failure."""
import functools
import re

import pytest

import _host_double_build as B

LIMIT = 900
SANS = ["asan", "tsan"]
run = functools.partial(B.run, "host_reads", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_reads_submits_equal_the_pointer_forms_on_1_2_3_and_8_devices(san):
    """Extension, rescue and CIGAR over one resident block on 1, 2, 3 and 8 devices, each cut into more chunks than there are
    devices: byte for byte bsw_submit_ref_t / bsw_matesw_ref_batch / bsw_cigar_ref_batch for the same bytes.  CIGAR slices start
    at every phase of a word inside longer reads.  The stand-in dies when a chunk's copy of the block does not live on its
    device.  bsw_reads_free answers BSW_E_BUSY until the last ticket is collected; a bad index, slice or block is refused in the
    caller's thread and makes no ticket."""
    m = re.search(r"parity: (\d+) cases, (\d+) chunks", run(san, "parity").stdout)
    assert m and int(m.group(1)) == 4 and int(m.group(2)) >= 4 * 24


@pytest.mark.parametrize("san", SANS)
def test_upload_and_free_from_a_second_thread_while_tickets_are_in_flight(san):
    m = re.search(r"threads: ok, (\d+) uploads", run(san, "threads").stdout)
    assert m and int(m.group(1)) >= 2


@pytest.mark.parametrize("san", SANS)
def test_every_hip_call_of_upload_and_of_the_three_submits_fails_in_turn(san):
    """nothing leaks, a ticket that reports success is bit-exact, and a context the watchdog did not kill completes the same
    three submits afterwards"""
    m = re.search(r"faults: C = (\d+), swept (\d+), dead (\d+)", run(san, "faults").stdout)
    assert m and int(m.group(2)) * 10 >= int(m.group(1)) * 9 and int(m.group(1)) > 60


@pytest.mark.parametrize("san", SANS)
def test_h2d_bytes_per_task_do_not_grow_with_the_reads(san):
    """bsw_host_stats: 50-base and 250-base reads cost the same bytes per task in all three stages (76 / 112 / 144: records only),
    and rescue and CIGAR cost at most the pointer form's bytes minus the sequence bytes it gathers from pageable memory"""
    out = run(san, "bytes").stdout
    got = re.findall(r"bytes: (\d+)-base reads: extension ([\d.]+), rescue ([\d.]+), CIGAR ([\d.]+) H2D", out)
    assert [g[0] for g in got] == ["50", "250"] and got[0][1:] == got[1][1:] == ("76.0", "112.0", "144.0"), out
    assert "bytes: ok" in out
