"""The asynchronous read-block upload on the host-memory HIP stand-in (tests/hip_double/), under ASan + UBSan and under TSan, as
stand-alone programs: bsw_reads_upload_start / bsw_reads_test / bsw_reads_wait / bsw_reads_image, the upload jobs on the slot
threads, and the ordering of the three *_reads_* submits behind an upload in flight.  No GPU is opened.

tests/hip_double/host_reads_async.cpp is built by its row in tests/_host_double_build.py: host_reads' objects, the new translation
unit, and a stand-in for launch_reads_pack that restates the word function as a nibble loop (launchers_reads_pack.cpp).  Expected
values: bsw_reads_upload's image, and the pointer forms' results for the same read bytes.  Every run has a time limit."""
import functools
import re

import pytest

import _host_double_build as B

LIMIT = 900
SANS = ["asan", "tsan"]
run = functools.partial(B.run, "host_reads_async", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_image_and_held_tickets_on_1_2_3_and_8_devices(san):
    """The image of every device's copy equals bsw_reads_upload's, reads in pageable memory (gathered) and in one registered
    arena (one DMA of the span), one piece per device and several.  With every stream held, the three tickets submitted right
    behind the start stay in flight; released, they equal the pointer forms.  Empty blocks are ready at once."""
    m = re.search(r"parity: (\d+) cases, (\d+) pieces", run(san, "parity").stdout)
    assert m and int(m.group(1)) == 8 and int(m.group(2)) >= 1 + 7 * 4


@pytest.mark.parametrize("san", SANS)
def test_third_upload_free_in_flight_and_destroy_in_flight(san):
    assert "limits: ok" in run(san, "limits").stdout


@pytest.mark.parametrize("san", SANS)
def test_watchdog_expiry_of_an_upload_kills_the_context(san):
    assert "watchdog: ok" in run(san, "watchdog").stdout


@pytest.mark.parametrize("san", SANS)
def test_every_hip_call_of_a_start_and_of_its_pieces_fails_in_turn(san):
    """no leak; a failed start makes no block; tickets of a failed upload fail with BSW_E_HIP and launch nothing that reads the
    block; a pointer-form ticket and a clean rerun succeed afterwards unless the watchdog killed the context"""
    m = re.search(r"faults: C = (\d+), swept (\d+), dead (\d+), refused (\d+), failed uploads (\d+)", run(san, "faults").stdout)
    assert m and int(m.group(2)) * 10 >= int(m.group(1)) * 9 and int(m.group(1)) > 60 and int(m.group(4)) >= 3 and int(m.group(5)) >= 5


@pytest.mark.parametrize("san", SANS)
def test_start_test_wait_and_submit_from_nine_threads(san):
    m = re.search(r"threads: ok, (\d+) rounds", run(san, "threads").stdout)
    assert m and int(m.group(1)) == 27
