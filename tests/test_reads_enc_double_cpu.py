"""The upload encodings of a resident read block on the host-memory HIP stand-in (tests/hip_double/), under ASan + UBSan and under
TSan, as stand-alone programs: bsw_reads_upload_enc and bsw_reads_upload_start_enc with codes, FASTQ letters and 4-bit words.  No
GPU is opened.

tests/hip_double/host_reads_enc.cpp is built by its row in tests/_host_double_build.py with a stand-in for launch_reads_pack that
restates the word function per base and honours every record's encoding (launchers_reads_pack_enc.cpp).  Expected value: the
image bsw_reads_upload makes of the codes the input spells.  Every run has a time limit."""
import functools
import re

import pytest

import _host_double_build as B

LIMIT = 600
SANS = ["asan", "tsan"]
run = functools.partial(B.run, "host_reads_enc", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_images_of_three_encodings_direct_and_gathered_on_one_and_two_copies(san):
    """every copy's image of the _start_enc upload equals bsw_reads_upload_enc's and bsw_reads_upload's of the equivalent codes;
    4 KiB pieces; on the gather path h2d_bytes grows per device by the raw bytes + 16 per read, exactly"""
    m = re.search(r"parity: (\d+) cases, (\d+) pieces", run(san, "parity").stdout)
    assert m and int(m.group(1)) == 2 * 3 * 2 and int(m.group(2)) >= 2 * int(m.group(1))


@pytest.mark.parametrize("san", SANS)
def test_refusals_allocate_and_launch_nothing(san):
    """unknown encoding, a packed read off its boundary, the existing per-read checks under every encoding, for both calls"""
    m = re.search(r"refusals: ok, (\d+)", run(san, "refusals").stdout)
    assert m and int(m.group(1)) == 2 * (3 + 5 + 3 * 4)


@pytest.mark.parametrize("san", SANS)
def test_first_hip_failure_of_each_call_kind_under_every_encoding(san):
    m = re.search(r"faults: ok, (\d+)", run(san, "faults").stdout)
    assert m and int(m.group(1)) == 3 * (5 * 2 + 4 * 2)
