"""The mate-rescue job (bsw_rescue_ref_start / _reads_start / _test / _finish) on the host-memory HIP stand-in
(tests/hip_double/host_rescue.cpp, built by the row this module adds to the table of tests/_host_double_build.py): plain, under
ASan + UBSan and under TSan.  The program is stand-alone and run directly; no GPU is opened and nothing is loaded into Python under
a sanitizer.  Every run has a time limit: a job that hangs is a failure."""
import functools
import re

import pytest

import _host_double_build as B

B.TABLE.setdefault("host_rescue", (["bsw_rescue_job", "bsw_rescue.c", "bsw_sdp.c", "bsw_reads"], [], B.PACK))

LIMIT = 900
SANS = ["plain", "asan", "tsan"]
run = functools.partial(B.run, "host_rescue", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_both_forms_on_one_two_and_three_devices(san):
    out = run(san, "forms").stdout
    m = re.search(r"forms: (\d+) contexts", out)
    assert m and int(m.group(1)) == 3 and "forms ok" in out, out


@pytest.mark.parametrize("san", SANS)
def test_two_multi_round_jobs_beside_a_cigar_and_an_extension_ticket(san):
    assert "mixed ok" in run(san, "mixed").stdout


@pytest.mark.parametrize("san", SANS)
def test_a_follow_up_round_that_finds_no_place(san):
    assert "busy ok" in run(san, "busy").stdout


@pytest.mark.parametrize("san", SANS)
def test_every_single_hip_failure(san):
    out = run(san, "faults").stdout
    m = re.search(r"faults: injection points visited = (\d+), a job failed (\d+) times", out)
    assert m and int(m.group(1)) >= 40 and int(m.group(2)) >= 30, out
