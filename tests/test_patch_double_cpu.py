"""bsw_patch_ref_batch and its two ticket forms on the host-memory HIP stand-in (tests/hip_double/host_patch.cpp, built by
its row in tests/_host_double_build.py): plain, under ASan + UBSan and under TSan.  The program is stand-alone and run directly; no GPU is
opened.  Expected values are the C oracle's ksw_global2 and a C restatement of mem_patch_reg's arithmetic inside the program.
Every run has a time limit: a ticket that hangs is a failure."""
import functools
import re

import pytest

import _host_double_build as B

LIMIT = 900
SANS = ["plain", "asan", "tsan"]
run = functools.partial(B.run, "host_patch", limit=LIMIT)


@pytest.mark.parametrize("san", SANS)
def test_three_forms_against_the_oracle(san):
    assert "parity ok" in run(san, "parity").stdout


@pytest.mark.parametrize("san", SANS)
def test_every_validation_code(san):
    assert "checks ok" in run(san, "checks").stdout


@pytest.mark.parametrize("san", SANS)
def test_sub_batches_and_ticket_cuts(san):
    out = run(san, "cuts", env={"BSW_F4_PATCH_WORK": "300000"}).stdout
    m = re.search(r"cuts: (\d+) sub-batches, (\d+) chunks of two tickets", out)
    assert m and int(m.group(1)) >= 5 and int(m.group(2)) >= 10 and "cuts ok" in out, out


@pytest.mark.parametrize("san", SANS)
def test_patch_tickets_beside_extension_and_cigar_tickets(san):
    assert "mixed ok" in run(san, "mixed").stdout


@pytest.mark.parametrize("san", SANS)
def test_every_single_hip_failure(san):
    out = run(san, "faults").stdout
    m = re.search(r"faults: injection points visited = (\d+), a call failed (\d+) times", out)
    assert m and int(m.group(1)) >= 60 and int(m.group(2)) >= 50, out
