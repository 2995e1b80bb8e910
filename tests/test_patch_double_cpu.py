"""bsw_patch_ref_batch and its two ticket forms on the host-memory HIP stand-in (tests/hip_double/host_patch.cpp, built by
tests/_patch_double_build.py): plain, under ASan + UBSan and under TSan.  The program is stand-alone and run directly; no GPU is
opened.  Expected values are the C oracle's ksw_global2 and a C restatement of mem_patch_reg's arithmetic inside the program.
Every run has a time limit: a ticket that hangs is a failure."""
import os
import re
import subprocess

import pytest

import _host_double_build as B
import _patch_double_build as PB

LIMIT = 900
SANS = ["plain", "asan", "tsan"]


def run(san, mode, **extra):
    exe = PB.program(san)
    log = os.path.join(os.path.dirname(exe), "san_patch_%s" % mode)
    e = B.env(san, **extra)
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log
    try:
        out = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired as ex:
        raise AssertionError("host_patch %s (%s) hit the time limit of %d s; last output: %r" % (mode, san, LIMIT, (ex.stdout or b"")[-600:]))
    reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            reports += open(os.path.join(d, f)).read()[-6000:]
    assert out.returncode == 0 and not reports, (mode, san, out.returncode, out.stdout[-1500:], out.stderr[-4000:], reports[-6000:])
    return out.stdout


@pytest.mark.parametrize("san", SANS)
def test_three_forms_against_the_oracle(san):
    assert "parity ok" in run(san, "parity")


@pytest.mark.parametrize("san", SANS)
def test_every_validation_code(san):
    assert "checks ok" in run(san, "checks")


@pytest.mark.parametrize("san", SANS)
def test_sub_batches_and_ticket_cuts(san):
    out = run(san, "cuts", BSW_F4_PATCH_WORK="300000")
    m = re.search(r"cuts: (\d+) sub-batches, (\d+) chunks of two tickets", out)
    assert m and int(m.group(1)) >= 5 and int(m.group(2)) >= 10 and "cuts ok" in out, out


@pytest.mark.parametrize("san", SANS)
def test_patch_tickets_beside_extension_and_cigar_tickets(san):
    assert "mixed ok" in run(san, "mixed")


@pytest.mark.parametrize("san", SANS)
def test_every_single_hip_failure(san):
    out = run(san, "faults")
    m = re.search(r"faults: injection points visited = (\d+), a call failed (\d+) times", out)
    assert m and int(m.group(1)) >= 60 and int(m.group(2)) >= 50, out
