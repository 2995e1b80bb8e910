"""The mem_sort_dedup_patch job (bsw_sdp_ref_start / _reads_start / _test / _finish) on the host-memory HIP stand-in
(tests/hip_double/host_sdp.cpp, built by tests/_sdp_double_build.py): plain, under ASan + UBSan and under TSan.  The program is
stand-alone and run directly; no GPU is opened and nothing is loaded into Python under a sanitizer.  Every run has a time limit:
a job that hangs is a failure."""
import os
import re
import subprocess

import pytest

import _host_double_build as B
import _sdp_double_build as SB

LIMIT = 900
SANS = ["plain", "asan", "tsan"]


def run(san, mode, **extra):
    exe = SB.program(san)
    log = os.path.join(os.path.dirname(exe), "san_sdp_%s" % mode)
    e = B.env(san, **extra)
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log
    try:
        out = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired as ex:
        raise AssertionError("host_sdp %s (%s) hit the time limit of %d s; last output: %r" % (mode, san, LIMIT, (ex.stdout or b"")[-600:]))
    reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            reports += open(os.path.join(d, f)).read()[-6000:]
    assert out.returncode == 0 and not reports, (mode, san, out.returncode, out.stdout[-1500:], out.stderr[-4000:], reports[-6000:])
    return out.stdout


@pytest.mark.parametrize("san", SANS)
def test_both_forms_on_one_two_and_three_devices(san):
    out = run(san, "forms")
    m = re.search(r"forms: (\d+) contexts", out)
    assert m and int(m.group(1)) == 3 and "forms ok" in out, out


@pytest.mark.parametrize("san", SANS)
def test_two_multi_round_jobs_beside_a_cigar_and_an_extension_ticket(san):
    assert "mixed ok" in run(san, "mixed")


@pytest.mark.parametrize("san", SANS)
def test_a_follow_up_round_that_finds_no_place(san):
    assert "busy ok" in run(san, "busy")


@pytest.mark.parametrize("san", SANS)
def test_every_single_hip_failure(san):
    out = run(san, "faults")
    m = re.search(r"faults: injection points visited = (\d+), a job failed (\d+) times", out)
    assert m and int(m.group(1)) >= 60 and int(m.group(2)) >= 50, out
