"""The upload encodings of a resident read block on the host-memory HIP stand-in (tests/hip_double/), under ASan + UBSan and under
TSan, as stand-alone programs: bsw_reads_upload_enc and bsw_reads_upload_start_enc with codes, FASTQ letters and 4-bit words.  No
GPU is opened.

tests/hip_double/host_reads_enc.cpp is built by tests/_reads_enc_double_build.py with a stand-in for launch_reads_pack that
restates the word function per base and honours every record's encoding (launchers_reads_pack_enc.cpp).  Expected value: the
image bsw_reads_upload makes of the codes the input spells.  Every run has a time limit."""
import os
import re
import subprocess

import pytest

import _host_double_build as B
import _reads_enc_double_build as E

LIMIT = 600
SANS = ["asan", "tsan"]


def run(san, mode):
    exe = E.program(san)
    log = os.path.join(os.path.dirname(exe), "san_reads_enc_%s" % mode)
    e = B.env(san)
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log
    try:
        out = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired as ex:
        raise AssertionError("host_reads_enc %s (%s) hit the time limit of %d s; last output: %r" % (mode, san, LIMIT, (ex.stdout or b"")[-600:]))
    reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            reports += open(os.path.join(d, f)).read()[-6000:]
    assert out.returncode == 0 and not reports, (mode, san, out.returncode, out.stdout[-1500:], out.stderr[-4000:], reports[-6000:])
    return out.stdout


@pytest.mark.parametrize("san", SANS)
def test_images_of_three_encodings_direct_and_gathered_on_one_and_two_copies(san):
    """every copy's image of the _start_enc upload equals bsw_reads_upload_enc's and bsw_reads_upload's of the equivalent codes;
    4 KiB pieces; on the gather path h2d_bytes grows per device by the raw bytes + 16 per read, exactly"""
    m = re.search(r"parity: (\d+) cases, (\d+) pieces", run(san, "parity"))
    assert m and int(m.group(1)) == 2 * 3 * 2 and int(m.group(2)) >= 2 * int(m.group(1))


@pytest.mark.parametrize("san", SANS)
def test_refusals_allocate_and_launch_nothing(san):
    """unknown encoding, a packed read off its boundary, the existing per-read checks under every encoding, for both calls"""
    m = re.search(r"refusals: ok, (\d+)", run(san, "refusals"))
    assert m and int(m.group(1)) == 2 * (3 + 5 + 3 * 4)


@pytest.mark.parametrize("san", SANS)
def test_first_hip_failure_of_each_call_kind_under_every_encoding(san):
    m = re.search(r"faults: ok, (\d+)", run(san, "faults"))
    assert m and int(m.group(1)) == 3 * (5 * 2 + 4 * 2)
