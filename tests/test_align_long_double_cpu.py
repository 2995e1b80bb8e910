"""The hosts of ksw_align2's long-query route (bsw_set_align_long) on the host-memory HIP stand-in (tests/hip_double/), under ASan +
UBSan and under TSan, as stand-alone programs.  No GPU is opened.

tests/hip_double/host_align_long.cpp is built by tests/_align_long_double_build.py: the objects of the other host-double programs,
the unit that owns the switch, and a stand-in for launch_align_long that computes with oracle/ksw_align_ref.c and dies when a task is
listed for a class that is not its own (the stand-in of launch_align dies when a task of more than 1 024 bases reaches it).  Expected
values: the oracle on the caller's bytes.  Every run has a time limit."""
import os
import re
import subprocess

import pytest

import _align_long_double_build as A
import _host_double_build as B

LIMIT = 900
SANS = ["asan", "tsan"]


def run(san, mode):
    exe = A.program(san)
    log = os.path.join(os.path.dirname(exe), "san_align_long_%s" % mode)
    e = B.env(san)
    e.pop("BSW_ALIGN_LONG", None)
    for k in ("ASAN_OPTIONS", "TSAN_OPTIONS", "UBSAN_OPTIONS"):
        e[k] += ":log_path=" + log
    try:
        out = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired as ex:
        raise AssertionError("host_align_long %s (%s) hit the time limit of %d s; last output: %r" % (mode, san, LIMIT, (ex.stdout or b"")[-600:]))
    reports = ""
    d = os.path.dirname(log)
    for f in sorted(os.listdir(d)):
        if f.startswith(os.path.basename(log) + "."):
            reports += open(os.path.join(d, f)).read()[-6000:]
    assert out.returncode == 0 and not reports, (mode, san, out.returncode, out.stdout[-1500:], out.stderr[-4000:], reports[-6000:])
    return out.stdout


@pytest.mark.parametrize("san", SANS)
def test_mode_0_refuses_modes_1_and_2_accept(san):
    """bsw_align_batch, ksw_align2 / ksw_align and bsw_matesw_ref_batch; 8 192 bases are refused under every mode; under mode 1 the
    long stand-in sees exactly the long tasks, under mode 2 every task"""
    m = re.search(r"gate: ok, (\d+) launches", run(san, "gate"))
    assert m and int(m.group(1)) >= 8


@pytest.mark.parametrize("san", SANS)
def test_sub_batch_split_with_long_tasks(san):
    m = re.search(r"split: ok, (\d+) sub-batches", run(san, "split"))
    assert m and int(m.group(1)) >= 2


@pytest.mark.parametrize("san", SANS)
def test_ticket_whose_mode_is_flipped_before_its_chunks_are_processed(san):
    """twelve one-task chunks behind stalled streams, the switch back at 0 before ten of them are looked at: every task still goes
    to the long launcher (mode 1: long mates; mode 2: short ones)"""
    m = re.search(r"flip: ok, (\d+) chunks", run(san, "flip"))
    assert m and int(m.group(1)) == 24


@pytest.mark.parametrize("san", SANS)
def test_every_hip_call_of_a_batch_with_long_tasks_fails_in_turn(san):
    m = re.search(r"faults: C = (\d+), visited (\d+), failed (\d+), ignored (\d+), long launches failed (\d+)", run(san, "faults"))
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) > 40 and int(m.group(5)) >= 8


@pytest.mark.parametrize("san", SANS)
def test_batch_without_long_tasks_makes_the_same_calls_as_with_the_switch_off(san):
    m = re.search(r"sequence: ok, (\d+) calls", run(san, "sequence"))
    assert m and int(m.group(1)) > 10
