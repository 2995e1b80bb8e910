"""The hosts of ksw_align2's long-query route (bsw_set_align_long) on the host-memory HIP stand-in (tests/hip_double/), under ASan +
UBSan and under TSan, as stand-alone programs.  No GPU is opened.

tests/hip_double/host_align_long.cpp is built by its row in tests/_host_double_build.py: the objects of the other host-double programs,
the unit that owns the switch, and a stand-in for launch_align_long that computes with oracle/ksw_align_ref.c and dies when a task is
listed for a class that is not its own (the stand-in of launch_align dies when a task of more than 1 024 bases reaches it).  Expected
values: the oracle on the caller's bytes.  Every run has a time limit."""
import functools
import re

import pytest

import _host_double_build as B

LIMIT = 900
SANS = ["asan", "tsan"]
run = functools.partial(B.run, "host_align_long", limit=LIMIT, env={"BSW_ALIGN_LONG": None})


@pytest.mark.parametrize("san", SANS)
def test_mode_0_refuses_modes_1_and_2_accept(san):
    """bsw_align_batch, ksw_align2 / ksw_align and bsw_matesw_ref_batch; 8 192 bases are refused under every mode; under mode 1 the
    long stand-in sees exactly the long tasks, under mode 2 every task"""
    m = re.search(r"gate: ok, (\d+) launches", run(san, "gate").stdout)
    assert m and int(m.group(1)) >= 8


@pytest.mark.parametrize("san", SANS)
def test_sub_batch_split_with_long_tasks(san):
    m = re.search(r"split: ok, (\d+) sub-batches", run(san, "split").stdout)
    assert m and int(m.group(1)) >= 2


@pytest.mark.parametrize("san", SANS)
def test_ticket_whose_mode_is_flipped_before_its_chunks_are_processed(san):
    """twelve one-task chunks behind stalled streams, the switch back at 0 before ten of them are looked at: every task still goes
    to the long launcher (mode 1: long mates; mode 2: short ones)"""
    m = re.search(r"flip: ok, (\d+) chunks", run(san, "flip").stdout)
    assert m and int(m.group(1)) == 24


@pytest.mark.parametrize("san", SANS)
def test_every_hip_call_of_a_batch_with_long_tasks_fails_in_turn(san):
    m = re.search(r"faults: C = (\d+), visited (\d+), failed (\d+), ignored (\d+), long launches failed (\d+)", run(san, "faults").stdout)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) > 40 and int(m.group(5)) >= 8


@pytest.mark.parametrize("san", SANS)
def test_batch_without_long_tasks_makes_the_same_calls_as_with_the_switch_off(san):
    m = re.search(r"sequence: ok, (\d+) calls", run(san, "sequence").stdout)
    assert m and int(m.group(1)) > 10
