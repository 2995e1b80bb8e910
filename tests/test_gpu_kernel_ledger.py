"""The kernel ledger on the GPU: every group of tests/_kernel_ledger.py (one set of routing switches, read once per process) runs
in a child process of its own under `rocprofv3 --kernel-trace`, one after the other.  The child compares every result of every
case with its reference, bit for bit (tests/_kernel_ledger_run.py); here the traces prove that each group dispatched every
kernel its cases name, and that the groups together dispatched every compiled kernel but those in UNREACHED."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import pytest

import _kernel_ledger as L
from test_kernel_ledger_cpu import compiled_kernels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "tests", "_kernel_ledger_run.py")


def rocprofv3():
    exe = shutil.which("rocprofv3")
    if exe is None and os.path.exists("/opt/rocm/bin/rocprofv3"):
        exe = "/opt/rocm/bin/rocprofv3"
    return exe


def switch_free_env():
    """the environment without any switch a ledger case (or a routing test) sets"""
    drop = set(k for c in L.CASES for k in c["env"]) | {"BSW_NARROW_SHARE", "BSW_NO_NARROW", "BSW_NO_LANE2", "BSW_FORK", "BSW_NO_FOLD",
                                                         "BSW_GLOBAL_LONG", "BSW_CHAIN_SELFTEST", "BSW_NO_WAVE_FORK", "BSW_NO_SMALL"}
    return {k: v for k, v in os.environ.items() if k not in drop}


def traced_kernels(outdir):
    names = {}
    files = glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under %s" % outdir
    for fn in files:
        with open(fn, newline="") as f:
            for row in csv.DictReader(f):
                k = L.normalise(row["Kernel_Name"])
                names[k] = names.get(k, 0) + 1
    return names


def test_every_compiled_kernel_is_dispatched_and_bit_exact(built, tmp_path):
    exe = rocprofv3()
    if exe is None:
        pytest.skip("rocprofv3 is not installed")
    build = compiled_kernels(built.lib_path())
    union = set()
    lines = []
    for g, cases in L.groups().items():
        env = switch_free_env()
        for c in cases:
            env.update(c["env"])
        out = str(tmp_path / g)
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, RUNNER, "--group", g]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        tail = r.stdout[-3000:] + r.stderr[-4000:]
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), "group %s: rc %s\n%s" % (g, r.returncode, tail)
        seen = traced_kernels(out)
        union |= set(seen)
        checked = {}
        for ln in r.stdout.splitlines():
            if ln.startswith("case "):
                f = ln.split()
                checked[f[1]] = int(f[3])
        for c in cases:
            assert c["name"] in checked, "group %s: case %s did not report\n%s" % (g, c["name"], tail)
            missing = [t for t in c["targets"] if t not in seen]
            assert not missing, "group %s, case %s: not dispatched: %s\n%s" % (g, c["name"], missing, tail)
            for t in c["targets"]:
                lines.append("%-62s %-34s %6d seeds  (%d launches in group %s)" % (t, c["name"], checked[c["name"]], seen[t], g))
    print("\n".join(sorted(lines)))
    want = build - set(L.UNREACHED)
    assert not (want - union), "compiled kernels no group dispatched: %s" % sorted(want - union)
    print("compiled %d, dispatched %d, unreached %d" % (len(build), len(union & build), len(L.UNREACHED)))
