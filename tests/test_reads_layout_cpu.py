"""Resident read blocks, the parts that need no GPU: the three task records of include/bwa_sw_mi355.h against the dtypes of
host.py (sizes 48 / 32 / 48, field offsets taken from the header by the C compiler), the ABI number, and the exports."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bsw_reads_upload", "bsw_reads_free", "bsw_reads_info", "bsw_submit_reads_t", "bsw_matesw_reads_submit_t",
       "bsw_cigar_reads_submit_t"]
FIELDS = {
    "bsw_rd_task": ["read", "init_score", "seed", "rmax0", "rmax1", "tag", "_pad"],
    "bsw_rd_mtask": ["read", "is_rev", "rb", "re", "xtra", "min_score"],
    "bsw_rd_ctask": ["read", "qb", "qe", "w", "rb", "re", "w_cap", "min_score", "max_tries", "_pad"],
}


def header_layout(tmp_path):
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "bwa_sw_mi355.h"', 'int main(void) {']
    for st, fs in FIELDS.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (st, st))
        for f in fs:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    src += ['printf("abi %d\\n", BSW_ABI_VERSION);', 'return 0; }']
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write("\n".join(src))
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    out = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        a = line.split()
        out[tuple(a[:-1])] = int(a[-1])
    return out


def test_task_records_match_the_header(host, tmp_path):
    lay = header_layout(tmp_path)
    assert lay[("abi",)] == 6
    for st, dt, size in (("bsw_rd_task", host.RD_TASK, 48), ("bsw_rd_mtask", host.RD_MTASK, 32), ("bsw_rd_ctask", host.RD_CTASK, 48)):
        assert lay[(st, "size")] == size == dt.itemsize
        assert list(dt.names) == FIELDS[st]
        for f in FIELDS[st]:
            assert dt.fields[f][1] == lay[(st, f)], (st, f)


def test_every_new_function_is_exported_and_bound(built, host):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    exported = set(re.findall(r" T (\w+)", syms))
    for name in NEW:
        assert name in exported and name in host.EXPORTS
        assert getattr(host.lib(), name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header)
    assert "#define BSW_ABI_VERSION 6" in header
