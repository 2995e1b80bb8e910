"""The word function of the asynchronous read-block upload (csrc/bsw_reads_pack.h: bsw_rdpack_word, what bsw_reads_pack_kernel
computes per lane and the host double's stand-in restates), compiled by g++ with ASan + UBSan into a stand-alone program
(tests/reads_pack_model.cpp) and checked against a byte loop: every start phase 0 - 15, lengths 0 - 49 and 65 535, byte values
0 - 255, the first and the last read of a buffer that carries exactly the documented slack, zero-length reads at the first, a
middle and the last position."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "reads_pack_model.cpp")


def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-o", exe, SRC])
    return exe


def test_word_function_against_a_byte_loop_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "reads_pack_model_san")
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok (\d+) words", r.stdout)
    assert m and int(m.group(1)) > 16 * 4 * 4097      # 16 phases x 4 layouts of the 65 535-base read alone, 4 097 words (one behind its end) each


def test_word_function_optimised(tmp_path):
    """the same program as the compiler builds it for speed (the kernel's host twin): -O3, no sanitizer"""
    exe = _build(tmp_path, ["-O3"], "reads_pack_model_o3")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_slack_is_what_the_header_documents():
    text = open(os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_reads_pack.h")).read()
    assert re.search(r"#define BSW_RDPACK_RAW_SLACK 16\b", text)
