"""The word function of the read-block upload under its three encodings (csrc/bsw_reads_pack.h: bsw_rdpack_word_enc, what
bsw_reads_pack_kernel computes per lane), compiled by g++ with ASan + UBSan into a stand-alone program
(tests/reads_pack_enc_model.cpp) and checked against per-base loops that restate the contract: codes and FASTQ letters at every
start phase 0 - 15, 4-bit words on both halves of a 16-byte line, lengths 1 - 40, 255, 256 and 257, all 256 byte values and all 16
nibble values, non-zero garbage behind every read, a buffer that carries exactly the documented slack, and encoding 0 equal to
bsw_rdpack_word."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "reads_pack_enc_model.cpp")


def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-o", exe, SRC])
    return exe


def _words(out):
    m = re.match(r"ok (\d+) (\d+) (\d+) words", out)
    assert m, out
    return [int(g) for g in m.groups()]


def test_three_encodings_against_per_base_loops_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "reads_pack_enc_model_san")
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    codes, letters, words = _words(r.stdout)
    # 43 lengths, three layouts, 16 phases (2 for words, four layouts): at least two words each
    assert codes == letters and codes > 43 * 3 * 16 * 2 and words > 43 * 4 * 2 * 2


def test_three_encodings_optimised(tmp_path):
    """the same program as the compiler builds it for speed (the kernel's host twin): -O3, no sanitizer"""
    exe = _build(tmp_path, ["-O3"], "reads_pack_enc_model_o3")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    _words(r.stdout)


def test_record_keeps_its_size_and_carries_the_encoding():
    text = open(os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_reads_pack.h")).read()
    rec = text[text.index("typedef struct bsw_rdpack_rec {"):text.index("} bsw_rdpack_rec;")]
    assert re.findall(r"\b(?:u?int32_t)\s+([^;]+);", rec) == ["raw_off, woff", "len", "enc"]
    head = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    for name, value in (("CODES", 0), ("ASCII", 1), ("PACKED", 2)):
        assert re.search(r"#define BSW_READS_%s\s+%d\b" % (name, value), head)
        assert re.search(r"#define BSW_RDPACK_%s\s+%du\b" % (name, value), text)
