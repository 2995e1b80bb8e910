"""CPU checks of bwa_gen_cigar2 on the resident reference (bsw_cigar_ref_batch): known answers of the restatement in
tests/_gencigar_ref.py (what the GPU tests compare against), bsw_infer_bw, the ABI of bsw_ctask / bsw_cresult, and a build
audit of the NM / MD kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _gencigar_ref as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_cigar_kernel.hip")
CODE = {c: i for i, c in enumerate("ACGTN")}
PEN = (6, 1, 6, 1)
A_MIN = -(1 << 31)

# three 10-base segments, l_pac = 30 (not a multiple of 4)
SEG1, SEG2, SEG3 = "GTTACAGTCA", "GTTACGGTCA", "CATGCATTGC"
GENOME = SEG1 + SEG2 + SEG3
L_PAC = len(GENOME)


def enc(s):
    return np.array([CODE[c] for c in s], dtype=np.uint8)


@pytest.fixture(scope="module")
def pac():
    return gc.pack_pac(enc(GENOME))


@pytest.fixture(scope="module")
def mat(host):
    return host.bwa_matrix()


def run(oracle, mat, pac, read, rb, re, w=100, **kw):
    return gc.reg2aln(oracle, mat, PEN, L_PAC, pac, enc(read), rb, re, w, **kw)


def test_fetch_matches_the_genome_on_both_strands(pac):
    assert "".join("ACGT"[b] for b in gc.bns_get_seq(pac, L_PAC, 10, 20)) == SEG2
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rc = "".join(comp[c] for c in reversed(GENOME))
    assert "".join("ACGT"[b] for b in gc.bns_get_seq(pac, L_PAC, 40, 50)) == rc[10:20] == "TGACCGTAAC"
    assert len(gc.bns_get_seq(pac, L_PAC, 25, 35)) == 0


def test_one_mismatch(oracle, mat, pac):
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10)
    assert (r["status"], r["cigar"], r["nm"], r["md"], r["score"]) == (0, [(0, 10)], 1, "5A4", 5)


def test_interior_deletion(oracle, mat, pac):
    r = run(oracle, mat, pac, "GTTGGTCA", 10, 20)
    assert (r["cigar"], r["nm"], r["md"], r["score"]) == ([(0, 3), (2, 2), (0, 5)], 2, "3^AC5", 0)


def test_leading_and_trailing_deletion_are_not_in_md_or_nm(oracle, mat, pac):
    r = run(oracle, mat, pac, "TGCATT", 20, 30)
    assert (r["cigar"], r["nm"], r["md"], r["score"]) == ([(2, 2), (0, 6), (2, 2)], 0, "6", -10)


def test_insertion_counts_in_nm_only(oracle, mat, pac):
    r = run(oracle, mat, pac, "GTTAGCGGTCA", 10, 20)
    assert (r["cigar"], r["nm"], r["md"]) == ([(0, 4), (1, 1), (0, 6)], 1, "10")


def test_reverse_strand_complements_letters_in_the_reversed_frame(oracle, mat, pac):
    # [40, 50) is revcomp(SEG2) = TGACCGTAAC; bwa aligns reverse(read) to reverse(rseq) = CAATGCCAGT
    r = run(oracle, mat, pac, "TGGCCGTAAC", 40, 50)          # A -> G at read position 2 = reversed position 7
    assert (r["cigar"], r["nm"], r["md"]) == ([(0, 10)], 1, "7T2")
    r = run(oracle, mat, pac, "TCCGTAAC", 40, 50)            # GA deleted at read position 1: near the END once reversed
    assert (r["cigar"], r["nm"], r["md"]) == ([(0, 7), (2, 2), (0, 1)], 2, "7^TC1")


def test_query_n_is_a_mismatch(oracle, mat, pac):
    r = run(oracle, mat, pac, "GTTACNGTCA", 0, 10)
    assert (r["cigar"], r["nm"], r["md"], r["score"]) == ([(0, 10)], 1, "5A4", 8)


def test_no_gap_shortcut(oracle, mat, pac):
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10, w=0)
    assert (r["band"], r["cigar"], r["score"], r["md"], r["tries"], r["w"]) == (None, [(0, 10)], 5, "5A4", 1, 0)
    r = run(oracle, mat, pac, "GTTGGTCA", 10, 20, w=0)       # unequal lengths: DP with band |10 - 8| + 3
    assert (r["band"], r["cigar"], r["md"]) == (5, [(0, 3), (2, 2), (0, 5)], "3^AC5")
    # w_ = 0 below w_cap: a second try with the same band returns the same score and ends the loop
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10, w=0, w_cap=8, min_score=100, max_tries=3)
    assert (r["tries"], r["w"], r["runs"]) == (2, 0, [0, 0])


@pytest.mark.parametrize("read,rb,re", [("", 0, 10), ("ACGT", 10, 10), ("ACGT", 12, 10), ("ACGT", 25, 35),
                                         ("ACGT", 55, 61), ("ACGT", -2, 8)])
def test_status_cases(oracle, mat, pac, read, rb, re):
    r = run(oracle, mat, pac, read, rb, re)
    assert r["status"] == 1 and r["tries"] == 1


def test_band_formula_at_hand_computed_points(mat):
    # l_query 150, rlen 152, a 1, o 6, e 1: max_gap = (75 - 6) / 1 + 1 = 70, w = (70 + 2 + 1) >> 1 = 36
    assert gc.band(mat, 6, 1, 6, 1, 150, 152, 100) == 36
    assert gc.band(mat, 6, 1, 6, 1, 150, 152, 20) == 20
    # l_query 10, rlen 8, w_ 0: min(.., 0) = 0, raised to |8 - 10| + 3 = 5
    assert gc.band(mat, 6, 1, 6, 1, 10, 8, 0) == 5
    # o_del 5 e_del 2 vs o_ins 7 e_ins 1 at l_query 101: max_del = (51 - 5) / 2 + 1 = 24, max_ins = (51 - 7) / 1 + 1 = 45
    assert gc.band(mat, 5, 2, 7, 1, 101, 101, 1000) == (45 + 0 + 1) >> 1 == 23


def test_retry_loop_cases(oracle, mat, pac):
    # a stop on an equal score: a 10-base read's band is |rlen - l_query| + 3 = 3 whatever w_ >= 1 is
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10, w=1, w_cap=64, min_score=100, max_tries=3)
    assert (r["runs"], r["tries"], r["w"], r["band"]) == ([1, 2], 2, 2, 3)
    # a stop at w_cap
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10, w=2, w_cap=3, min_score=100, max_tries=3)
    assert r["runs"] == [2, 3] and r["w"] == 3
    # min_score reached on the first try
    r = run(oracle, mat, pac, "GTTACTGTCA", 0, 10, w=1, w_cap=64, min_score=0, max_tries=3)
    assert r["tries"] == 1


def test_infer_bw_matches_the_restatement(host):
    rng = np.random.default_rng(5)
    for _ in range(3000):
        l1, l2 = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        if rng.random() < 0.3:
            l2 = l1
        a, q, r = int(rng.integers(1, 3)), int(rng.integers(0, 12)), int(rng.integers(1, 4))
        score = int(rng.integers(-50, min(l1, l2) * a + 1))
        assert host.infer_bw(l1, l2, score, a, q, r) == gc.infer_bw(l1, l2, score, a, q, r), (l1, l2, score, a, q, r)
    assert gc.infer_bw(150, 150, 150, 1, 6, 1) == 0
    assert gc.infer_bw(150, 150, 130, 1, 6, 1) == int((150 - 130 - 6) / 1 + 2.) == 16
    assert gc.infer_bw(100, 120, 90, 1, 6, 1) == 20


def test_ctask_and_cresult_layout_match_the_header(host, tmp_path):
    fields = [("bsw_ctask", host.CTASK), ("bsw_cresult", host.CRESULT)]
    body = []
    for name, dt in fields:
        body.append('printf("%%zu\\n", sizeof(%s));' % name)
        for f in dt.names:
            body.append('printf("%%zu\\n", offsetof(%s, %s));' % (name, f))
    src = tmp_path / "lay.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bwa_sw_mi355.h"\nint main(void){%s return 0;}\n' % "".join(body))
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, dt in fields:
        want.append(dt.itemsize)
        want.extend(dt.fields[f][1] for f in dt.names)
    assert got == want


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_md_kernel_builds_for_gfx950_without_scratch():
    out = subprocess.check_output(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function",
                                   "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", KERNEL, "-o", "-"],
                                  stderr=subprocess.DEVNULL, text=True)
    assert "bsw_cigar_md_kernel" in out
    sizes = [int(x) for x in re.findall(r"ScratchSize: (\d+)", out)]
    assert sizes and all(x == 0 for x in sizes), sizes
    spills = [int(x) for x in re.findall(r"\.(?:s|v)gpr_spill_count:\s+(\d+)", out)]
    assert spills and all(x == 0 for x in spills), spills
