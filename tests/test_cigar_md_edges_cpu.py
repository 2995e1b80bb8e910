"""CPU side of the NM / MD kernel's edge cases (tests/_md_cases.py; the GPU side is test_gpu_cigar_md_edges.py).

1. The reference's answer to every planted case really shows the feature the case is there for: a GPU test that compares with
   these answers cannot pass without the kernel having walked that edge.
2. rebuild() restores the target from the read, the CIGAR and the MD alone, for every planted case and for 300 random reads
   per strand: that pins _gencigar_ref.md_nm by the definition of MD, not by a second reading of bwa's loop."""
import re

import numpy as np
import pytest

import _md_cases as mc

STRANDS = [0, 1]


def by_name(oracle, strand, ts=False):
    return {name: (s, w) for (name, s), w in zip(mc.cases(strand, ts), mc.answers(oracle, strand, ts))}


def test_every_case_lies_on_its_strand_and_has_an_answer(oracle):
    for strand in STRANDS:
        for ts in (False, True):
            got = by_name(oracle, strand, ts)
            assert len(got) == len(mc.cases(strand, ts))                       # no name twice
            for name, (s, w) in got.items():
                assert (s["rb"] >= mc.L_PAC) == bool(strand) and w["status"] == 0, name
    assert [n for n, _ in mc.cases(0)] == [n for n, _ in mc.cases(1)]


@pytest.mark.parametrize("strand", STRANDS)
def test_sparse_long_m(oracle, strand):
    c = by_name(oracle, strand)
    _, w = c["a"]
    runs = mc.md_runs(w["md"])
    assert (w["cigar"], w["nm"], runs) == ([(0, 8191)], 12, mc.A_RUNS)
    assert max(runs) >= 1000 and 2046 in runs and 1000 in runs                 # 4-digit runs: steps skipped and resumed
    assert runs[0] == 0 and runs[-1] == 0                                      # a leading 0X, a trailing X0
    assert runs[3:5] == [313, 0] and runs[5:7] == [686, 0]                     # 335|336 a lane boundary, 1023|1024 a step boundary
    assert re.fullmatch(r"0[ACGT]9[ACGT]10[ACGT]313[ACGT]0[ACGT]686[ACGT]0[ACGT]100[ACGT]2046[ACGT]1827[ACGT]1000[ACGT]2188[ACGT]0",
                        w["md"])
    s, w = c["a_n"]
    assert (s["read"] == 4).sum() == 2
    assert (w["cigar"], w["nm"]) == ([(0, 8191)], 13)                          # the N at a match position is one more edit
    assert mc.md_runs(w["md"]) == mc.A_RUNS[:8] + [874, 1171] + mc.A_RUNS[9:]


@pytest.mark.parametrize("strand", STRANDS)
def test_digit_transitions(oracle, strand):
    _, w = by_name(oracle, strand)["b"]
    assert (w["cigar"], w["nm"]) == ([(0, 4000)], 6)
    assert mc.md_runs(w["md"]) == mc.B_RUNS + [1777]


@pytest.mark.parametrize("strand", STRANDS)
def test_m_lengths_at_nibble_and_step_edges(oracle, strand):
    c = by_name(oracle, strand)
    for ln in mc.C_LENS:
        _, w = c["c%d" % ln]
        assert w["cigar"] == [(0, ln)], ln
        assert (w["nm"], mc.md_runs(w["md"])) == ((2, [0, ln - 2, 0]) if ln > 1 else (1, [0, 0])), (ln, w["md"])
        _, w = c["c%d_last" % ln]
        assert (w["cigar"], w["nm"], mc.md_runs(w["md"])) == ([(0, ln)], 1, [ln - 1, 0]), (ln, w["md"])


@pytest.mark.parametrize("strand", STRANDS)
def test_interior_deletions(oracle, strand):
    c = by_name(oracle, strand)
    for d in mc.D_LENS:
        for name, extra in (("d%d" % d, 0),) + ((("d64_n", 1),) if d == 64 else ()):
            s, w = c[name]
            cig = w["cigar"]
            assert [op for op, _ in cig] == [0, 2, 0] and cig[1][1] == d, (name, cig)      # one D of d, strictly inside
            assert abs(cig[0][1] - mc.D_FLANK) <= 3 and cig[0][1] + cig[2][1] == 2 * mc.D_FLANK, (name, cig)
            assert len(re.findall(r"\^", w["md"])) == 1 and re.search(r"\d\^[ACGT]{%d}\d" % d, w["md"]), name
            assert w["nm"] == d + 2 + extra, name
            assert w["band"] == max(100, d + 3)                                # bwa's formula widens the band by itself
            assert (s["read"] == 4).sum() == 2 * extra


@pytest.mark.parametrize("strand", STRANDS)
def test_dense_steps_through_the_no_gap_shortcut(oracle, strand):
    c = by_name(oracle, strand)
    for ln in mc.E_LENS:
        for name, tries in (("e%d" % ln, 1), ("e%d_retry" % ln, 2)):
            _, w = c[name]
            assert (w["cigar"], w["band"], w["tries"], w["nm"]) == ([(0, ln)], None, tries, ln), name
            assert len(w["md"]) >= 2 * ln and set(mc.md_runs(w["md"])) == {0}, name
    for lo in (3072, 3000):
        _, w = c["e_clean%d" % lo]
        assert (w["cigar"], w["band"], w["nm"]) == ([(0, 8191)], None, 8191 - 1024)
        runs = mc.md_runs(w["md"])
        assert runs[lo] == 1024 and set(runs[:lo] + runs[lo + 1:]) == {0}      # the token at M index lo + 1 024 has 4 digits
        assert len(w["md"]) >= 2 * (8191 - 1024)
    s, w = by_name(oracle, strand, ts=True)["e1025_ts"]
    cell = mc.aligned(mc.genome_pac(), s["rb"], s["re"]).astype(int) * 5 + (s["read"][::-1] if strand else s["read"])
    ts, flat = int(mc.MAT_TS[cell].astype(int).sum()), int(mc.MAT[cell].astype(int).sum())
    assert (w["band"], w["score"]) == (None, ts) and ts != flat                 # the score depends on which bases meet


@pytest.mark.parametrize("strand", STRANDS)
def test_op_order(oracle, strand):
    c = by_name(oracle, strand)
    _, w = c["f_ins"]
    assert (w["cigar"], w["nm"], w["md"]) == ([(1, 7), (0, 300), (1, 5)], 12, "300")
    _, w = c["f_piece"]
    assert (w["cigar"], w["nm"], w["md"]) == ([(2, 20), (0, 260), (2, 20)], 0, "260")     # a leading and a trailing D
    _, w = c["f_two_del"]
    assert [op for op, _ in w["cigar"]] == [0, 2, 0, 2, 0] and [n for op, n in w["cigar"] if op == 2] == [10, 15], w["cigar"]
    assert w["nm"] == 25 and re.fullmatch(r"\d+\^[ACGT]{10}\d+\^[ACGT]{15}\d+", w["md"]), w["md"]
    _, w = by_name(oracle, strand, ts=True)["f_subdel"]
    assert w["cigar"] == [(0, 150), (2, 20), (0, 150)] and w["nm"] == 22
    assert "0^" in w["md"] and re.fullmatch(r"40[ACGT]108[ACGT]0\^[ACGT]{20}150", w["md"]), w["md"]


def test_rebuild_refuses_a_wrong_md():
    read = np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)
    got, edits = mc.rebuild(read, [(0, 3), (2, 2), (0, 3)], "1G1^TT0A2", False)
    assert (got.tolist(), edits) == ([0, 2, 2, 3, 3, 0, 0, 1], 4)
    got, edits = mc.rebuild(read, [(2, 1), (0, 2), (1, 2), (0, 2), (2, 3)], "3A0", True)     # reversed read 1 0 3 2 1 0
    assert (got.tolist(), edits) == ([1, 0, 1, 3], 3)
    for cigar, md in (([(0, 6)], "5"), ([(0, 6)], "7"), ([(0, 6)], "2G3"), ([(0, 3), (2, 2), (0, 3)], "3^T3"),
                      ([(0, 3), (2, 2), (0, 3)], "4^TT2"), ([(0, 3), (2, 2), (0, 3)], "6"), ([(0, 6)], "3^TT3"), ([(0, 6)], "6A")):
        with pytest.raises((AssertionError, IndexError)):
            mc.rebuild(read, cigar, md, False)


@pytest.mark.parametrize("strand", STRANDS)
def test_md_rebuilds_the_target_on_every_planted_case(oracle, strand):
    n = 0
    for ts in (False, True):
        for (name, s), w in zip(mc.cases(strand, ts), mc.answers(oracle, strand, ts)):
            mc.check_rebuild(s, w["cigar"], w["md"], w["nm"])
            n += 1
    assert n == len(mc.cases(strand)) + len(mc.cases(strand, True))


@pytest.mark.parametrize("strand", STRANDS)
def test_md_rebuilds_the_target_on_random_reads(oracle, strand):
    specs = mc.random_reads(strand, 300)
    want = mc.reference(oracle, specs)
    assert len(want) == 300
    for s, w in zip(specs, want):
        assert w["status"] == 0
        mc.check_rebuild(s, w["cigar"], w["md"], w["nm"])
    assert sum(w["md"].count("^") for w in want) > 50 and sum(1 for w in want for op, _ in w["cigar"] if op == 1) > 50
    assert any((s["read"] == 4).any() for s in specs)
