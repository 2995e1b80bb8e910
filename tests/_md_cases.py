"""Planted inputs for the edges of bsw_cigar_md_kernel (NM and MD from the final CIGAR), their reference answers and a
reference-free check of an MD string.

Every case is a read derived from the bases of [rb, re) with edits at exact places of the ALIGNED order: bwa aligns
reverse(read) to reverse(rseq) on the reverse strand, so the edits are planted on the reversed view there and both strands
bring the same M indices, lanes and steps to the kernel.  The kernel walks an M op in steps of 1 024 bases, 16 per lane, and
a deletion in steps of 2 048; the cases sit on those edges (see the builders).

Answers come from _gencigar_ref.reg2aln with the oracle's ksw_global2; nothing here calls the product library."""
import re

import numpy as np

import _gencigar_ref as gc
from test_gpu_cigar_ref import L_PAC, interval, read_of, spec

SEED = 2024
PEN = (6, 1, 6, 1)                     # o_del, e_del, o_ins, e_ins: bwa's defaults, as bsw_default_params
MAT = np.full((5, 5), -4, dtype=np.int8)
MAT[np.arange(4), np.arange(4)] = 1
MAT[4, :] = -1
MAT[:, 4] = -1
MAT = MAT.reshape(25)
# With one price for every mismatch ksw_global2 never leaves a substitution directly before a deletion: moving the deletion
# one base to the left only changes the substituted base's partner, the score stays, and the backtrack prefers the diagonal,
# so the mismatch ends up behind the deletion.  A matrix that charges transitions (A<->G, C<->T) 2 and transversions 4 makes
# "a transition, then the deletion" strictly better; the case that needs it runs in a batch of its own with this matrix.
MAT_TS = MAT.reshape(5, 5).copy()
for _a, _b in ((0, 2), (1, 3)):
    MAT_TS[_a, _b] = MAT_TS[_b, _a] = -2
MAT_TS = MAT_TS.reshape(25)

A_SUBS = (0, 10, 21, 335, 336, 1023, 1024, 1125, 3172, 5000, 6001, 8190)
A_RUNS = [0, 9, 10, 313, 0, 686, 0, 100, 2046, 1827, 1000, 2188, 0]
B_RUNS = [9, 10, 99, 100, 999, 1000]
C_LENS = (1, 15, 16, 17, 1023, 1024, 1025, 2048)
D_LENS = (63, 64, 65, 2047, 2048, 2049, 4100)
E_LENS = (1024, 1025, 8191)
D_FLANK = 350
# windows found by scanning seeded windows with the reference until it showed the feature (start offsets inside a strand)
F_PIECE_AT = {0: 226888, 1: 280961}    # a read that is an interior piece of its window: a leading AND a trailing D
F_SUBDEL_AT = {0: 141055, 1: 231121}   # a substitution directly before a deletion, "...X0^..." in MD (with MAT_TS)

_pac = []


def genome_pac():
    """the genome of test_gpu_cigar_ref.py: L_PAC seeded random bases, packed"""
    if not _pac:
        _pac.append(gc.pack_pac(np.random.default_rng(SEED).integers(0, 4, L_PAC).astype(np.uint8)))
    return _pac[0]


def aligned(pac, rb, re_):
    """the bases of [rb, re) in the order the kernel walks them"""
    rseq = gc.bns_get_seq(pac, L_PAC, rb, re_)
    return rseq[::-1].copy() if rb >= L_PAC else rseq


def as_read(rb, a):
    """a read given in aligned order, as the caller holds it"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a[::-1].copy() if rb >= L_PAC else a


def sub_at(a, idx, by=1):
    a = a.copy()
    idx = np.asarray(idx, dtype=np.int64)
    a[idx] = (a[idx] + by) & 3
    return a


def window(strand, at, rlen):
    lo = 0 if strand == 0 else L_PAC
    return lo + at, lo + at + rlen


def piece_read(pac, strand, at):
    rb, re_ = window(strand, at, 300)
    return spec(as_read(rb, aligned(pac, rb, re_)[20:280]), rb, re_, w=100)


def subdel_read(pac, strand, at):
    rb, re_ = window(strand, at, 320)
    a = aligned(pac, rb, re_)
    return spec(as_read(rb, np.concatenate([sub_at(a[:150], [40, 149], by=2), a[170:]])), rb, re_, w=100)


def dense(a):
    """every base differs from the target's, every 97th is an N"""
    i = np.arange(len(a))
    q = ((a + 1 + i % 3) % 4).astype(np.uint8)
    q[96::97] = 4
    return q


def build(pac, strand):
    """the planted cases of one strand: a list of (name, spec), in a fixed order"""
    rng = np.random.default_rng(100 + strand)
    out = []

    def add(name, a, rb, re_, **kw):
        out.append((name, spec(as_read(rb, a), rb, re_, **kw)))

    # a. a sparse long M: clean steps between mismatching ones, lane 63 then lane 0 of the next step, a 4-digit run,
    #    a leading 0X and a trailing X0.  g: an N at a match position and one at a planted substitution
    rb, re_ = interval(rng, 8191, strand)
    a = sub_at(aligned(pac, rb, re_), A_SUBS)
    add("a", a, rb, re_, w=100)
    n = a.copy()
    n[[2000, 5000]] = 4
    add("a_n", n, rb, re_, w=100)
    # b. successive match runs of 9, 10, 99, 100, 999 and 1 000 bases
    rb, re_ = interval(rng, 4000, strand)
    at, p = [], -1
    for u in B_RUNS:
        p += u + 1
        at.append(p)
    add("b", sub_at(aligned(pac, rb, re_), at), rb, re_, w=100)
    # c. M ops that end at a nibble, a lane, a step: a substitution at the first and at the last base, and at the last alone
    for ln in C_LENS:
        rb, re_ = interval(rng, ln, strand)
        add("c%d" % ln, sub_at(aligned(pac, rb, re_), [0, ln - 1] if ln > 1 else [0]), rb, re_, w=100)
        add("c%d_last" % ln, sub_at(aligned(pac, rb, re_), [ln - 1], by=2), rb, re_, w=100)
    # d. interior deletions around one store of 64 letters and around one step of 2 048; a substitution in each flank
    for d in D_LENS:
        rb, re_ = interval(rng, 2 * D_FLANK + d, strand)
        a = aligned(pac, rb, re_)
        q = sub_at(np.concatenate([a[:D_FLANK], a[D_FLANK + d:]]), [100, D_FLANK + 200])
        add("d%d" % d, q, rb, re_, w=100)
        if d == 64:
            n = q.copy()
            n[[100, 500]] = 4
            add("d64_n", n, rb, re_, w=100)
    # e. the no-gap shortcut over more than one step, every lane of every step full of mismatches
    for ln in E_LENS:
        rb, re_ = interval(rng, ln, strand)
        q = dense(aligned(pac, rb, re_))
        add("e%d" % ln, q, rb, re_, w=0, max_tries=1)
        add("e%d_retry" % ln, q, rb, re_, w=0, w_cap=50, min_score=1000, max_tries=3)
    for lo in (3072, 3000):            # a clean stretch of 1 024: a dense step starts with (or holds) a 4-digit token
        rb, re_ = interval(rng, 8191, strand)
        a = aligned(pac, rb, re_)
        q = dense(a)
        q[lo:lo + 1024] = a[lo:lo + 1024]
        add("e_clean%d" % lo, q, rb, re_, w=0, max_tries=1)
    # f. op order: leading and trailing I; leading and trailing D (a substitution directly before a deletion: build_ts)
    rb, re_ = interval(rng, 300, strand)
    a = aligned(pac, rb, re_)
    front, back = rng.integers(0, 4, 7).astype(np.uint8), rng.integers(0, 4, 5).astype(np.uint8)
    front[0], back[-1] = (a[0] + 1) & 3, (a[-1] + 1) & 3                       # no base of the copy can move into the junk
    add("f_ins", np.concatenate([front, a, back]), rb, re_, w=100)
    out.append(("f_piece", piece_read(pac, strand, F_PIECE_AT[strand])))
    rb, re_ = interval(rng, 300, strand)                                       # five ops: the most of any case
    a = aligned(pac, rb, re_)
    add("f_two_del", np.concatenate([a[:100], a[110:200], a[215:]]), rb, re_, w=100)
    return out


def build_ts(pac, strand):
    """the cases of the transition / transversion matrix: a substitution directly before a deletion, and a dense no-gap read
    whose score now depends on which bases meet"""
    rng = np.random.default_rng(200 + strand)
    rb, re_ = interval(rng, 1025, strand)
    q = dense(aligned(pac, rb, re_))
    return [("f_subdel", subdel_read(pac, strand, F_SUBDEL_AT[strand])),
            ("e1025_ts", spec(as_read(rb, q), rb, re_, w=0, max_tries=1))]


_cases = {}


def cases(strand, ts=False):
    """the planted cases of one strand; ts: the few that run with MAT_TS"""
    if (strand, ts) not in _cases:
        _cases[strand, ts] = (build_ts if ts else build)(genome_pac(), strand)
    return _cases[strand, ts]


def reference(oracle, specs, mat=MAT):
    return [gc.reg2aln(oracle, mat, PEN, L_PAC, genome_pac(), s["read"], s["rb"], s["re"], s["w"], s["w_cap"], s["min_score"],
                       s["max_tries"]) for s in specs]


_answers = {}


def answers(oracle, strand, ts=False):
    """the reference's answers to cases(strand, ts), computed once and shared; nobody changes them"""
    if (strand, ts) not in _answers:
        _answers[strand, ts] = reference(oracle, [s for _, s in cases(strand, ts)], MAT_TS if ts else MAT)
    return _answers[strand, ts]


def random_reads(strand, n=300):
    """seeded random 150-base reads as in test_gpu_cigar_ref.py: substitutions, indels, some with Ns"""
    rng = np.random.default_rng(300 + strand)
    pac = genome_pac()
    out = []
    for k in range(n):
        rb, re_ = interval(rng, int(rng.integers(140, 165)), strand)
        out.append(spec(read_of(rng, pac, rb, re_, 150, 0.04, 0.03, 0.01 if k % 3 == 0 else 0.0), rb, re_, w=100))
    return out


def md_runs(md):
    return [int(x) for x in re.findall(r"\d+", md)]


MD_FORMAT = re.compile(r"\d+(?:(?:[ACGTN]|\^[ACGTN]+)\d+)*")
MD_TOKEN = re.compile(r"(\d+)|\^([ACGTN]+)|([ACGTN])")


def rebuild(read, cigar, md, rev):
    """The aligned target from the read, the CIGAR and the MD alone, by the definition of MD: over all M ops taken together a
    number copies that many read bases and a letter is the target's base at a mismatch; '^' supplies the bases of an interior
    D; an I skips read bases; a leading or trailing D is in neither.  Letters go back through the strand's alphabet.
    Returns (target bases in aligned order without the outer D ops, edit count)."""
    assert MD_FORMAT.fullmatch(md), md[:80]
    code = {c: i for i, c in enumerate("TGCAN" if rev else "ACGTN")}
    q = np.asarray(read, dtype=np.uint8)
    q = q[::-1] if rev else q
    toks = [t for t in MD_TOKEN.findall(md) if t[0] == "" or int(t[0])]      # a run of 0 only separates
    out, ti, run, x, edits = [], 0, 0, 0, 0
    for k, (op, ln) in enumerate(cigar):
        if op == 0:
            need = ln
            while need:
                if run:
                    t = min(run, need)
                    out.append(q[x:x + t])
                    x, run, need = x + t, run - t, need - t
                    continue
                num, dele, letter = toks[ti]
                ti += 1
                if num:
                    run = int(num)
                    continue
                assert letter, ("a deletion inside an M op", k, md[:80])
                assert code[letter] != int(q[x]), ("a mismatch letter equal to the read's base", x)
                out.append(np.array([code[letter]], dtype=np.uint8))
                x, need, edits = x + 1, need - 1, edits + 1
        elif op == 1:
            x += ln
            edits += ln
        elif op == 2 and 0 < k < len(cigar) - 1:
            assert run == 0, ("a match run reaches into a deletion", k)
            dele = toks[ti][1]
            ti += 1
            assert len(dele) == ln, (k, ln, len(dele))
            out.append(np.array([code[c] for c in dele], dtype=np.uint8))
            edits += ln
    assert run == 0 and ti == len(toks) and x == len(q), (run, ti, len(toks), x, len(q))
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), edits


def check_rebuild(s, cigar, md, nm):
    """rebuild() must give the bases of bns_get_seq between the outer D ops, and NM edits"""
    rev = s["rb"] >= L_PAC
    want = aligned(genome_pac(), s["rb"], s["re"])
    lead = cigar[0][1] if cigar[0][0] == 2 else 0
    trail = cigar[-1][1] if len(cigar) > 1 and cigar[-1][0] == 2 else 0
    got, edits = rebuild(s["read"], cigar, md, rev)
    assert np.array_equal(got, want[lead:len(want) - trail]), (s["rb"], s["re"], cigar[:8], md[:80])
    assert edits == nm, (edits, nm, cigar[:8], md[:80])
