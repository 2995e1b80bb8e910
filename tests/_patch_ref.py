"""CPU restatement of mem_patch_reg (bwamem.c of bwa >= 0.7.10, as recalled: bwa's source is not in the tree), for the tests of
bsw_patch_ref_batch.  The alignment's score is _gencigar_ref.gen_cigar2's; the arithmetic on both sides of it is IEEE double, in
bwa's order, with bwa's FLOAT constants promoted to double.  Nothing here calls the product library."""
import math

import numpy as np

import _gencigar_ref as G

F005 = float(np.float32(0.05))           # 0.05f  = 0.0500000007...
F010 = float(np.float32(0.05) * np.float32(2))        # 0.05f * 2 (a float product, exact)
F090 = float(np.float32(0.90))           # 0.90f

# why a call returns 0 before the alignment (pretest()'s second value), in bwa's order
STRAND, COLINEAR, GAP_W, GAP_R, OVL_W, OVL_R, RUNS = "strand", "colinear", "gap_w", "gap_r", "ovl_w", "ovl_r", "runs"


def reg(rb, re, qb, qe, score, w=0):
    return dict(rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), score=int(score), w=int(w))


def _div(x, y):
    """C's double division: x / 0 is an infinity or a NaN, not an error"""
    if y == 0:
        return math.nan if x == 0 or x != x else math.copysign(math.inf, x)
    return x / y


def pretest(opt_w, l_pac, a, b):
    """-> (runs 0/1, w_ or 0, why)"""
    if a["rb"] < l_pac and b["rb"] >= l_pac:
        return 0, 0, STRAND
    if a["qb"] >= b["qb"] or a["qe"] >= b["qe"] or a["re"] >= b["re"]:
        return 0, 0, COLINEAR
    w = abs((a["re"] - b["rb"]) - (a["qe"] - b["qb"]))
    r = abs(_div(float(a["re"] - b["rb"]), float(b["re"] - a["rb"])) - _div(float(a["qe"] - b["qb"]), float(b["qe"] - a["qb"])))
    if a["re"] < b["rb"] or a["qe"] < b["qb"]:
        if w > opt_w << 1:
            return 0, 0, GAP_W
        if r >= F005:
            return 0, 0, GAP_R
    else:
        if w > opt_w << 2:
            return 0, 0, OVL_W
        if r >= F010:
            return 0, 0, OVL_R
    w += a["w"] + b["w"]
    w = min(w, opt_w << 2)
    return 1, w, RUNS


def _to_int(x):
    return int(x)                        # C's (int): truncation towards zero (the tests stay inside int's range)


def expected_scores(a, b):
    s = b["score"] + a["score"]
    q_s = _to_int(float(b["qe"] - a["qb"]) / ((b["qe"] - b["qb"]) + (a["qe"] - a["qb"])) * s + .499)
    r_s = _to_int(float(b["re"] - a["rb"]) / ((b["re"] - b["rb"]) + (a["re"] - a["rb"])) * s + .499)
    return q_s, r_s


def decide(a, b, score):
    """mem_patch_reg's return value once bwa_gen_cigar2 has answered `score`"""
    q_s, r_s = expected_scores(a, b)
    if _div(float(score), float(max(q_s, r_s))) < F090:
        return 0
    return score


def patch_reg(oracle, mat, pen, opt_w, l_pac, pac, read, a, b):
    """One mem_patch_reg call as bsw_presult reports it: dict(score, w, gscore, status) plus why / shortcut / rev for the tests'
    counts.  read: the whole read."""
    runs, w, why = pretest(opt_w, l_pac, a, b)
    out = dict(score=0, w=0, gscore=0, status=1, why=why, shortcut=False, rev=a["rb"] >= l_pac)
    if not runs:
        return out
    rb, re = a["rb"], b["re"]
    if rb < 0 or re > 2 * l_pac:         # bns_get_seq cannot return the interval whole
        out["why"] = "noaln"
        return out
    g = G.gen_cigar2(oracle, mat, pen, w, l_pac, pac, np.asarray(read[a["qb"]:b["qe"]], dtype=np.uint8), rb, re)
    if g["status"]:
        out["why"] = "noaln"
        return out
    ret = decide(a, b, g["score"])
    out.update(score=ret, w=w, gscore=g["score"], status=0 if ret > 0 else 2, shortcut=g["band"] is None)
    return out
