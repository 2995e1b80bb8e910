"""CPU restatement of bwa's mate rescue (mem_matesw, bwamem_pair.c) and mem_infer_dir, for the tests of bsw_matesw_ref_batch.
The alignment is the oracle's ksw_align2; the window fetch is _gencigar_ref.bns_get_seq.  bwa's source is not in the tree:
these are its 0.7.x semantics as recalled.  Nothing here calls the product library."""
import numpy as np

import _gencigar_ref as gc

NOT_RUN = {"score": 0, "te": -1, "qe": -1, "score2": -1, "te2": -1, "tb": -1, "qb": -1}
ALN = ("score", "te", "qe", "score2", "te2", "tb", "qb")


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir: (orientation, distance) of an anchor at b1 and a mate at b2."""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    dist = p2 - b1 if p2 > b1 else b1 - p2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), dist


def windows(anchor_rb, l_ms, l_pac, low, high, failed):
    """mem_matesw's window per orientation r: (rb, re, is_rev, skip)."""
    out = []
    for r in range(4):
        is_rev = (r >> 1) != (r & 1)
        is_larger = not (r >> 1)
        if not is_rev:
            rb = anchor_rb + low[r] if is_larger else anchor_rb - high[r]
            re = (anchor_rb + high[r] if is_larger else anchor_rb - low[r]) + l_ms
        else:
            rb = (anchor_rb + low[r] if is_larger else anchor_rb - high[r]) - l_ms
            re = anchor_rb + high[r] if is_larger else anchor_rb - low[r]
        rb = max(rb, 0)
        re = min(re, 2 * l_pac)
        out.append((rb, re, int(is_rev), 1 if failed[r] else 0))
    return out


def revcomp(ms):
    ms = np.asarray(ms, dtype=np.uint8)
    return np.where(ms < 4, 3 - ms, 4).astype(np.uint8)[::-1].copy()


def runs(l_pac, l_ms, rb, re):
    return l_ms > 0 and rb < re and not (rb < l_pac < re) and rb >= 0 and re <= 2 * l_pac


def matesw(oracle, mat, pen, l_pac, pac, ms, is_rev, rb, re, xtra, min_score):
    """One task of bsw_matesw_ref_batch: dict(aln=dict, status, rb, re, qb, qe, score, csub, seedcov)."""
    zero = {"status": 1, "rb": 0, "re": 0, "qb": 0, "qe": 0, "score": 0, "csub": 0, "seedcov": 0}
    l_ms = len(ms)
    if not runs(l_pac, l_ms, rb, re):
        return dict(zero, aln=dict(NOT_RUN))
    ref = gc.bns_get_seq(pac, l_pac, rb, re)
    assert len(ref) == re - rb
    seq = revcomp(ms) if is_rev else np.asarray(ms, dtype=np.uint8)
    a = oracle.align2(seq, ref, mat, *pen, xtra)
    aln = {k: a[k] for k in ALN}
    if not (aln["score"] >= min_score and aln["qb"] >= 0):
        return dict(zero, status=2, aln=aln)
    b = {"status": 0, "aln": aln}
    b["qb"] = l_ms - (aln["qe"] + 1) if is_rev else aln["qb"]
    b["qe"] = l_ms - aln["qb"] if is_rev else aln["qe"] + 1
    b["rb"] = 2 * l_pac - (rb + aln["te"] + 1) if is_rev else rb + aln["tb"]
    b["re"] = 2 * l_pac - (rb + aln["tb"]) if is_rev else rb + aln["te"] + 1
    b["score"], b["csub"] = aln["score"], aln["score2"]
    b["seedcov"] = min(b["re"] - b["rb"], b["qe"] - b["qb"]) >> 1
    return b


def xtra_of(l_ms, a, min_seed_len):
    """mem_matesw's xtra: KSW_XSUBO | KSW_XSTART | (l_ms * a < 250 ? KSW_XBYTE : 0) | (min_seed_len * a)."""
    return 0x40000 | 0x80000 | (0x10000 if l_ms * a < 250 else 0) | (min_seed_len * a)


def matesw_batch(oracle, atask_dtype, mat, pen, l_pac, pac, mates, is_rev, rb, re, xtra, min_score, nthreads=16):
    """matesw() over many tasks, the alignments on the oracle's threaded ksw_align2 batch.  Returns a dict of arrays with the
    fields of bsw_mresult (aln as an int32[n, 7] in ALN order)."""
    n = len(mates)
    keep = []
    at = np.zeros(n, dtype=atask_dtype)
    run = np.zeros(n, dtype=bool)
    for i in range(n):
        if not runs(l_pac, len(mates[i]), int(rb[i]), int(re[i])):
            continue
        run[i] = True
        ref = gc.bns_get_seq(pac, l_pac, int(rb[i]), int(re[i]))
        seq = revcomp(mates[i]) if is_rev[i] else np.ascontiguousarray(mates[i], dtype=np.uint8)
        keep += [ref, seq]
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = (seq.ctypes.data, ref.ctypes.data, len(seq),
                                                                                        len(ref), int(xtra[i]))
    idx = np.nonzero(run)[0]
    aln = np.tile(np.array([NOT_RUN[k] for k in ALN], dtype=np.int32), (n, 1))
    if len(idx):
        aln[idx], _ = oracle.align2_batch(mat, *pen, at[idx], nthreads=nthreads)
    score, te, qe, score2, tb, qb = (aln[:, ALN.index(k)].astype(np.int64) for k in ("score", "te", "qe", "score2", "tb", "qb"))
    l_ms = np.array([len(m) for m in mates], dtype=np.int64)
    rev = np.asarray(is_rev, dtype=bool)
    rb, re = np.asarray(rb, dtype=np.int64), np.asarray(re, dtype=np.int64)
    keep_it = run & (score >= np.asarray(min_score, dtype=np.int64)) & (qb >= 0)
    out = {"aln": aln, "status": np.where(run, np.where(keep_it, 0, 2), 1)}
    out["qb"] = np.where(rev, l_ms - (qe + 1), qb)
    out["qe"] = np.where(rev, l_ms - qb, qe + 1)
    out["rb"] = np.where(rev, 2 * l_pac - (rb + te + 1), rb + tb)
    out["re"] = np.where(rev, 2 * l_pac - (rb + tb), rb + te + 1)
    out["score"], out["csub"] = score, score2
    out["seedcov"] = np.minimum(out["re"] - out["rb"], out["qe"] - out["qb"]) >> 1
    for k in ("qb", "qe", "rb", "re", "score", "csub", "seedcov"):
        out[k] = np.where(keep_it, out[k], 0)
    return out
