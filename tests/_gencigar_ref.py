"""CPU restatement of bwa_gen_cigar2 (bwa.c) and of mem_reg2aln's band-widening loop and infer_bw (bwamem.c), for the
tests of bsw_cigar_ref_batch.  The DP is the oracle's ksw_global2; the fetch (bns_get_seq) is numpy over the 2-bit pac, and
NM / MD follow bwa's CIGAR walk.  Nothing here calls the product library."""
import numpy as np

NEG = -(1 << 30)


def pac_base(pac, x):
    return (int(pac[x >> 2]) >> ((~x & 3) << 1)) & 3


def unpack_pac(pac, l_pac):
    p = np.asarray(pac, dtype=np.uint8)
    b = np.stack([(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3], axis=1).reshape(-1)
    return b[:l_pac].astype(np.uint8)


_unpacked = {}


def bns_get_seq(pac, l_pac, beg, end):
    """bwa's bns_get_seq: bases of [beg, end) in bwa coordinates (reverse strand = complement of the mirrored forward);
    the range is clipped to [0, 2*l_pac) and comes back empty when it bridges l_pac."""
    key = (id(pac), l_pac)
    if key not in _unpacked:
        _unpacked.clear()
        _unpacked[key] = (pac, unpack_pac(pac, l_pac))
    fwd = _unpacked[key][1]
    if end < beg:
        beg, end = end, beg
    end = min(end, 2 * l_pac)
    beg = max(beg, 0)
    if beg >= l_pac:
        x = np.arange(beg, end, dtype=np.int64)
        return (3 - fwd[2 * l_pac - 1 - x]).astype(np.uint8)
    if end <= l_pac:
        return fwd[beg:end].copy()
    return np.zeros(0, dtype=np.uint8)


def pack_pac(bases):
    b = np.asarray(bases, dtype=np.uint8)
    b4 = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)]).reshape(-1, 4)
    return (b4[:, 0] << 6 | b4[:, 1] << 4 | b4[:, 2] << 2 | b4[:, 3]).astype(np.uint8)


def band(mat, o_del, e_del, o_ins, e_ins, l_query, rlen, w_):
    max_ins = int(float(((l_query + 1) >> 1) * int(mat[0]) - o_ins) / e_ins + 1.)
    max_del = int(float(((l_query + 1) >> 1) * int(mat[0]) - o_del) / e_del + 1.)
    max_gap = max(max_ins, max_del, 1)
    d = abs(rlen - l_query)
    return max(min((max_gap + d + 1) >> 1, w_), d + 3)


def md_nm(cigar, query, rseq, rev):
    """bwa's walk: returns (NM, MD string).  cigar = [(op, len)], ops 0 M, 1 I, 2 D."""
    int2base = "TGCAN" if rev else "ACGTN"
    x = y = u = n_mm = n_gap = 0
    md = []
    for k, (op, ln) in enumerate(cigar):
        if op == 0:                   # for each base: a mismatch emits u and the reference letter, a match counts in u
            prev = 0
            for j in np.nonzero(np.asarray(query[x:x + ln]) != np.asarray(rseq[y:y + ln]))[0].tolist():
                md.append(str(u + j - prev))
                md.append(int2base[rseq[y + j]])
                n_mm += 1
                u, prev = 0, j + 1
            u += ln - prev
            x += ln
            y += ln
        elif op == 2:
            if 0 < k < len(cigar) - 1:
                md.append(str(u))
                md.append("^")
                md.extend(int2base[rseq[y + i]] for i in range(ln))
                u = 0
                n_gap += ln
            y += ln
        elif op == 1:
            x += ln
            n_gap += ln
    md.append(str(u))
    return n_mm + n_gap, "".join(md)


def gen_cigar2(oracle, mat, pen, w_, l_pac, pac, query, rb, re):
    """One bwa_gen_cigar2 call.  Returns dict(status, score, cigar, nm, md, band)."""
    o_del, e_del, o_ins, e_ins = pen
    l_query = len(query)
    if l_query <= 0 or rb >= re or (rb < l_pac < re):
        return dict(status=1)
    rseq = bns_get_seq(pac, l_pac, rb, re)
    if len(rseq) != re - rb:
        return dict(status=1)
    q = np.asarray(query, dtype=np.uint8)
    rev = rb >= l_pac
    if rev:
        q, rseq = q[::-1].copy(), rseq[::-1].copy()
    if l_query == re - rb and w_ == 0:
        cigar = [(0, l_query)]
        score = sum(int(mat[int(rseq[i]) * 5 + int(q[i])]) for i in range(l_query))
        bw = None
    else:
        bw = band(mat, o_del, e_del, o_ins, e_ins, l_query, len(rseq), w_)
        g = oracle.global2(q, rseq, mat, o_del, e_del, o_ins, e_ins, bw)
        score, cigar = g["score"], g["cigar"]
    nm, md = md_nm(cigar, q, rseq, rev)
    return dict(status=0, score=score, cigar=cigar, nm=nm, md=md, band=bw)


def reg2aln(oracle, mat, pen, l_pac, pac, query, rb, re, w, w_cap=0, min_score=-(1 << 31), max_tries=1):
    """mem_reg2aln's loop around gen_cigar2 with the task fields of bsw_ctask.  Returns the final try's dict plus w, tries,
    and the list of bands run."""
    wcap = w_cap if w_cap else w
    max_tries = max_tries if max_tries else 1
    w2, last, i, runs = w, NEG, 0, []
    while True:
        w2 = min(w2, wcap)
        r = gen_cigar2(oracle, mat, pen, w2, l_pac, pac, query, rb, re)
        runs.append(w2)
        if r["status"]:
            r.update(w=w2, tries=1, runs=runs, stop="status")
            return r
        score = r["score"]
        if score == last or w2 == wcap:
            stop = "equal" if score == last else "cap"
            break
        last = score
        w2 <<= 1
        i += 1
        if not (i < max_tries and score < min_score):
            stop = "tries" if i >= max_tries else "score"
            break
    r.update(w=runs[-1], tries=len(runs), runs=runs, stop=stop)
    return r


def infer_bw(l1, l2, score, a, q, r):
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int(float(min(l1, l2) * a - score - q) / r + 2.)
    return max(w, abs(l1 - l2))
