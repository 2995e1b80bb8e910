"""mem_sort_dedup_patch restated sequentially in Python (bwamem.c of bwa 0.7.12 - 0.7.17 as recalled; bwa's source is not in the
tree), and the seeded workload its tests and tools/sdp_rate.py share.  TEST INFRASTRUCTURE: the yardstick for bsw_sdp_* (the engine
of bsw_sdp.c and the job built on it); nothing here calls them.

The restatement walks bwa's two loops read by read.  mem_patch_reg is tests/_patch_ref.py::patch_reg (CPU oracle), called ONLY
when the loop reaches it; the redundancy test's arithmetic is numpy.float32 (bwa's mask_level_redun is a C float).  Both sorts
are stable, the rule the library documents.

A workload is a dict: l_pac, both, pac, reads (uint8 arrays), regs (per read: a list of region dicts in the caller's order)."""
import numpy as np

import _chain2aln_ref as C
import _patch_ref as P

FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "sub", "csub", "rid", "n_comp", "read", "src")
PREG = ("rb", "re", "qb", "qe", "score", "w")


def preg(r):
    return {k: r[k] for k in PREG}


def key12(q, p):
    return tuple(q[k] for k in PREG) + tuple(p[k] for k in PREG)


class Patcher:
    """mem_patch_reg through the CPU oracle, one call at a time; the answers are remembered (the engine's test asks again)"""
    def __init__(self, host, oracle, params, wl):
        p = params[0]
        self.oracle, self.mat, self.opt_w, self.wl = oracle, p["mat"], int(p["w"]), wl
        self.pen = (int(p["o_del"]), int(p["e_del"]), int(p["o_ins"]), int(p["e_ins"]))
        self.memo, self.calls = {}, 0

    def __call__(self, read, a, b):
        k = (read,) + key12(a, b)
        self.calls += 1
        if k not in self.memo:
            self.memo[k] = P.patch_reg(self.oracle, self.mat, self.pen, self.opt_w, self.wl["l_pac"], self.wl["pac"], self.wl["reads"][read],
                                       preg(a), preg(b))
        return self.memo[k]

    def pretest(self, a, b):
        return P.pretest(self.opt_w, self.wl["l_pac"], preg(a), preg(b))


def redundant(p, q, mlr, cnt=None):
    """the test of bwa's inner loop in binary32; cnt["float_edge"] counts the pairs that double arithmetic decides otherwise"""
    orr = q["re"] - p["rb"]
    oq = q["qe"] - p["qb"] if q["qb"] < p["qb"] else p["qe"] - q["qb"]
    mr = min(q["re"] - q["rb"], p["re"] - p["rb"])
    mq = min(q["qe"] - q["qb"], p["qe"] - p["qb"])
    f = np.float32(mlr)
    got = bool(np.float32(orr) > f * np.float32(mr) and np.float32(oq) > f * np.float32(mq))
    if cnt is not None:
        dbl = orr > float(f) * mr and oq > float(f) * mq           # the float constant promoted, as C would without the casts
        if dbl != got:
            cnt["float_edge"] += 1
            cnt["float_edge_mr100"] += (mr == 100 and orr == 95 and dbl and not got)
    return got


def descends(p, q, gap):
    return p["rid"] == q["rid"] and p["rb"] < q["re"] + gap


def first_round(a, patcher, mlr=.95, gap=10000):
    """the speculation on the sorted UNMODIFIED regions of one read: every (i, j) down to which the descent's condition holds, that
    is not redundant, has q.rb < p.rb and passes the pre-tests -> list of (j, i)"""
    out = []
    for i in range(1, len(a)):
        j = i - 1
        while j >= 0 and descends(a[i], a[j], gap):
            q = a[j]
            if not redundant(a[i], q, mlr) and q["rb"] < a[i]["rb"] and patcher.pretest(q, a[i])[0]:
                out.append((j, i))
            j -= 1
    return out


def new_counts():
    return dict(alns=0, merges=0, kills_p=0, kills_q=0, dups=0, rounds=0, tasks_first=0, tasks=0, float_edge=0, float_edge_mr100=0,
                rid_hidden=0, reach_after_merge=0, noaln=0, not_merged=0, why={}, equal_re=0, dup_runs3=0)


def sdp_read(regs, read, patcher, cnt, mlr=.95, gap=10000, patch=True, presorted=False):
    """mem_sort_dedup_patch on one read's regions (dicts; copied) -> the surviving regions in bwa's order.  cnt: counts over the
    workload (new_counts), cnt["rounds"] = this read's rounds (the caller takes the maximum)"""
    a = [dict(r) for r in regs]
    n = len(a)
    rounds = 0
    if n <= 1:
        return a, rounds
    if not presorted:
        a = sorted(a, key=lambda r: r["re"])              # stable
    cnt["equal_re"] += sum(a[i]["re"] == a[i - 1]["re"] for i in range(1, n))
    for r in a:
        r["n_comp"] = 1
    known = set()
    if patch:                                               # what round 1 asks for
        for j, i in first_round(a, patcher, mlr, gap):
            known.add(key12(a[j], a[i]))
            cnt["tasks_first"] += 1
            cnt["tasks"] += 1
        rounds = 1 if known else 0
    for i in range(1, n):
        p = a[i]
        if p["rid"] != a[i - 1]["rid"] or p["rb"] >= a[i - 1]["re"] + gap:
            if p["rid"] != a[i - 1]["rid"] and any(descends(p, a[k], gap) and a[k]["qe"] > a[k]["qb"] for k in range(i - 1)):
                cnt["rid_hidden"] += 1
            continue
        rb0 = p["rb"]
        j = i - 1
        while j >= 0 and descends(p, a[j], gap):
            q = a[j]
            if q["qe"] == q["qb"]:
                j -= 1
                continue
            if p["rb"] != rb0 and rb0 >= q["re"] + gap:
                cnt["reach_after_merge"] += 1
            if redundant(p, q, mlr, cnt):
                if p["score"] < q["score"]:
                    p["qe"] = p["qb"]
                    cnt["kills_p"] += 1
                    break
                q["qe"] = q["qb"]
                cnt["kills_q"] += 1
            elif q["rb"] < p["rb"] and patch:
                runs, _, why = patcher.pretest(q, p)
                cnt["why"][why] = cnt["why"].get(why, 0) + 1
                if runs:
                    if key12(q, p) not in known:           # a merge stands between this pair and what was asked: one more round
                        rounds += 1
                        k, asked = j, []
                        while k >= 0 and descends(p, a[k], gap):
                            qq = a[k]
                            if (qq["qe"] > qq["qb"] and not redundant(p, qq, mlr) and qq["rb"] < p["rb"] and patcher.pretest(qq, p)[0]
                                    and (k == j or key12(qq, p) not in known)):
                                asked.append(key12(qq, p))
                            k -= 1
                        known.update(asked)
                        cnt["tasks"] += len(asked)
                    res = patcher(read, q, p)
                    cnt["alns"] += 1
                    cnt["noaln"] += res["status"] == 1
                    cnt["not_merged"] += res["status"] == 2
                    if res["score"] > 0:
                        cnt["merges"] += 1
                        p["n_comp"] += q["n_comp"] + 1
                        for f in ("seedcov", "sub", "csub"):
                            p[f] = max(p[f], q[f])
                        p["qb"], p["rb"] = q["qb"], q["rb"]
                        p["truesc"] = p["score"] = res["score"]
                        p["w"] = res["w"]
                        q["qb"] = q["qe"]
            j -= 1
        if j >= 0 and p["rid"] != a[j]["rid"] and p["qe"] > p["qb"]:
            if any(descends(p, a[k], gap) and a[k]["qe"] > a[k]["qb"] for k in range(j)):
                cnt["rid_hidden"] += 1
    a = [r for r in a if r["qe"] > r["qb"]]
    a = sorted(a, key=lambda r: (-r["score"], r["rb"], r["qb"]))     # stable
    same = [i >= 1 and (a[i]["score"], a[i]["rb"], a[i]["qb"]) == (a[i - 1]["score"], a[i - 1]["rb"], a[i - 1]["qb"]) for i in range(len(a))]
    cnt["dups"] += sum(same)
    cnt["dup_runs3"] += sum(same[i] and same[i - 1] for i in range(1, len(a)))
    return [r for r, s in zip(a, same) if not s], rounds


def sdp(wl, patcher, **opt):
    """-> (regions of every read laid end to end, out_start, counts, rounds per read)"""
    cnt = new_counts()
    out, start, rounds = [], [0], []
    src = 0
    for ri, regs in enumerate(wl["regs"]):
        mine = [dict(r, src=src + k) for k, r in enumerate(regs)]
        src += len(regs)
        got, rd = sdp_read(mine, ri, patcher, cnt, **opt)
        out += got
        start.append(len(out))
        rounds.append(rd)
    cnt["rounds"] = max(rounds) if rounds else 0
    return out, start, cnt, rounds


def arrays(host, wl):
    """-> (SREG array, reg_start, lens): the caller's order, src left 0 (the library ignores it on input)"""
    n = sum(len(r) for r in wl["regs"])
    s = np.zeros(n, dtype=host.SREG)
    start = np.zeros(len(wl["regs"]) + 1, dtype=np.uint64)
    at = 0
    for ri, regs in enumerate(wl["regs"]):
        for r in regs:
            for f in FIELDS[:-1]:
                s[at][f] = r[f]
            at += 1
        start[ri + 1] = at
    return s, start, np.array([len(r) for r in wl["reads"]], dtype=np.int32)


def same_regions(got, want):
    """got: SREG array, want: the restatement's list -> None, or the first difference"""
    if len(got) != len(want):
        return "regions: %d, the restatement has %d" % (len(got), len(want))
    for f in FIELDS:
        w = np.array([a[f] for a in want], dtype=got.dtype[f]) if want else np.zeros(0, dtype=got.dtype[f])
        bad = np.nonzero(got[f] != w)[0]
        if len(bad):
            i = int(bad[0])
            return "region %d field %s: %r, the restatement has %r (%r)" % (i, f, got[f][i], w[i], want[i])
    return None


def same_stats(st, cnt, n_reads, n_in, n_out):
    want = dict(reads=n_reads, regs_in=n_in, regs_out=n_out, merges=cnt["merges"], kills_p=cnt["kills_p"], kills_q=cnt["kills_q"],
                dups=cnt["dups"], rounds=cnt["rounds"], tasks_first=cnt["tasks_first"], tasks=cnt["tasks"], alns_bwa=cnt["alns"])
    return None if st == want else "stats %r, the restatement has %r" % (st, want)


# ---- the seeded workload -----------------------------------------------------------------------------------------------------------

def region(rb, re, qb, qe, score, read, rid=0, w=0, rng=None, n_comp=0):
    r = dict(rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), score=int(score), truesc=int(score), w=int(w), seedcov=(int(qe) - int(qb)) // 2,
             sub=0, csub=0, rid=int(rid), n_comp=int(n_comp), read=int(read))
    if rng is not None:
        r["sub"], r["csub"], r["seedcov"] = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(10, qe - qb + 1))
    return r


def place(rng, L, span, strand=None):
    """a start in [0, 2L) coordinates such that [x, x + span) lies inside one contig of one strand -> (x, rid)"""
    strand = int(rng.integers(0, 2)) if strand is None else strand
    while True:
        x = int(rng.integers(50, L - span - 50)) + strand * L
        if C.contig_of(x)[1] == C.contig_of(x + span)[1]:
            return x, C.contig_of(x)[1]


def segmented(rng, both, L, ri, n_seg, lo=45, hi=75, junk_last=False, strand=None):
    """a read of n_seg colinear pieces of the genome with an insertion or a deletion of 0 - 12 bases between them, and a region per
    piece: its score is the piece's length less a share of the gap's cost, so that a true join passes mem_patch_reg's 0.90 ratio"""
    lens = [int(rng.integers(lo, hi + 1)) for _ in range(n_seg)]
    x, rid = place(rng, L, sum(lens) + 13 * n_seg + 4, strand)
    parts, regs, q, r = [], [], 0, x
    for k, ln in enumerate(lens):
        if k:
            d = int(rng.integers(0, 13))
            if rng.integers(0, 2):
                parts.append(rng.integers(0, 4, d).astype(np.uint8))
                q += d
            else:
                r += d
        seg = both[r:r + ln].copy()
        if junk_last and k == n_seg - 1:
            seg = rng.integers(0, 4, ln).astype(np.uint8)
        parts.append(seg)
        cl = int(rng.integers(0, 4)) if k else 0
        cr = int(rng.integers(0, 4)) if k < n_seg - 1 else 0
        regs.append(region(r + cl, r + ln - cr, q + cl, q + ln - cr, ln - cl - cr - int(rng.integers(8, 14)), ri, rid, int(rng.integers(0, 20)), rng))
        q += ln
        r += ln
    read = np.concatenate(parts).astype(np.uint8)
    sub = np.nonzero(rng.random(len(read)) < 0.004)[0]
    read[sub] = (read[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
    return read, regs, rid


def make_workload(n_reads=340, seed=516, genome=None):      # (with this seed no read needs a fourth round; the tests assert it)
    """reads of 1 - 4 colinear segments off both strands with their regions (in a shuffled order), decoy regions of other contigs,
    and hand-made reads for every branch of the loop: both redundancy kills, the binary32 boundary, a descent hidden behind another
    rid, a pair only a merge brings within max_chain_gap = 100, equal re, exact duplicates (three in a row too), reads with no and
    with one region, every pre-test's failure, an interval that bridges l_pac."""
    g = genome or C.make_genome()
    L, both = g["l_pac"], g["both"]
    rng = np.random.default_rng(seed)
    reads, regs = [], []

    def rand_read(n):
        x, rid = place(rng, L, n + 10)
        return both[x:x + n].copy(), x, rid

    for i in range(n_reads):
        ri, kind, odd = len(reads), i % 34, (i // 34) % 2
        if kind < 16:                                           # 1 - 4 segments; every fourth 4-segment read ends in junk (the ratio fails)
            n_seg = 1 + kind % 4
            read, mine, rid = segmented(rng, both, L, ri, n_seg, junk_last=(kind == 15))
            if kind in (4, 9):                                  # a decoy on another contig
                dx, drid = place(rng, L, 80)
                mine.append(region(dx, dx + 40, 5, 45, 22, ri, drid + 3 if drid == rid else drid, 3, rng))
        elif kind == 16:                                        # no region
            read, mine = rand_read(100)[0], []
        elif kind == 17:                                        # one region: returned untouched, n_comp included
            read, x, rid = rand_read(100)
            mine = [region(x + 3, x + 90, 3, 90, 80, ri, rid, 4, rng, n_comp=7)]
        elif kind in (18, 19):                                  # a shadow one base on: p (the later re) has the lower / the higher score
            read, mine, rid = segmented(rng, both, L, ri, 2)
            b = mine[int(rng.integers(0, 2))]
            mine.append(dict(b, rb=b["rb"] - 1, re=b["re"] + 1, qb=b["qb"], qe=b["qe"], score=b["score"] + (-5 if kind == 18 else 5)))
        elif kind == 20:                                        # the binary32 boundary: mr = 100, or = 95, oq = 98 of mq = 100
            read, x, rid = rand_read(140)
            mine = [region(x, x + 100, 0, 100, 92, ri, rid, 2, rng), region(x + 5, x + 105, 2, 102, 92, ri, rid, 2, rng)]
        elif kind == 21:                                        # another rid between two regions that would join
            read, mine, rid = segmented(rng, both, L, ri, 2)
            mid = (mine[0]["re"] + mine[1]["re"]) // 2
            mine.append(region(mid - 30, mid, 10, 40, 25, ri, rid + 7, 1, rng))
        elif kind == 22:                                        # two long segments and a region Z of a later part of the read inside the
            read, mine, rid = segmented(rng, both, L, ri, 2, 150, 160)     # first: within 100 of p only once p has swallowed the first
            z0 = mine[0]["rb"] + 5
            mine.append(region(z0, z0 + 40, mine[1]["qb"] + 60, mine[1]["qb"] + 100, 30, ri, rid, 0, rng))
        elif kind == 23:                                        # equal re, equal scores: which is q is the stable order's to say
            read, x, rid = rand_read(120)
            mine = [region(x, x + 100, 0, 100, 90, ri, rid, 1, rng), region(x + 3, x + 100, 3, 100, 90, ri, rid, 5, rng)]
            if odd:
                mine.reverse()
        elif kind == 24:                                        # exact (score, rb, qb) duplicates the loop never compares: other rids
            read, x, rid = rand_read(120)
            mine = [region(x, x + 90 + k, 0, 90 + k, 77, ri, rid + 10 + k, k, rng) for k in range(3 if odd else 2)]
            mine.append(region(x + 200, x + 260, 30, 90, 50, ri, rid, 0, rng))
        elif kind == 25:                                        # strands: q at the end of the forward strand, p at the start of the other
            read = rand_read(220)[0]
            mine = [region(L - 300, L - 200, 0, 100, 90, ri, 2), region(L + 100, L + 200, 110, 210, 90, ri, 2)]
        elif kind == 26:                                        # not colinear: the later piece of the reference is the earlier of the read
            read, x, rid = rand_read(220)
            mine = [region(x, x + 100, 110, 210, 90, ri, rid), region(x + 110, x + 210, 0, 100, 90, ri, rid)]
        elif kind == 27:                                        # a gap wider than the band / beyond the ratio
            read, x, rid = rand_read(220)
            g_ = 300 if odd else 60
            mine = [region(x, x + 100, 0, 100, 90, ri, rid), region(x + 100 + g_, x + 200 + g_, 100, 200, 90, ri, rid)]
        elif kind == 28:                                        # overlapping, by amounts too different for the band
            read, x, rid = rand_read(1040)
            mine = [region(x, x + 520, 0, 520, 500, ri, rid), region(x + 70, x + 590, 510, 1030, 500, ri, rid)]
        elif kind == 29:                                        # ... within the band, beyond the ratio
            read, x, rid = rand_read(200)
            mine = [region(x, x + 100, 0, 100, 90, ri, rid), region(x + 40, x + 140, 95, 195, 90, ri, rid)]
        elif kind == 30:                                        # the joined interval bridges l_pac: bwa_gen_cigar2 has no alignment
            read = both[L - 160:L + 60].copy()
            mine = [region(L - 160, L - 60, 0, 100, 90, ri, 2), region(L - 55, L + 45, 105, 205, 90, ri, 2)]
        else:                                                   # three segments, the middle one twice (a repeat copy elsewhere, same rid)
            read, mine, rid = segmented(rng, both, L, ri, 3)
            m = mine[1]
            far = m["re"] + 20000
            if far + 100 < 2 * L and (far + 100 < L) == (m["rb"] < L) and C.contig_of(far)[1] == C.contig_of(far + 100)[1] == rid:
                mine.append(dict(m, rb=far, re=far + (m["re"] - m["rb"]), score=m["score"] - 3))
        order = rng.permutation(len(mine)) if kind not in (23,) else np.arange(len(mine))
        reads.append(np.ascontiguousarray(read, dtype=np.uint8))
        regs.append([mine[k] for k in order])
    wl = dict(g)
    wl.update(reads=reads, regs=regs)
    return wl
