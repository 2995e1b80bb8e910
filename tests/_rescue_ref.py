"""The mate-rescue loop of mem_sam_pe with mem_matesw inside it, restated sequentially in Python (bwamem_pair.c of bwa 0.7.12 - 0.7.17
as recalled; bwa's source is not in the tree), and the seeded workload its tests and tools/rescue_rate.py share.  TEST
INFRASTRUCTURE: the yardstick for bsw_rescue_* (the engine of bsw_rescue.c and the job built on it); nothing here calls them.

The restatement walks bwa's loop pair by pair, direction by direction, anchor by anchor.  A window is aligned on the CPU oracle
(tests/_matesw_ref.py::matesw) ONLY when the loop reaches it; the pass that ends an orientation is tests/_sdp_ref.py::sdp_read with
patch = False.  What round 1 would ask for and what a stall would add are bookkeeping beside the walk: they change no region.

A workload is a dict: l_pac, both, pac, contigs ((offset, len) ...), reads (uint8 arrays; 2k and 2k + 1 are mates), regs (per
read: a list of region dicts, bwa's order: score descending), and what was built by hand (`hand`: name -> pair index)."""
import numpy as np

import _gencigar_ref as gc
import _matesw_ref as M
import _sdp_ref as S

NEW = 0x80000000
CONTIGS = ((0, 20000), (20000, 21001), (41001, 19000))
L_PAC = 60001
LOW, HIGH = 100, 500
LATE_SITES = (5000, 12000, 50000)        # x1 of the hand-made late cases: a copy of the mate is planted 300 bases to the left

FR = dict(low=[0, LOW, 0, 0], high=[0, HIGH, 0, 0], failed=[1, 0, 1, 1])
# name -> (options of bsw_rescue_opt on top of the defaults, with the contig table or without)
CONFIGS = {
    "fr": (dict(FR), True),
    "two": (dict(low=[LOW, LOW, 0, 0], high=[HIGH, HIGH, 0, 0], failed=[0, 0, 1, 1]), True),      # FF and FR live
    "mm1": (dict(FR, max_matesw=1), True),
    "nocontig": (dict(FR), False),
}
DEFAULTS = dict(pen_unpaired=17, max_matesw=50, min_seed_len=19, a=1, mask_level_redun=.95, max_chain_gap=10000)


def options(name, contigs=CONTIGS):
    """name: a key of CONFIGS, or (options on top of the defaults, with the contig table or without) itself
    -> (every option as a dict, the contig table or None)"""
    over, with_contigs = CONFIGS[name] if isinstance(name, str) else name
    return dict(DEFAULTS, **over), (tuple(contigs) if with_contigs else None)


def pen_of(params):
    p = params[0]
    return int(p["o_del"]), int(p["e_del"]), int(p["o_ins"]), int(p["e_ins"])


class Aligner:
    """one window through the CPU oracle, one call at a time; the answers are remembered (the engine's test asks again)"""
    def __init__(self, oracle, params, wl):
        self.oracle, self.mat, self.pen, self.wl = oracle, params[0]["mat"], pen_of(params), wl
        self.memo, self.calls = {}, 0

    def __call__(self, read, is_rev, rb, re, xtra, min_score):
        k = (read, is_rev, rb, re, xtra, min_score)
        self.calls += 1
        if k not in self.memo:
            self.memo[k] = M.matesw(self.oracle, self.mat, self.pen, self.wl["l_pac"], self.wl["pac"], self.wl["reads"][read], is_rev, rb, re,
                                    xtra, min_score)
        return self.memo[k]


def contig_step(l_pac, contigs, rid_a, rb, re):
    """bns_fetch_seq's part: -> (passed, rb, re, clamped)"""
    mid = (rb + re) >> 1
    fwd = 2 * l_pac - 1 - mid if mid >= l_pac else mid
    rid = next(k for k, (o, n) in enumerate(contigs) if o <= fwd < o + n)
    o, n = contigs[rid]
    lo, hi = (o, o + n) if mid < l_pac else (2 * l_pac - o - n, 2 * l_pac - o)
    nrb, nre = max(rb, lo), min(re, hi)
    return rid == rid_a, nrb, nre, (nrb, nre) != (rb, re)


def window(wl, opt, contigs, a, l_ms, r, cnt=None):
    """orientation r of anchor a -> (a task exists, rb, re, is_rev)"""
    rb, re, is_rev, _ = M.windows(a["rb"], l_ms, wl["l_pac"], opt["low"], opt["high"], opt["failed"])[r]
    passed = True
    if rb < re and contigs is not None:
        passed, rb, re, clamped = contig_step(wl["l_pac"], contigs, a["rid"], rb, re)
        if cnt is not None:
            cnt["clamped"] += passed and clamped
            cnt["other_contig"] += not passed
    long_enough = re - rb >= opt["min_seed_len"]
    if cnt is not None and passed and not long_enough:
        cnt["short"] += 1
    return passed and long_enough, rb, re, is_rev


def skips(wl, opt, a, ma):
    skip = [1 if f else 0 for f in opt["failed"]]
    for m in ma:
        r, dist = M.infer_dir(wl["l_pac"], a["rb"], m["rb"])
        if opt["low"][r] <= dist <= opt["high"][r]:
            skip[r] = 1
    return skip


def anchors_of(regs, opt, cnt=None):
    """the anchors of one read's regions: within pen_unpaired of the first, in input order, max_matesw at most"""
    near = [g for g in regs if g["score"] >= regs[0]["score"] - opt["pen_unpaired"]]
    if cnt is not None:
        cnt["pen_cut"] += len(regs) - len(near)
        cnt["max_cut"] += max(0, len(near) - opt["max_matesw"])
    return near[:opt["max_matesw"]]


def task_of(wl, opt, mate, rb, re, is_rev):
    l_ms = len(wl["reads"][mate])
    return (mate, is_rev, rb, re, M.xtra_of(l_ms, opt["a"], opt["min_seed_len"]), opt["min_seed_len"])


def first_round(wl, opt, contigs, src_regs):
    """what round 1 asks for: every (anchor, r) not skipped on the INITIAL ma whose clamped window passes -> {(anchor src, r): task}"""
    out = {}
    for d in range(len(wl["reads"])):
        mate = d ^ 1
        if not src_regs[d]:
            continue
        for a in anchors_of(src_regs[d], opt):
            skip = skips(wl, opt, a, src_regs[mate])
            for r in range(4):
                if not skip[r]:
                    ok, rb, re, is_rev = window(wl, opt, contigs, a, len(wl["reads"][mate]), r)
                    if ok:
                        out[a["src"], r] = task_of(wl, opt, mate, rb, re, is_rev)
    return out


def new_counts():
    return dict(pairs=0, anchors=0, alns=0, pushed=0, rounds=0, tasks_first=0, tasks=0, late=0, pen_cut=0, max_cut=0, clamped=0, other_contig=0,
                short=0, status1=0, status2=0, equal_existing=0, rev_anchor_push=0, into_empty=0, proper_dirs=0, unused=0, shrank=0,
                byte_tasks=0, word_tasks=0, two_live_push=0, late_pairs=[])


def rescue(wl, aligner, name="fr", stop_after_round_1=False):
    """-> (the regions of every read laid end to end, out_start, n_sw per pair, counts).  stop_after_round_1: the host of the old
    recipe, which never sends a second round: an orientation it has no result for is passed over as if it had not run."""
    opt, contigs = options(name, wl.get("contigs", CONTIGS))
    cnt = new_counts()
    n_reads = len(wl["reads"])
    src_regs, at = [], 0
    for regs in wl["regs"]:
        src_regs.append([dict(g, src=at + k) for k, g in enumerate(regs)])
        at += len(regs)
    known = first_round(wl, opt, contigs, src_regs)
    cnt["tasks_first"] = cnt["tasks"] = len(known)
    reached = set()
    final = [[dict(g) for g in regs] for regs in src_regs]
    n_sw = [0] * (n_reads // 2)
    stalls = [0] * n_reads
    cnt["pairs"] = n_reads // 2
    for d in range(n_reads):
        mate = d ^ 1
        l_ms = len(wl["reads"][mate])
        if not src_regs[d]:
            continue
        anchors = anchors_of(src_regs[d], opt, cnt)
        cnt["anchors"] += len(anchors)
        ma = [dict(g) for g in src_regs[mate]]
        ran_any = False
        for ai, a in enumerate(anchors):
            skip = skips(wl, opt, a, ma)
            if all(skip):
                continue
            n = 0
            for r in range(4):
                if skip[r]:
                    continue
                ok, rb, re, is_rev = window(wl, opt, contigs, a, l_ms, r, cnt)
                if ok:
                    key = (a["src"], r)
                    if key not in known:                        # the loop has reached a window round 1 did not send
                        if stop_after_round_1:
                            ok = False
                        else:
                            stalls[d] += 1
                            asked = {key: task_of(wl, opt, mate, rb, re, is_rev)}
                            for r2 in range(r + 1, 4):
                                if not skip[r2]:
                                    ok2, rb2, re2, rev2 = window(wl, opt, contigs, a, l_ms, r2)
                                    if ok2 and (a["src"], r2) not in known:
                                        asked[a["src"], r2] = task_of(wl, opt, mate, rb2, re2, rev2)
                            for a3 in anchors[ai + 1:]:
                                skip3 = skips(wl, opt, a3, ma)
                                for r3 in range(4):
                                    if not skip3[r3] and (a3["src"], r3) not in known:
                                        ok3, rb3, re3, rev3 = window(wl, opt, contigs, a3, l_ms, r3)
                                        if ok3:
                                            asked[a3["src"], r3] = task_of(wl, opt, mate, rb3, re3, rev3)
                            known.update(asked)
                            cnt["tasks"] += len(asked)
                            cnt["late"] += len(asked)
                            cnt["late_pairs"].append(d >> 1)
                if ok:
                    t = task_of(wl, opt, mate, rb, re, is_rev)
                    reached.add((a["src"], r))
                    cnt["byte_tasks" if t[4] & 0x10000 else "word_tasks"] += 1
                    res = aligner(*t)
                    cnt["status1"] += res["status"] == 1
                    cnt["status2"] += res["status"] == 2
                    if res["status"] != 1:
                        n += 1
                        ran_any = True
                    if res["status"] == 0:
                        b = dict(rb=res["rb"], re=res["re"], qb=res["qb"], qe=res["qe"], score=res["score"], truesc=0, w=0, seedcov=res["seedcov"],
                                 sub=0, csub=res["csub"], rid=a["rid"], n_comp=0, read=mate, src=NEW | a["src"])
                        cnt["pushed"] += 1
                        cnt["into_empty"] += not ma
                        cnt["rev_anchor_push"] += a["rb"] >= wl["l_pac"]
                        cnt["two_live_push"] += r == 0
                        cnt["equal_existing"] += any((m["score"], m["rb"], m["qb"]) == (b["score"], b["rb"], b["qb"]) for m in ma)
                        i = next((i for i, m in enumerate(ma) if m["score"] < b["score"]), len(ma))
                        ma.insert(i, b)
                if n > 0:
                    before = len(ma)
                    ma, _ = S.sdp_read(ma, mate, None, S.new_counts(), mlr=opt["mask_level_redun"], gap=opt["max_chain_gap"], patch=False)
                    cnt["shrank"] += len(ma) < before
            n_sw[d >> 1] += n
            cnt["alns"] += n
        cnt["proper_dirs"] += not ran_any and bool(src_regs[mate]) and not any((a["src"], r) in known for a in anchors for r in range(4))
        final[mate] = ma
    cnt["unused"] = len(set(known) - reached)
    cnt["rounds"] = (1 + max(stalls)) if cnt["tasks_first"] else 0
    out, start = [], [0]
    for regs in final:
        out += regs
        start.append(len(out))
    return out, start, n_sw, cnt


def same_stats(st, cnt, n_in, n_out):
    want = dict(pairs=cnt["pairs"], anchors=cnt["anchors"], rounds=cnt["rounds"], tasks_first=cnt["tasks_first"], tasks=cnt["tasks"],
                alns_bwa=cnt["alns"], pushed=cnt["pushed"], regs_in=n_in, regs_out=n_out, late=cnt["late"])
    return None if st == want else "stats %r, the restatement has %r" % (st, want)


def answer(host, aligner, tasks):
    """what the rescue ticket would write for these RD_MTASK records"""
    res = np.zeros(len(tasks), dtype=host.MRESULT)
    for k, t in enumerate(tasks):
        r = aligner(int(t["read"]), int(t["is_rev"]), int(t["rb"]), int(t["re"]), int(t["xtra"]), int(t["min_score"]))
        for f in M.ALN:
            res[k]["aln"][f] = r["aln"][f]
        for f in ("status", "rb", "re", "qb", "qe", "score", "csub", "seedcov"):
            res[k][f] = r[f]
    return res


# ---- the seeded workload -----------------------------------------------------------------------------------------------------------

def make_genome(seed=77):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, L_PAC).astype(np.uint8)
    for x1 in LATE_SITES:
        g[x1 - 300:x1 - 200] = g[x1 + 6:x1 + 106]
    return dict(l_pac=L_PAC, both=np.concatenate([g, 3 - g[::-1]]).astype(np.uint8), pac=gc.pack_pac(g), contigs=CONTIGS)


def rid_of(c):
    f = c if c < L_PAC else 2 * L_PAC - 1 - c
    return next(k for k, (o, n) in enumerate(CONTIGS) if o <= f < o + n)


def reg(c, n, read, score=None, qb=0, rid=None):
    """a region of n bases at bwa coordinate c"""
    return S.region(c, c + n, qb, qb + n, n if score is None else score, read, rid_of(c) if rid is None else rid)


def make_workload(n100=96, n_long=8, long_len=250, seed=2718):
    """pairs of 100-base reads (KSW_XBYTE) and of long_len-base reads (250: the 16-bit path), FR pairs off both strands: proper
    pairs, mates without a region, two anchors a few bases apart, junk mates, decoy regions, same-strand pairs (rescued only with
    FF live), an anchor beyond pen_unpaired; then the cases built by hand (`hand`)."""
    g = make_genome()
    L, both = g["l_pac"], g["both"]
    rng = np.random.default_rng(seed)
    reads, regs, hand = [], [], {}

    def at(c, n, subs=0):
        s = both[c:c + n].copy()
        for i in rng.choice(n, subs, replace=False) if subs else ():
            s[i] = (s[i] + 1 + rng.integers(0, 3)) % 4
        return np.ascontiguousarray(s, dtype=np.uint8)

    def junk(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    def mate_coord(x, n, dist, same_strand=False):
        """the coordinate of an n-base mate whose bsw_infer_dir distance from an anchor at x is dist"""
        if same_strand:
            return x + dist
        return 2 * L - 1 - (x + dist)                           # p2 = x + dist is 2L - 1 - rb of the mate

    def pair(a_read, a_regs, m_read, m_regs, name=None):
        k = len(reads)
        for g_ in a_regs:
            g_["read"] = k
        for g_ in m_regs:
            g_["read"] = k + 1
        reads.extend([a_read, m_read])
        regs.extend([a_regs, m_regs])
        if name:
            hand[name] = k // 2
        return k

    def spot(n, strand=None):
        """an anchor coordinate with HIGH + n bases of its contig on either side"""
        strand = int(rng.integers(0, 2)) if strand is None else strand
        o, ln = CONTIGS[int(rng.integers(0, 3))]
        margin = HIGH + n + 50
        f = int(rng.integers(o + margin, o + ln - margin))
        return f if strand == 0 else 2 * L - f - n

    def bulk(i, n):
        kind = i % 10
        x = spot(n, strand=1 if kind == 2 else None)
        m = mate_coord(x, n, int(rng.integers(LOW + 5, HIGH - 5)))
        subs = int(rng.integers(0, 5))
        a = [reg(x, n, 0)]
        if kind == 0:                                           # proper already
            pair(at(x, n), a, at(m, n, subs), [reg(m, n, 0, score=n - 5 * subs)])
        elif kind in (1, 2):                                    # the mate has no region; the anchor on either strand / the reverse
            pair(at(x, n), a, at(m, n, subs), [])
        elif kind == 3:                                         # two anchors three bases apart: the second finds the rescued mate in range
            a.append(S.region(x + 3, x + n, 3, n, n - 10, 0, rid_of(x)))
            pair(at(x, n), a, at(m, n, subs), [])
        elif kind == 4:                                         # nothing to find
            pair(at(x, n), a, junk(n), [])
        elif kind == 5:                                         # the mate's only region is a decoy elsewhere: both directions rescue
            dcy = spot(n)
            pair(at(x, n), a, at(m, n, subs), [reg(dcy, n, 0, score=40)])
        elif kind == 6:                                         # a partial region of the mate in range already
            pair(at(x, n), a, at(m, n, subs), [S.region(m + 20, m + 60, 20, 60, 40, 0, rid_of(m))])
        elif kind == 7:                                         # a same-strand pair: found only with FF live
            m = mate_coord(x, n, int(rng.integers(LOW + 5, HIGH - 5)), same_strand=True)
            pair(at(x, n), a, at(m, n, subs), [])
        elif kind == 8:                                         # a second region beyond pen_unpaired
            a.append(reg(spot(n), n, 0, score=n - 40))
            pair(at(x, n), a, at(m, n, subs), [])
        else:                                                   # both reads carry their true region, 40 bases too far apart
            far = mate_coord(x, n, HIGH + 40)
            pair(at(x, n), a, at(far, n), [reg(far, n, 0)])

    for i in range(n100):
        bulk(i, 100)
    for i in range(n_long):
        bulk((1, 2, 0, 1, 4, 3, 1, 5)[i % 8], long_len)

    # ---- by hand (100 bases, exact mates) ----
    # the late case: Rlow (a piece of the mate, dist 95: out of range for a1) is killed as redundant by the rescued full-length
    # region (dist 105); a2 = a1 - 400 had only Rlow in range (495; the full-length one is at 505), and its window holds the copy
    for x1 in LATE_SITES:
        m = mate_coord(x1, 100, 105)
        pair(at(x1, 100), [reg(x1, 100, 0), reg(x1 - 400, 100, 0, score=90)], at(m, 100), [S.region(m + 10, m + 50, 10, 50, 40, 0, rid_of(m))],
             name="late" if x1 == LATE_SITES[0] else None)
    x = 8000                                                    # the same rescued region twice: dist 105 from a1, 99 from a2 (window, not range)
    m = mate_coord(x, 100, 105)
    pair(at(x, 100), [reg(x, 100, 0), S.region(x + 6, x + 100, 6, 100, 90, 0, 0)], at(m, 100), [], name="equal")
    x = 20000 - 300                                             # the window is cut at the end of contig 0; the mate lies inside
    m = mate_coord(x, 100, 219)
    pair(at(x, 100), [reg(x, 100, 0)], at(m, 100), [], name="clamp")
    x = 20000 - 120                                             # mid of the window lies in contig 1
    pair(at(x, 100), [reg(x, 100, 0)], junk(100), [], name="other_contig")
    pair(junk(100), [S.region(2 * L - 12, 2 * L - 2, 0, 10, 10, 0, 0)], junk(100), [], name="short")      # 12 bases of window left
    x = L - 300                                                 # the window bridges l_pac: status 1 without a contig table
    m = mate_coord(x, 100, 249)
    pair(at(x, 100), [reg(x, 100, 0)], at(m, 100), [], name="bridge")
    x = 30000                                                   # three anchors for max_matesw = 1
    m = mate_coord(x, 100, 300)
    pair(at(x, 100), [reg(x, 100, 0), S.region(x + 2, x + 100, 2, 100, 95, 0, 1), S.region(x + 4, x + 100, 4, 100, 93, 0, 1)], at(m, 100), [], name="many")
    wl = dict(g)
    wl.update(reads=reads, regs=regs, hand=hand)
    return wl
