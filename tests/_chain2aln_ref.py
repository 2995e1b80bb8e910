"""mem_chain2aln restated sequentially in Python (bwamem.c of bwa 0.7.12 - 0.7.17 as recalled; bwa's source is not in the tree), and
the seeded workload its tests and tools/chain2aln_rate.py share.  TEST INFRASTRUCTURE: the yardstick for bsw_chain2aln_plan /
bsw_chain2aln_replay and the job built on them; nothing here calls them.

The reference walks bwa's loop read by read and chain by chain and extends a seed (through the CPU oracle: oracle.pair_batch for
variants H and M, _rtl_ref.pair_batch for RTL) ONLY when the loop reaches it unskipped.  Targets are cut from `both`, the
reference in bwa's coordinates (forward strand, then its reverse complement): what bsw_pac_get_seq returns for an interval that
does not bridge l_pac.

A workload is a dict: l_pac, both, pac, reads (uint8 arrays), chains (list of dicts read / seeds [(rbeg, qbeg, len, score)] /
rlo / rhi / rid / frac_rep, sorted by read)."""
import numpy as np


def pen_of(params):
    p = params[0] if getattr(params, "shape", None) else params
    return dict(a=int(p["mat"][0]), o_del=int(p["o_del"]), e_del=int(p["e_del"]), o_ins=int(p["o_ins"]), e_ins=int(p["e_ins"]), w=int(p["w"]))


def cal_max_gap(pen, qlen):
    l_del = int(float(qlen * pen["a"] - pen["o_del"]) / pen["e_del"] + 1.)
    l_ins = int(float(qlen * pen["a"] - pen["o_ins"]) / pen["e_ins"] + 1.)
    l = max(l_del, l_ins, 1)
    return min(l, pen["w"] << 1)


def chain_window(pen, seeds, l_query, l_pac, rlo=0, rhi=0):
    """-> (rmax0, rmax1, bridge_clamped, contig_clamped)"""
    r0, r1 = l_pac << 1, 0
    for rbeg, qbeg, ln, _ in seeds:
        rq = l_query - qbeg - ln
        r0 = min(r0, rbeg - (qbeg + cal_max_gap(pen, qbeg)))
        r1 = max(r1, rbeg + ln + (rq + cal_max_gap(pen, rq)))
    r0, r1 = max(r0, 0), min(r1, l_pac << 1)
    bridged = r0 < l_pac < r1
    if bridged:
        if seeds[0][0] < l_pac:
            r1 = l_pac
        else:
            r0 = l_pac
    clamped = False
    if rhi > rlo:
        clamped = r0 < rlo or r1 > rhi
        r0, r1 = max(r0, rlo), min(r1, rhi)
    return r0, r1, bridged, clamped


def build_tasks(host, pen, reads, both, items):
    """items: (read index, rbeg, qbeg, len, rmax0, rmax1, tag) -> (TASK array, arena): what bsw_seed_to_task lays out"""
    parts, offs, at = [], [], 0
    for ri, rbeg, qbeg, ln, r0, r1, _ in items:
        q = reads[ri]
        four = (q[:qbeg][::-1], both[r0:rbeg][::-1], q[qbeg + ln:], both[rbeg + ln:r1])
        if qbeg == 0:
            four = (four[0], four[1][:0], four[2], four[3])
        if qbeg + ln == len(q):
            four = (four[0], four[1], four[2], four[3][:0])
        for x in four:
            parts.append(x)
            offs.append(at)
            at += len(x)
    arena = np.concatenate(parts + [np.zeros(8, np.uint8)]).astype(np.uint8)
    t = np.zeros(len(items), dtype=host.TASK)
    base = arena.ctypes.data
    o = np.array(offs, dtype=np.uint64).reshape(-1, 4) + np.uint64(base)
    ln4 = np.array([len(x) for x in parts], dtype=np.int32).reshape(-1, 4)
    for k, (pf, lf) in enumerate((("lquery", "lqlen"), ("ltarget", "ltlen"), ("rquery", "rqlen"), ("rtarget", "rtlen"))):
        t[pf] = np.where(ln4[:, k] > 0, o[:, k], 0)
        t[lf] = ln4[:, k]
    t["h0"] = [it[3] * pen["a"] for it in items]
    t["init_score"] = -1
    t["qbeg"] = [it[2] for it in items]
    t["tag"] = [it[6] for it in items]
    return t, arena


def run_oracle(oracle, rtl, params, tasks, nthreads=1):
    if int(params["variant"][0]) == 2:
        return rtl.pair_batch(params, tasks)
    return oracle.pair_batch(params, tasks, nthreads=nthreads)


class Extender:
    """one seed through the CPU oracle, on demand"""
    def __init__(self, host, oracle, rtl, params, wl):
        self.host, self.oracle, self.rtl, self.params, self.wl, self.pen, self.calls = host, oracle, rtl, params, wl, pen_of(params), 0

    def __call__(self, ri, seed, r0, r1, tag):
        t, keep = build_tasks(self.host, self.pen, self.wl["reads"], self.wl["both"], [(ri, seed[0], seed[1], seed[2], r0, r1, tag)])
        self.calls += 1
        return run_oracle(self.oracle, self.rtl, self.params, t)[0]


def explains(pen, p, s, l_query, seedlen0_frac, why=None):
    rbeg, qbeg, ln, _ = s
    if rbeg < p["rb"] or rbeg + ln > p["re"] or qbeg < p["qb"] or qbeg + ln > p["qe"]:
        return False
    if seedlen0_frac >= 0 and ln - p["seedlen0"] > seedlen0_frac * l_query:
        if why is not None:
            why["seedlen0"] = True
        return False
    qd, rd = qbeg - p["qb"], rbeg - p["rb"]
    w = min(cal_max_gap(pen, min(qd, rd)), p["w"])
    if qd - rd < w and rd - qd < w:
        return True
    qd, rd = p["qe"] - (qbeg + ln), p["re"] - (rbeg + ln)
    w = min(cal_max_gap(pen, min(qd, rd)), p["w"])
    return qd - rd < w and rd - qd < w


def chain2aln(extend, params, wl, seedlen0_frac=.1, ovl_len_frac=.95):
    """-> (regions in push order, the reads in order; extended flag per seed; counters of what the workload exercised)"""
    pen, l_pac = pen_of(params), wl["l_pac"]
    regs, extended = [], []
    cnt = dict(seeds=0, extended=0, rescued=0, cross_chain_skips=0, seedlen0_exempt=0, clamped=0, bridged=0, qbeg0=0, qend=0)
    first, av, av_read = 0, [], None
    for ci, ch in enumerate(wl["chains"]):
        ri, seeds = ch["read"], ch["seeds"]
        lq = len(wl["reads"][ri])
        if ri != av_read:
            av, av_read = [], ri
        r0, r1, bridged, clamped = chain_window(pen, seeds, lq, l_pac, ch["rlo"], ch["rhi"])
        cnt["bridged"] += bridged
        cnt["clamped"] += clamped
        n = len(seeds)
        srt = sorted((seeds[i][3] << 32) | i for i in range(n))
        ext_here = [False] * n
        for k in range(n - 1, -1, -1):
            si = srt[k] & 0xffffffff
            s = seeds[si]
            cnt["seeds"] += 1
            cnt["qbeg0"] += s[1] == 0
            cnt["qend"] += s[1] + s[2] == lq
            why = {}
            by = next((p for p in av if explains(pen, p, s, lq, seedlen0_frac, why)), None)
            if by is not None:
                rescued = False
                for i in range(k + 1, n):
                    if srt[i] == 0:
                        continue
                    t = seeds[srt[i] & 0xffffffff]
                    if t[2] < s[2] * ovl_len_frac:
                        continue
                    if s[1] <= t[1] and s[1] + s[2] - t[1] >= s[2] >> 2 and t[1] - s[1] != t[0] - s[0]:
                        rescued = True
                        break
                    if t[1] <= s[1] and t[1] + t[2] - s[1] >= s[2] >> 2 and s[1] - t[1] != s[0] - t[0]:
                        rescued = True
                        break
                if not rescued:
                    srt[k] = 0
                    cnt["cross_chain_skips"] += by["chain"] != ci
                    continue
                cnt["rescued"] += 1
            elif why.get("seedlen0"):
                cnt["seedlen0_exempt"] += 1
            r = extend(ri, s, r0, r1, first + si)
            a = dict(rb=s[0] + int(r["rb"]), re=s[0] + s[2] + int(r["re"]), qb=int(r["qb"]), qe=s[1] + s[2] + int(r["qe"]), score=int(r["score"]),
                     truesc=int(r["truesc"]), w=int(r["w"]), seedlen0=s[2], rid=ch["rid"], frac_rep=float(np.float32(ch["frac_rep"])),
                     read=ri, chain=ci, seed=first + si)
            a["seedcov"] = sum(t[2] for t in seeds if t[1] >= a["qb"] and t[1] + t[2] <= a["qe"] and t[0] >= a["rb"] and t[0] + t[2] <= a["re"])
            av.append(a)
            regs.append(a)
            ext_here[si] = True
            cnt["extended"] += 1
        extended += ext_here
        first += n
    return regs, extended, cnt


REG_FIELDS = ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "seedlen0", "rid", "frac_rep", "read", "chain", "seed")


def same_regions(got, want):
    """got: CREG array, want: the reference's list -> None, or the first difference"""
    if len(got) != len(want):
        return "regions: %d, the reference has %d" % (len(got), len(want))
    for f in REG_FIELDS:
        w = np.array([a[f] for a in want], dtype=got.dtype[f]) if want else np.zeros(0, dtype=got.dtype[f])
        bad = np.nonzero(got[f] != w)[0]
        if len(bad):
            i = int(bad[0])
            return "region %d field %s: %r, the reference has %r (%r)" % (i, f, got[f][i], w[i], want[i])
    return None


def arrays(host, wl):
    """-> (CHAIN array, CSEED array, lens)"""
    ch = np.zeros(len(wl["chains"]), dtype=host.CHAIN)
    sd = np.zeros(sum(len(c["seeds"]) for c in wl["chains"]), dtype=host.CSEED)
    at = 0
    for i, c in enumerate(wl["chains"]):
        ch[i] = (c["read"], len(c["seeds"]), at, c["rlo"], c["rhi"], c["rid"], c["frac_rep"])
        for s in c["seeds"]:
            sd[at] = (s[0], s[1], s[2], s[3], 0)
            at += 1
    return ch, sd, np.array([len(r) for r in wl["reads"]], dtype=np.int32)


# ---- the seeded workload -----------------------------------------------------------------------------------------------------------

CONTIGS = (0, 50000, 120001)          # contig offsets on the forward strand; the last contig ends at l_pac
L_PAC = 200003


def make_genome(seed=20240):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, L_PAC).astype(np.uint8)
    b4 = np.concatenate([g, np.zeros((-L_PAC) % 4, np.uint8)]).reshape(-1, 4)
    pac = (b4[:, 0] << 6 | b4[:, 1] << 4 | b4[:, 2] << 2 | b4[:, 3]).astype(np.uint8)
    return dict(l_pac=L_PAC, both=np.concatenate([g, 3 - g[::-1]]).astype(np.uint8), pac=pac)


def contig_of(pos, l_pac=L_PAC):
    """the contig interval of a position in [0, 2*l_pac) coordinates, and its index"""
    f = pos if pos < l_pac else 2 * l_pac - 1 - pos
    k = max(i for i, o in enumerate(CONTIGS) if o <= f)
    lo, hi = CONTIGS[k], (CONTIGS[k + 1] if k + 1 < len(CONTIGS) else l_pac)
    return ((lo, hi) if pos < l_pac else (2 * l_pac - hi, 2 * l_pac - lo)), k


def make_workload(n_reads, seed, len_lo=100, len_hi=250, genome=None, min_seed=12):
    """reads of len_lo .. len_hi bases off both strands with substitutions and at most one indel; 1 - 5 chains each: the true
    locus (its exact-match segments as seeds, some cut in two; behind an indel a seed of the other diagonal reaching back over
    the cut), sometimes a one-seed chain in front of it or a thinned copy behind it, decoy chains at random loci; every tenth
    read at a contig edge with the contig interval set, every tenth where the window would bridge l_pac."""
    g = genome or make_genome()
    L, both = g["l_pac"], g["both"]
    rng = np.random.default_rng(seed)
    reads, chains = [], []
    for i in range(n_reads):
        Lr = int(rng.integers(len_lo, len_hi + 1))
        kind = i % 10
        d = int(rng.integers(1, 5)) if rng.random() < 0.45 else 0
        ins = bool(rng.integers(0, 2))
        span = Lr + (d if not ins else 0) + 2
        strand = int(rng.integers(0, 2))
        edge = int(rng.integers(0, 25))
        if kind == 6:                                           # at a contig edge
            (lo, hi), _ = contig_of(int(rng.integers(0, L)) + strand * L)
            pos = lo + edge if rng.integers(0, 2) else hi - span - edge
        elif kind == 7:                                         # the window would bridge l_pac
            pos = L - span - edge if strand == 0 else L + edge
        else:
            pos = int(rng.integers(400, L - 400 - span)) + strand * L
            if contig_of(pos)[1] != contig_of(pos + span)[1]:
                pos -= span + 300                               # inside one contig
        cut = int(rng.integers(30, Lr - 30)) if d else Lr
        tmpl = both[pos:pos + span]
        if d and ins:
            r = np.concatenate([tmpl[:cut], rng.integers(0, 4, d).astype(np.uint8), tmpl[cut:]])[:Lr]
            cut2, shift = cut + d, -d                           # read[q] = ref[pos + q + shift] for q >= cut2
        elif d:
            r = np.concatenate([tmpl[:cut], tmpl[cut + d:]])[:Lr]
            cut2, shift = cut, d
        else:
            r = tmpl[:Lr].copy()
            cut2, shift = Lr, 0
        r = r.astype(np.uint8)
        subs = np.nonzero(rng.random(Lr) < rng.choice([0.01, 0.03, 0.05]))[0]
        r[subs] = (r[subs] + 1 + rng.integers(0, 3, len(subs))) % 4
        reads.append(r)
        # exact-match segments of the true alignment
        brk = sorted(set(int(x) for x in subs) | set(range(cut, cut2)))
        segs, a = [], 0
        for b in brk + [Lr]:
            for lo_, hi_ in ((a, min(b, cut)), (max(a, cut2), b)):
                if hi_ - lo_ >= min_seed:
                    segs.append((lo_, hi_ - lo_))
            a = b + 1
        if not segs:
            segs.append((0, min_seed))                          # (bwa would have no chain; a seed need not match)
        true = []
        for qb, ln in segs:
            sh = shift if qb >= cut2 else 0
            if ln >= 30 and rng.random() < 0.7:                 # re-seeding: two seeds over one segment, sometimes beside the whole
                m = int(rng.integers(12, ln - 12))
                ov = int(rng.integers(0, 8))
                true += [(pos + qb + sh, qb, m + ov), (pos + qb + m + sh, qb + m, ln - m)]
                if rng.random() < 0.4:
                    true.append((pos + qb + sh, qb, ln))
            else:
                true.append((pos + qb + sh, qb, ln))
        if d:                                                   # behind the indel: a seed of that diagonal reaching back over the cut
            post = [s for s in true if s[1] >= cut2]
            if post:
                rb, qb, ln = post[0]
                m = min(int(rng.integers(5, 28)), qb)
                true.append((rb - m, qb - m, ln + m))
        mode = int(rng.integers(0, 4))
        def scored(ss):
            if mode == 0:
                return [(rb, qb, ln, int(rng.integers(10, 61))) for rb, qb, ln in ss]      # scores unrelated to the lengths
            if mode == 1:
                return [(rb, qb, ln, max(ln - int(rng.integers(0, 3)), 0)) for rb, qb, ln in ss]
            return [(rb, qb, ln, ln) for rb, qb, ln in ss]                                  # score = len
        order = rng.permutation(len(true))
        main = scored([true[j] for j in order])
        (clo, chi), rid = contig_of(pos)
        setc = kind == 6 or (kind != 7 and bool(rng.integers(0, 2)))
        def chain(ss, here=True):
            return dict(read=i, seeds=ss, rlo=clo if (setc and here) else 0, rhi=chi if (setc and here) else 0, rid=rid if here else -1,
                        frac_rep=float(rng.integers(0, 9)) / 8)
        mine = []
        if rng.random() < 0.25:                                 # a one-seed chain in front: a short piece of a true seed
            rb, qb, ln = true[int(rng.integers(0, len(true)))]
            k = min(ln, int(rng.integers(12, 16)))
            mine.append(chain(scored([(rb, qb, k)])))
        if rng.random() < 0.2:
            mine.append(None)                                   # (a decoy in front of the true chain)
        mine.append(chain(main))
        if rng.random() < 0.5 and len(true) > 1:                # a thinned copy behind it
            keep = [true[j] for j in range(len(true)) if rng.random() < 0.6] or [true[0]]
            mine.append(chain(scored(keep)))
        while len(mine) < 5 and rng.random() < 0.45:
            mine.append(None)
        for c in mine[:5]:
            if c is None:                                       # a decoy: 1 - 3 colinear seeds at a random locus
                st = int(rng.integers(0, 2))
                rp = int(rng.integers(400, L - 400 - Lr)) + st * L
                ss, qb = [], int(rng.integers(0, 30))
                for _ in range(int(rng.integers(1, 4))):
                    ln = int(rng.integers(min_seed, 31))
                    if qb + ln > Lr:
                        break
                    ss.append((rp + qb, qb, ln))
                    qb += ln + int(rng.integers(0, 40))
                c = chain(scored(ss or [(rp, 0, min_seed)]), here=False)
            chains.append(c)
    wl = dict(g)
    wl.update(reads=reads, chains=chains)
    return wl
