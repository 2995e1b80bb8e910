"""GPU parity of bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch and bsw_matesw_ref_batch across the bounds of their
hosts' sub-batch loops: 2^20 tasks, 4 GiB of backtrack bytes, 2^28 sub-optimal list entries.  A batch on one side of a bound is
all the other tests run; here the second sub-batch gets res + a, cigars + a * max_cigar, md + a * max_md, its scratch offsets
start again at 0, and the first one's slices end at the bound.

Every batch cycles through D distinct tasks (D odd, neighbours of different lengths), so the expectation is D oracle answers
and result k is compared, in full and with numpy, with the answer of task k mod D.  What keeps a comparison from passing
vacuously is asserted on the ORACLE's answers before the library runs.  The 2^31 sequence-byte bound is not reached here (it
needs about 2 GiB of pinned staging and 3 GiB on the device for one call).  Measured on an MI355X: 0.6 to 1.6 s per test."""
import numpy as np
import pytest

import _gen
import _gencigar_ref as gc
import _matesw_ref as mr

pytestmark = pytest.mark.gpu

L_PAC = 700_001
INT_MIN = -(1 << 31)
XBYTE, XSUBO, XSTART = 0x10000, 0x40000, 0x80000
COUNT = (1 << 20) + 37


@pytest.fixture(scope="module")
def genome(ctx):
    rng = np.random.default_rng(4242)
    bases = rng.integers(0, 4, L_PAC).astype(np.uint8)
    pac = gc.pack_pac(bases)
    ref = ctx.ref_upload(pac, L_PAC)
    yield pac, ref, bases
    ctx.ref_free(ref)


def pen_of(p):
    return int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0])


def cycle(distinct, n):
    return np.ascontiguousarray(distinct[np.arange(n) % len(distinct)])


# ---- global ------------------------------------------------------------------------------------------------------------------
def gtasks_of(host, pairs, ws):
    gt = np.zeros(len(pairs), dtype=host.GTASK)
    for i, ((q, t), w) in enumerate(zip(pairs, ws)):
        gt[i]["query"], gt[i]["target"], gt[i]["qlen"], gt[i]["tlen"], gt[i]["w"] = q.ctypes.data, t.ctypes.data, len(q), len(t), w
    return gt


def check_global(host, oracle, ctx, pairs, ws, n, max_cigar, min_ops=0):
    p = host.default_params()
    D = len(pairs)
    assert D % 2 == 1
    want = [oracle.global2(q, t, p["mat"][0], *pen_of(p), w) for (q, t), w in zip(pairs, ws)]
    assert all(w >= abs(len(q) - len(t)) for (q, t), w in zip(pairs, ws))          # no task under the band-too-narrow exemption
    assert all(len(x["cigar"]) <= max_cigar for x in want)
    if min_ops:
        assert sum(1 for x in want if len(x["cigar"]) >= min_ops) * 2 >= D, [len(x["cigar"]) for x in want]
    e_score = np.array([x["score"] for x in want], dtype=np.int32)
    e_n = np.array([len(x["cigar"]) for x in want], dtype=np.int32)
    e_cig = np.zeros((D, max_cigar), dtype=np.uint32)
    for i, x in enumerate(want):
        e_cig[i, :e_n[i]] = [ln << 4 | op for op, ln in x["cigar"]]
    res, cig = ctx.global_batch(p, cycle(gtasks_of(host, pairs, ws), n), max_cigar=max_cigar)
    idx = np.arange(n) % D
    bad = np.nonzero((res["score"] != e_score[idx]) | (res["n_cigar"] != e_n[idx]))[0]
    assert len(bad) == 0, [(int(k), int(k % D), int(res["score"][k]), int(e_score[k % D]), int(res["n_cigar"][k]), int(e_n[k % D])) for k in bad[:5]]
    mask = np.arange(max_cigar)[None, :] < e_n[idx][:, None]
    bad = np.nonzero(((cig != e_cig[idx]) & mask).any(axis=1))[0]
    assert len(bad) == 0, [(int(k), int(k % D)) for k in bad[:5]]


def tiny_pairs(rng, bases, D):
    pairs, ws = [], []
    for i in range(D):
        ql, tl = 1 + (i * 3) % 8, 1 + (i * 5 + 2) % 10
        at = int(rng.integers(0, len(bases) - 40))
        q = bases[at + i % 2:at + i % 2 + ql].copy()
        if i % 3 == 0:
            q[len(q) // 2] = (q[len(q) // 2] + 1) & 3
        pairs.append((q, bases[at:at + tl].copy()))
        ws.append(abs(ql - tl) + 3)
    return pairs, ws


def test_global_batch_of_more_than_2_20_tasks(host, oracle, ctx, genome):
    rng = np.random.default_rng(1)
    pairs, ws = tiny_pairs(rng, genome[2], 11)
    check_global(host, oracle, ctx, pairs, ws, COUNT, 8)


def long_pairs(rng, bases, D, length, step, indel=0.002):
    pairs = []
    for i in range(D):
        tl = length - i * step
        at = int(rng.integers(0, len(bases) - tl))
        t = bases[at:at + tl].copy()
        pairs.append((_gen.mutate(rng, t, tl - (i % 3) * 2, 0.01, indel), t))
    return pairs


def test_global_batch_of_more_than_4_gib_of_backtrack_in_the_ring_kernel(host, oracle, ctx, genome):
    """141 alignments of 8 000 bases with w = 2 000: 4 001 x 8 000 backtrack bytes each, 4.5 GB."""
    rng = np.random.default_rng(2)
    pairs = long_pairs(rng, genome[2], 5, 8000, 3)
    n = 141
    assert sum(min(len(pairs[k % 5][0]), 4001) * len(pairs[k % 5][1]) for k in range(n)) > 4 << 30
    check_global(host, oracle, ctx, pairs, [2000] * 5, n, 512, min_ops=3)


def test_global_batch_of_more_than_4_gib_of_backtrack_in_the_register_kernel(host, oracle, ctx, genome):
    """4 500 alignments of about 1 000 bases with w = 500: about 1 MB of backtrack bytes each."""
    rng = np.random.default_rng(3)
    pairs = long_pairs(rng, genome[2], 7, 1020, 4, indel=0.006)
    assert all(len(q) <= 1023 for q, _ in pairs)
    n = 4500
    assert sum(min(len(pairs[k % 7][0]), 1001) * len(pairs[k % 7][1]) for k in range(n)) > 4 << 30
    check_global(host, oracle, ctx, pairs, [500] * 7, n, 128, min_ops=3)


# ---- local alignment -----------------------------------------------------------------------------------------------------------
def atasks_of(host, pairs, xtras):
    at = np.zeros(len(pairs), dtype=host.ATASK)
    for i, ((q, t), x) in enumerate(zip(pairs, xtras)):
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = q.ctypes.data, t.ctypes.data, len(q), len(t), x
    return at


def planted(rng, bases, ql, tl, copies):
    at = int(rng.integers(0, len(bases) - tl))
    t = bases[at:at + tl].copy()
    off = int(rng.integers(0, tl - ql + 1))
    q = t[off:off + ql].copy()
    for _ in range(copies):                                   # planted repeats of the query: score2, and a start to find
        o = int(rng.integers(0, tl - ql + 1))
        t[o:o + ql] = q
    return q, t


def subo_shares(aln, xtras):
    """on the oracle's answers: at least a quarter of the KSW_XSUBO tasks have score2 >= 0, at least a quarter tb >= 0"""
    subo = [a for a, x in zip(aln, xtras) if x & XSUBO]
    assert 0 < len(subo) < len(xtras)                          # a few tasks without KSW_XSUBO in between
    assert sum(1 for a in subo if a[3] >= 0) * 4 >= len(subo), aln
    assert sum(1 for a in subo if a[5] >= 0) * 4 >= len(subo), aln


def check_align(host, oracle, ctx, pairs, xtras, n, shares=True):
    p = host.default_params()
    D = len(pairs)
    assert D % 2 == 1
    at = atasks_of(host, pairs, xtras)
    want, _ = oracle.align2_batch(p["mat"][0], *pen_of(p), at, nthreads=8)
    if shares:
        subo_shares(want.tolist(), xtras)
    res = ctx.align_batch(p, cycle(at, n))
    got = np.stack([res[k] for k in mr.ALN], axis=1)
    bad = np.nonzero((got != want[np.arange(n) % D]).any(axis=1))[0]
    assert len(bad) == 0, [(int(k), int(k % D), got[k].tolist(), want[k % D].tolist()) for k in bad[:5]]


def test_align_batch_of_more_than_2_20_tasks(host, oracle, ctx, genome):
    rng = np.random.default_rng(4)
    pairs = [planted(rng, genome[2], 1 + (i * 3) % 8, 9 + (i * 7) % 30, 2) for i in range(11)]
    xtras = [XSUBO | XSTART | (XBYTE if i & 1 else 0) | (4 if len(pairs[i][0]) > 4 else 1) for i in range(11)]
    check_align(host, oracle, ctx, pairs, xtras, COUNT, shares=False)


B_N = 4651                       # 8 of 9 distinct tasks carry KSW_XSUBO: 4 134 slices of about 65 532 entries, 270.9 M > 2^28


def b_xtras(qlens):
    x = [XSUBO | XSTART | (XBYTE if i & 1 else 0) | (10 if q > 30 else 4) for i, q in enumerate(qlens)]
    x[1] &= ~XSUBO               # the loop counts its target towards the bound and gives it no slice
    return x


def test_align_batch_of_more_than_2_28_suboptimal_list_entries(host, oracle, ctx, genome):
    rng = np.random.default_rng(5)
    qlens = [8, 150, 33, 250, 5, 120, 70, 200, 16]
    pairs = [planted(rng, genome[2], q, 65535 - (i % 2) * 7, 6) for i, q in enumerate(qlens)]
    xtras = b_xtras(qlens)
    assert sum(len(pairs[k % 9][1]) for k in range(B_N) if xtras[k % 9] & XSUBO) > 1 << 28
    check_align(host, oracle, ctx, pairs, xtras, B_N)


# ---- bwa_gen_cigar2 on the resident reference ---------------------------------------------------------------------------------------
def check_cigar(host, oracle, ctx, genome, specs, n, max_cigar, max_md, min_ops=0, md_share=False):
    pac, ref, _ = genome
    p = host.default_params()
    D = len(specs)
    assert D % 2 == 1
    want = [gc.reg2aln(oracle, p["mat"][0], pen_of(p), L_PAC, pac, s["read"], s["rb"], s["re"], s["w"], s["w_cap"], s["min_score"], s["max_tries"])
            for s in specs]
    live = [w for w in want if not w["status"]]
    assert all(len(w["cigar"]) <= max_cigar and len(w["md"]) + 1 <= max_md for w in live)
    if min_ops:
        assert len(live) == D and sum(1 for w in live if len(w["cigar"]) >= min_ops) * 2 >= D, [len(w["cigar"]) for w in live]
    if md_share:
        assert sum(1 for w in live if any(c in w["md"] for c in "ACGT^")) * 4 >= D, [w.get("md") for w in want]
    ct = np.zeros(D, dtype=host.CTASK)
    for i, s in enumerate(specs):
        ct[i]["query"], ct[i]["l_query"], ct[i]["w"] = s["read"].ctypes.data, len(s["read"]), s["w"]
        ct[i]["rb"], ct[i]["re"], ct[i]["w_cap"], ct[i]["min_score"], ct[i]["max_tries"] = s["rb"], s["re"], s["w_cap"], s["min_score"], s["max_tries"]
    res, cig, md = ctx.cigar_ref_batch(p, ref, cycle(ct, n), max_cigar=max_cigar, max_md=max_md)
    idx = np.arange(n) % D
    e = np.zeros(D, dtype=host.CRESULT)
    e_cig = np.zeros((D, max_cigar), dtype=np.uint32)
    e_md = []
    for i, w in enumerate(want):
        e["w"][i], e["tries"][i], e["status"][i] = w["w"], w["tries"], w["status"]
        if w["status"]:
            e["nm"][i] = -1
            e_md.append("")
            continue
        e["score"][i], e["n_cigar"][i], e["nm"][i], e["md_len"][i] = w["score"], len(w["cigar"]), w["nm"], len(w["md"])
        e_cig[i, :len(w["cigar"])] = [ln << 4 | op for op, ln in w["cigar"]]
        e_md.append(w["md"])
    for f in ("score", "n_cigar", "nm", "md_len", "w", "tries", "status", "_pad"):
        bad = np.nonzero(res[f] != e[f][idx])[0]
        assert len(bad) == 0, (f, [(int(k), int(k % D), int(res[f][k]), int(e[f][k % D])) for k in bad[:5]])
    mask = np.arange(max_cigar)[None, :] < e["n_cigar"][idx][:, None]
    bad = np.nonzero(((cig != e_cig[idx]) & mask).any(axis=1))[0]
    assert len(bad) == 0, [(int(k), int(k % D)) for k in bad[:5]]
    bad = [k for k in range(n) if md[k] != e_md[k % D]]
    assert not bad, [(k, k % D, md[k], e_md[k % D]) for k in bad[:5]]


def cspec(read, rb, re, w=10, w_cap=0, min_score=INT_MIN, max_tries=1):
    return dict(read=np.ascontiguousarray(read, dtype=np.uint8), rb=int(rb), re=int(re), w=w, w_cap=w_cap, min_score=min_score, max_tries=max_tries)


def test_cigar_ref_batch_of_more_than_2_20_tasks(host, oracle, ctx, genome):
    pac = genome[0]
    rng = np.random.default_rng(6)
    specs = []
    for i in range(13):
        rl = 3 + (i * 3) % 8
        rb = (L_PAC if i % 2 else 0) + int(rng.integers(0, L_PAC - 20))
        re = rb + rl
        q = gc.bns_get_seq(pac, L_PAC, rb, re).copy()
        w = 10
        if i % 4 == 0 and len(q) > 4:
            q = np.delete(q, 2)
        if i % 4 == 1:
            q[len(q) // 2] = (q[len(q) // 2] + 2) & 3
        if i % 4 == 2 and len(q) > 3:
            q = np.insert(q, 1, (q[1] + 1) & 3)
        if i % 4 == 3:
            q[0] = (q[0] + 1) & 3
            w = 0                                               # the no-gap shortcut (when the lengths agree)
        if i == 5:
            rb, re = L_PAC - 3, L_PAC + 4                       # bridges l_pac: status 1
        specs.append(cspec(q[:8], rb, re, w=w))
    check_cigar(host, oracle, ctx, genome, specs, COUNT, 6, 24, md_share=True)


def long_reads(rng, pac, D, length, step, w, indel=0.002):
    specs = []
    for i in range(D):
        rl = length - i * step
        rb = (L_PAC if i % 2 else 0) + int(rng.integers(0, L_PAC - rl))
        specs.append(cspec(_gen.mutate(rng, gc.bns_get_seq(pac, L_PAC, rb, rb + rl), rl - (i % 3) * 2, 0.01, indel), rb, rb + rl, w=w))
    return specs


def z_need(p, specs, n):
    mat, pen = p["mat"][0], pen_of(p)
    tot = 0
    for k in range(n):
        s = specs[k % len(specs)]
        rl = s["re"] - s["rb"]
        tot += min(len(s["read"]), 2 * gc.band(mat, *pen, len(s["read"]), rl, (1 << 31) - 1) + 1) * rl
    return tot


def test_cigar_ref_batch_of_more_than_4_gib_of_backtrack_in_the_ring_kernel(host, oracle, ctx, genome):
    """141 reads of 8 000 bases, w = 3 000: bwa's formula gives the band 1 998, 3 997 x 8 000 backtrack bytes each; the
    slices of the first sub-batch end at the bound."""
    rng = np.random.default_rng(7)
    specs = long_reads(rng, genome[0], 5, 8000, 3, 3000)
    assert z_need(host.default_params(), specs, 141) > 4 << 30
    check_cigar(host, oracle, ctx, genome, specs, 141, 512, 2048, min_ops=3)


def test_cigar_ref_batch_of_more_than_4_gib_of_backtrack_in_the_register_kernel(host, oracle, ctx, genome):
    """9 000 reads of about 1 000 bases, w = 500: band 248, half a megabyte of backtrack bytes each."""
    rng = np.random.default_rng(8)
    specs = long_reads(rng, genome[0], 7, 1020, 4, 500, indel=0.006)
    assert all(len(s["read"]) <= 1023 for s in specs)
    assert z_need(host.default_params(), specs, 9000) > 4 << 30
    check_cigar(host, oracle, ctx, genome, specs, 9000, 128, 1024, min_ops=3)


# ---- mate rescue -------------------------------------------------------------------------------------------------------------------
def check_matesw(host, oracle, ctx, genome, specs, n, shares=True):
    pac, ref, _ = genome
    p = host.default_params()
    D = len(specs)
    assert D % 2 == 1
    want = mr.matesw_batch(oracle, host.ATASK, p["mat"][0], pen_of(p), L_PAC, pac, [s["mate"] for s in specs], [s["is_rev"] for s in specs],
                           [s["rb"] for s in specs], [s["re"] for s in specs], [s["xtra"] for s in specs], [s["min_score"] for s in specs], nthreads=8)
    if shares:
        subo_shares(want["aln"].tolist(), [s["xtra"] for s in specs])
        assert {s["is_rev"] for s in specs} == {0, 1}
    mt = np.zeros(D, dtype=host.MTASK)
    for i, s in enumerate(specs):
        mt[i]["mate"], mt[i]["l_ms"], mt[i]["is_rev"] = (s["mate"].ctypes.data if len(s["mate"]) else 0), len(s["mate"]), s["is_rev"]
        mt[i]["rb"], mt[i]["re"], mt[i]["xtra"], mt[i]["min_score"] = s["rb"], s["re"], s["xtra"], s["min_score"]
    res = ctx.matesw_ref_batch(p, ref, cycle(mt, n))
    idx = np.arange(n) % D
    got = np.stack([res["aln"][k] for k in mr.ALN], axis=1)
    bad = np.nonzero((got != want["aln"][idx]).any(axis=1))[0]
    assert len(bad) == 0, [(int(k), int(k % D), got[k].tolist(), want["aln"][k % D].tolist()) for k in bad[:5]]
    for f in ("status", "rb", "re", "qb", "qe", "score", "csub", "seedcov"):
        bad = np.nonzero(res[f] != np.asarray(want[f])[idx])[0]
        assert len(bad) == 0, (f, [(int(k), int(k % D), int(res[f][k]), int(want[f][k % D])) for k in bad[:5]])
    assert (res["_pad"] == 0).all()


def mate_specs(rng, pac, lens, tlen_of, xtras):
    specs = []
    for i, lm in enumerate(lens):
        tl = tlen_of(i)
        rb = (L_PAC if i % 3 == 1 else 0) + int(rng.integers(0, L_PAC - tl))
        win = gc.bns_get_seq(pac, L_PAC, rb, rb + tl)
        off = int(rng.integers(0, tl - lm + 1))
        aligned = win[off:off + lm].copy()
        is_rev = i % 2
        specs.append(dict(mate=np.ascontiguousarray(mr.revcomp(aligned) if is_rev else aligned), is_rev=is_rev, rb=rb, re=rb + tl, xtra=xtras[i],
                          min_score=min(lm, 19)))
    return specs


def test_matesw_ref_batch_of_more_than_2_20_tasks(host, oracle, ctx, genome):
    rng = np.random.default_rng(9)
    lens = [2 + (i * 3) % 7 for i in range(9)]
    xtras = [XSUBO | XSTART | (XBYTE if i & 1 else 0) | (4 if lens[i] > 4 else 2) for i in range(9)]
    specs = mate_specs(rng, genome[0], lens, lambda i: 12 + (i * 7) % 30, xtras)
    specs[4]["re"] = specs[4]["rb"]                             # an empty window: status 1
    check_matesw(host, oracle, ctx, genome, specs, COUNT, shares=False)


def test_matesw_ref_batch_of_more_than_2_28_suboptimal_list_entries(host, oracle, ctx, genome):
    """Windows of 65 535 bases cut from a genome of 700 001 overlap, so a mate that is frequent in one is found again (score2)."""
    rng = np.random.default_rng(10)
    lens = [8, 150, 33, 250, 5, 120, 70, 200, 16]
    xtras = b_xtras(lens)
    specs = mate_specs(rng, genome[0], lens, lambda i: 65535 - (i % 2) * 5, xtras)
    assert sum(specs[k % 9]["re"] - specs[k % 9]["rb"] for k in range(B_N) if xtras[k % 9] & XSUBO) > 1 << 28
    check_matesw(host, oracle, ctx, genome, specs, B_N)
