"""GPU parity of bsw_matesw_ref_batch (mem_matesw's ksw_align2 against the resident reference) with the CPU restatement in
tests/_matesw_ref.py: every field of ksw_align2's result, the status and mem_matesw's region, bit for bit; and equality with
bsw_align_batch on host-fetched, host-reverse-complemented sequences."""
import numpy as np
import pytest

import _gen
import _gencigar_ref as gc
import _matesw_ref as mr

pytestmark = pytest.mark.gpu

L_PAC = 300_003                       # not a multiple of 4
XBYTE, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
FIELDS = ("status", "rb", "re", "qb", "qe", "score", "csub", "seedcov")


@pytest.fixture(scope="module")
def genome(ctx):
    rng = np.random.default_rng(77)
    pac = gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))
    ref = ctx.ref_upload(pac, L_PAC)
    yield pac, ref
    ctx.ref_free(ref)


def pen_of(p):
    return int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0])


def task(mate, is_rev, rb, re, xtra=None, min_score=19):
    mate = np.ascontiguousarray(mate, dtype=np.uint8)
    if xtra is None:
        xtra = mr.xtra_of(len(mate), 1, 19)
    return dict(mate=mate, is_rev=int(is_rev), rb=int(rb), re=int(re), xtra=int(xtra), min_score=int(min_score))


def mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.03, indel=0.005, nrate=0.0, junk=0.0):
    """a mate of l_ms bases whose aligned form (reverse-complemented when is_rev) comes from somewhere inside [rb, re)"""
    if rng.random() < junk or re - rb < 2:
        m = rng.integers(0, 4, l_ms).astype(np.uint8)
    else:
        w = gc.bns_get_seq(pac, L_PAC, rb, re)
        a = int(rng.integers(0, max(1, len(w) - l_ms // 2)))
        src = np.concatenate([w[a:], rng.integers(0, 4, l_ms).astype(np.uint8)])
        m = _gen.mutate(rng, src, l_ms, sub, indel)
        if is_rev:
            m = mr.revcomp(m)
    if nrate:
        m[rng.random(l_ms) < nrate] = 4
    return m


def window(rng, strand, length):
    lo = 0 if strand == 0 else L_PAC
    rb = lo + int(rng.integers(0, L_PAC - length + 1))
    return rb, rb + length


def make_mtasks(host, specs, arena=None):
    mt = np.zeros(len(specs), dtype=host.MTASK)
    keep, off = [], 0
    for i, s in enumerate(specs):
        m = s["mate"]
        if arena is not None and len(m):
            arena.u8[off:off + len(m)] = m
            ptr = arena.ptr + off
            off += len(m) + 1
        else:
            keep.append(m)
            ptr = m.ctypes.data if len(m) else 0
        mt[i]["mate"], mt[i]["l_ms"], mt[i]["is_rev"] = ptr, len(m), s["is_rev"]
        mt[i]["rb"], mt[i]["re"], mt[i]["xtra"], mt[i]["min_score"] = s["rb"], s["re"], s["xtra"], s["min_score"]
    return mt, keep


def expected(host, oracle, p, pac, specs):
    return mr.matesw_batch(oracle, host.ATASK, p["mat"][0], pen_of(p), L_PAC, pac, [s["mate"] for s in specs],
                           [s["is_rev"] for s in specs], [s["rb"] for s in specs], [s["re"] for s in specs],
                           [s["xtra"] for s in specs], [s["min_score"] for s in specs])


def check(host, oracle, ctx, p, genome, specs, arena=None):
    pac, ref = genome
    mt, keep = make_mtasks(host, specs, arena)
    res = ctx.matesw_ref_batch(p, ref, mt)
    want = expected(host, oracle, p, pac, specs)
    got_aln = np.stack([res["aln"][k] for k in mr.ALN], axis=1)
    bad = np.nonzero((got_aln != want["aln"]).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), specs[i]["is_rev"], specs[i]["rb"], specs[i]["re"], len(specs[i]["mate"]), hex(specs[i]["xtra"]),
                            got_aln[i].tolist(), want["aln"][i].tolist()) for i in bad[:5]]
    for f in FIELDS:
        bad = np.nonzero(res[f] != want[f])[0]
        assert len(bad) == 0, (f, [(int(i), int(res[f][i]), int(want[f][i])) for i in bad[:5]])
    assert (res["_pad"] == 0).all()
    return res, want


def test_both_halves_both_orientations(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(1)
    specs = []
    for i in range(1200):
        strand, is_rev = i & 1, (i >> 1) & 1
        rb, re = window(rng, strand, int(rng.integers(400, 700)))
        specs.append(task(mate_in(rng, pac, rb, re, 150, is_rev, junk=0.1), is_rev, rb, re))
    res, _ = check(host, oracle, ctx, host.default_params(), genome, specs)
    for strand in (0, 1):
        for is_rev in (0, 1):
            sel = np.array([(s["rb"] >= L_PAC) == strand and s["is_rev"] == is_rev for s in specs])
            assert (res["status"][sel] == 0).sum() > 200 and (res["status"][sel] == 2).any(), (strand, is_rev)
    kept = res["status"] == 0
    # a kept region lands on the other strand exactly when the mate was reverse-complemented
    on_rev = res["rb"] >= L_PAC
    win_rev = np.array([s["rb"] >= L_PAC for s in specs])
    isr = np.array([s["is_rev"] for s in specs], dtype=bool)
    assert (on_rev[kept] == (win_rev ^ isr)[kept]).all()


def test_clamped_bridging_and_empty_windows(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(2)
    specs = []
    for is_rev in (0, 1):
        for rb, re in ((0, 500), (0, 1), (2 * L_PAC - 500, 2 * L_PAC), (2 * L_PAC - 1, 2 * L_PAC), (L_PAC - 400, L_PAC),
                       (L_PAC, L_PAC + 400)):
            specs.append(task(mate_in(rng, pac, rb, re, 150, is_rev), is_rev, rb, re))
        # status 1: bridging l_pac, empty, reversed, outside [0, 2*l_pac), and an empty mate
        for rb, re in ((L_PAC - 200, L_PAC + 200), (L_PAC - 1, L_PAC + 1), (1000, 1000), (1000, 900), (-5, 300),
                       (2 * L_PAC - 300, 2 * L_PAC + 5), (2 * L_PAC, 2 * L_PAC + 100)):
            specs.append(task(rng.integers(0, 4, 150), is_rev, rb, re))
        specs.append(task(np.zeros(0, np.uint8), is_rev, 100, 600))
    res, _ = check(host, oracle, ctx, host.default_params(), genome, specs)
    assert (res["status"] == 1).sum() == 16
    assert (res["status"] == 0).sum() >= 8
    assert (res["aln"]["score"][res["status"] == 1] == 0).all() and (res["aln"]["te"][res["status"] == 1] == -1).all()


def class_lengths():
    """each align class's last query length and one more than the previous class's (byte and word classes alike)"""
    ends = [128, 160, 256, 512, 1024]
    out = [1, 2]
    for k, e in enumerate(ends):
        out.append(e)
        if k:
            out.append(ends[k - 1] + 1)
    return out


@pytest.mark.parametrize("mode", ["byte", "word"])
def test_every_align_class(host, oracle, ctx, genome, mode):
    pac, _ = genome
    rng = np.random.default_rng(3 if mode == "byte" else 4)
    specs = []
    for l_ms in class_lengths():
        for is_rev in (0, 1):
            for strand in (0, 1):
                rb, re = window(rng, strand, l_ms + int(rng.integers(50, 600)))
                x = XSUBO | XSTART | 19 | (XBYTE if mode == "byte" else 0)
                specs.append(task(mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.02), is_rev, rb, re, xtra=x, min_score=1))
    res, _ = check(host, oracle, ctx, host.default_params(), genome, specs)
    if mode == "byte":
        assert (res["aln"]["score"] == 255).sum() >= 8          # 8-bit saturation of the long queries
    assert (res["status"] == 0).sum() > len(specs) // 3


def test_flag_combinations_and_ns(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(5)
    specs = []
    flags = [0, XSTART, XSUBO, XSUBO | XSTART, XSTOP, XSTOP | XSTART, XSUBO | XSTOP | XSTART]
    for i in range(700):
        fl = flags[i % len(flags)] | (XBYTE if (i // len(flags)) & 1 else 0)
        thr = int(rng.choice([0, 10, 30, 60, 140, 0xffff]))
        is_rev, strand = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        l_ms = int(rng.choice([36, 101, 150, 250]))
        rb, re = window(rng, strand, int(rng.integers(l_ms, 900)))
        m = mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.04, indel=0.01, nrate=0.02 if i % 3 == 0 else 0.0, junk=0.1)
        specs.append(task(m, is_rev, rb, re, xtra=fl | thr, min_score=int(rng.integers(0, 60))))
    res, want = check(host, oracle, ctx, host.default_params(), genome, specs)
    assert (res["aln"]["te2"] >= 0).any() and (res["aln"]["qb"] >= 0).any() and (res["aln"]["qb"] == -1).any()
    assert (res["status"] == 2).any() and (res["status"] == 0).any()
    assert any((s["mate"] == 4).any() and s["is_rev"] and r == 0 for s, r in zip(specs, res["status"]))


def test_other_penalties_and_a_65535_base_window(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(6)
    specs = []
    for strand in (0, 1):
        for is_rev in (0, 1):
            rb, re = window(rng, strand, 65535)
            w = gc.bns_get_seq(pac, L_PAC, rb, re)
            m = _gen.mutate(rng, w[60000:], 250, 0.03, 0.01)
            specs.append(task(mr.revcomp(m) if is_rev else m, is_rev, rb, re))
    for _ in range(40):
        is_rev = int(rng.integers(0, 2))
        rb, re = window(rng, int(rng.integers(0, 2)), 800)
        specs.append(task(mate_in(rng, pac, rb, re, 250, is_rev, sub=0.05, indel=0.02), is_rev, rb, re))
    res, _ = check(host, oracle, ctx, host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1), genome, specs)
    assert (res["status"][:4] == 0).all() and (res["aln"]["tb"][:4] > 59000).all()


COMP = [3, 2, 1, 0, 4]


def general_specs(pac):
    """400 tasks under a matrix that is symmetric neither under transposition nor under complement (_gen.general_matrix): both
    strands x both is_rev, mates of 24 to 250 bases with xtra as mem_matesw builds it from the matrix's a (8-bit mode for the short
    ones), N in a third of the mates"""
    rng = np.random.default_rng(10)
    mat = _gen.general_matrix(rng, off_hi=-1)
    a = int(mat.diagonal()[:4].max())
    specs = []
    for i in range(400):
        strand, is_rev = i & 1, (i >> 1) & 1
        l_ms = (24, 60, 150, 250)[(i >> 2) & 3]
        rb, re = window(rng, strand, l_ms + int(rng.integers(100, 450)))
        m = mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.04, indel=0.01, nrate=0.02 if i % 3 == 0 else 0.0, junk=0.05)
        specs.append(task(m, is_rev, rb, re, xtra=mr.xtra_of(l_ms, a, 19), min_score=int(rng.choice([19, 19 * a]))))
    return mat, specs


def test_matrix_without_symmetry_on_both_strands_and_orientations(host, oracle, ctx, genome):
    """The reverse complement of is_rev belongs to the QUERY index of mat[target * 5 + query] and nowhere else.  Under bwa's
    matrices complementing the target index as well, or instead, or swapping the indices, changes nothing; here each reads another
    matrix.  The guard: with both codes complemented the CPU restatement itself answers differently on 199 of 200 is_rev tasks
    (measured; half is asserted)."""
    pac, _ = genome
    mat, specs = general_specs(pac)
    p = host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1)
    p["mat"][0] = mat.reshape(25)
    res, want = check(host, oracle, ctx, p, genome, specs)
    byte = np.array([(s["xtra"] & XBYTE) != 0 for s in specs])
    for strand in (0, 1):
        for is_rev in (0, 1):
            sel = np.array([(s["rb"] >= L_PAC) == strand and s["is_rev"] == is_rev for s in specs])
            assert sel.sum() == 100 and (res["status"][sel] == 0).sum() >= 60 and (res["status"][sel & byte] == 0).sum() >= 10, (strand, is_rev)
    p2 = host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1)
    p2["mat"][0] = mat[COMP][:, COMP].reshape(25)
    other = expected(host, oracle, p2, pac, specs)
    rev = np.array([s["is_rev"] == 1 for s in specs])
    differ = ((other["aln"] != want["aln"]).any(axis=1) & rev).sum()
    print("both codes complemented: %d of %d is_rev tasks differ" % (differ, rev.sum()))
    assert differ >= 0.49 * rev.sum()


def test_byte_mode_rejections(host, ctx, genome):
    """what bsw_align_batch rejects in 8-bit mode (include/bwa_sw_mi355.h at KSW_XBYTE), here too, per task"""
    _, ref = genome
    m = np.zeros(200, dtype=np.uint8)

    def rc_of(p, x1):
        mt = np.zeros(2, dtype=host.MTASK)
        for t, x in zip(mt, (XSUBO | XSTART | 19, x1)):
            t["mate"], t["l_ms"], t["rb"], t["re"], t["xtra"] = m.ctypes.data, 100, 0, 500, x
        try:
            ctx.matesw_ref_batch(p, ref, mt)
            return 0, ""
        except host.BswError as e:
            return e.code, str(e)

    pos = host.default_params(mat=np.arange(1, 26, dtype=np.int8))
    assert rc_of(pos, XSUBO | XSTART | 19)[0] == 0                           # 16-bit mode runs
    code, text = rc_of(pos, XBYTE | XSUBO | XSTART | 19)
    assert code == -2 and "mate task 1" in text and "KSW_XBYTE" in text and "smallest entry is 1" in text, text
    zero = host.default_params(mat=np.arange(0, 25, dtype=np.int8))
    assert rc_of(zero, XBYTE | XSUBO | XSTART | 19)[0] == 0                  # a smallest entry of 0 is accepted
    assert rc_of(host.default_params(o_del=254, e_del=1, o_ins=250, e_ins=5), XBYTE | XSTART)[0] == 0
    for over in (dict(o_del=255, e_del=1), dict(o_ins=250, e_ins=6)):
        assert rc_of(host.default_params(**over), XSTART)[0] == 0
        code, text = rc_of(host.default_params(**over), XBYTE | XSTART)
        assert code == -3 and "mate task 1" in text and "KSW_XBYTE" in text, text


@pytest.mark.parametrize("memory", ["pageable", "registered"])
def test_registered_and_pageable_mates(host, oracle, ctx, genome, memory):
    pac, _ = genome
    rng = np.random.default_rng(7)
    specs = []
    for _ in range(3000):
        is_rev = int(rng.random() < 0.9)
        rb, re = window(rng, int(rng.integers(0, 2)), int(rng.integers(500, 600)))
        specs.append(task(mate_in(rng, pac, rb, re, int(rng.integers(100, 151)), is_rev), is_rev, rb, re))
    arena = host.HostArena(sum(len(s["mate"]) + 1 for s in specs) + 64) if memory == "registered" else None
    try:
        check(host, oracle, ctx, host.default_params(), genome, specs, arena=arena)
    finally:
        if arena is not None:
            arena.free()


def test_empty_batch(host, ctx, genome):
    _, ref = genome
    assert len(ctx.matesw_ref_batch(host.default_params(), ref, np.zeros(0, dtype=host.MTASK))) == 0


def test_errors(host, ctx, genome):
    _, ref = genome
    p = host.default_params()
    m = np.zeros(1100, dtype=np.uint8)

    def rc_of(ref_, p_=p, **f):
        mt = np.zeros(2, dtype=host.MTASK)
        for t in mt:
            t["mate"], t["l_ms"], t["rb"], t["re"], t["xtra"] = m.ctypes.data, 100, 0, 500, XSUBO | XSTART | 19
        for k, v in f.items():
            mt[1][k] = v
        try:
            ctx.matesw_ref_batch(p_, ref_, mt)
            return 0
        except host.BswError as e:
            return e.code

    assert rc_of(ref) == 0
    assert rc_of(ref, l_ms=1025) == -3
    assert rc_of(ref, l_ms=1024) == 0
    assert rc_of(ref, rb=1000, re=1000 + 65536) == -3
    assert rc_of(ref, rb=1000, re=1000 + 65535) == 0
    assert rc_of(ref, l_ms=-1) == -2
    assert rc_of(ref, mate=0) == -2
    assert rc_of(ref, is_rev=2) == -2
    assert rc_of(ref, xtra=0x100000) == -2
    assert rc_of(None) == -2
    assert rc_of(ref, p_=host.default_params(mat=np.full(25, -1, np.int8))) == -2


def test_two_hundred_thousand_mixed_tasks(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(8)
    specs = []
    for i in range(200_000):
        is_rev = int(rng.random() < 0.9)
        l_ms = 150 if i % 5 else int(rng.choice([60, 101, 250]))
        k = int(rng.integers(0, 50))
        if k == 0:
            rb, re = L_PAC - 100, L_PAC + 100                   # bridging: status 1
        else:
            rb, re = window(rng, int(rng.integers(0, 2)), l_ms + int(rng.integers(100, 400)))
        specs.append(task(mate_in(rng, pac, rb, re, l_ms, is_rev, junk=0.05, nrate=0.001), is_rev, rb, re))
    res, _ = check(host, oracle, ctx, host.default_params(), genome, specs)
    assert (res["status"] == 1).any() and (res["status"] == 2).any() and (res["status"] == 0).sum() > 150_000


def test_equals_align_batch_on_host_fetched_sequences(host, ctx, genome):
    pac, ref = genome
    p = host.default_params()
    rng = np.random.default_rng(9)
    specs = []
    for l_ms in (36, 150, 250, 700):
        for _ in range(60):
            is_rev = int(rng.integers(0, 2))
            rb, re = window(rng, int(rng.integers(0, 2)), l_ms + int(rng.integers(50, 500)))
            specs.append(task(mate_in(rng, pac, rb, re, l_ms, is_rev, nrate=0.01), is_rev, rb, re))
    mt, keep = make_mtasks(host, specs)
    res = ctx.matesw_ref_batch(p, ref, mt)
    at = np.zeros(len(specs), dtype=host.ATASK)
    for i, s in enumerate(specs):                # the host recipe: bns_get_seq, reverse-complement the mate when is_rev
        rseq = gc.bns_get_seq(pac, L_PAC, s["rb"], s["re"])
        q = mr.revcomp(s["mate"]) if s["is_rev"] else s["mate"]
        keep += [q, rseq]
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = q.ctypes.data, rseq.ctypes.data, len(q), len(rseq), s["xtra"]
    ar = ctx.align_batch(p, at)
    for k in mr.ALN:
        assert (res["aln"][k] == ar[k]).all(), k
