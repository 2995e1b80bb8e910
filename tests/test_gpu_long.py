"""The long-query kernel (bsw_long_kernel.hip: query sides of 1 024 - 8 191 bases) against the CPU oracle, bit-exact on every
field: a parameter fuzz at long lengths, one constructed case per mechanism of the kernel (the live band in chunks of 64
columns, F across chunks, the target refill, the closed-form first row, int32 scores up to BSW_MAX_SCORE, ties, the LDS row
shared by four wavefronts, band retries), every entry point that can hand it a long seed, task 0 as a long seed in front of
lane seeds, and several devices.  Each constructed case also checks, on the oracle's output, that the construct happened."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _gen
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

# both sides of the register / LDS boundary and of the two LDS classes (2 048 and 8 192 columns)
EDGE = (1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049, 8190, 8191)
MAX_SCORE = 1 << 20
E_LIMIT = -3


def _seq(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _read(rng, t, n, sub=0.01, indel=0.0):
    return _gen.mutate(rng, t, n, sub, indel)


def _asym_matrix(rng):
    """A random int8 5x5 matrix, [target][query], that is not its own transpose, also in its N row / column."""
    while True:
        m = rng.integers(-6, 3, (5, 5)).astype(np.int8)
        for i in range(4):
            m[i, i] = rng.integers(1, 6)
        if (m != m.T).any() and (m[4, :4] != m[:4, 4]).any():
            return m.reshape(25)


def _n_codes(rng, a, rate):
    """Ns at `rate`, written as any of the codes 4 - 7 (the library reads every code above 4 as N; the oracle, like bwa,
    indexes its matrix with the code: it gets the sequences with 4 in their place, _clean)."""
    a = a.copy()
    hit = rng.random(len(a)) < rate
    a[hit] = rng.integers(4, 8, int(hit.sum()))
    return a


def _clean(seeds):
    return [{k: (np.minimum(v, 4).astype(np.uint8) if k in ("lq", "lt", "rq", "rt") else v) for k, v in s.items()} for s in seeds]


def _tasks(host, seeds):
    """(tasks with codes 4 - 7 for the GPU, the same tasks with N = 4 for the oracle, what keeps their bases alive)"""
    t, a = host.make_tasks(seeds)
    tc, ac = host.make_tasks(_clean(seeds))
    return t, tc, (a, ac)


def _check(ctx, oracle, p, tasks):
    want = oracle.pair_batch(p, tasks, nthreads=8)
    assert_same(ctx.extend_pairs(p, tasks), want, tasks)
    return want


def _sides(want, tasks):
    """EXT records of the sides that ran, with their query lengths."""
    ql = np.concatenate([tasks["lqlen"], tasks["rqlen"]])
    ext = np.concatenate([want["left"], want["right"]])
    return ext[ql > 0], ql[ql > 0]


# ---- a. parameter fuzz at long lengths ----------------------------------------------------------------------------------

@pytest.mark.parametrize("qmax", [1025, 1100, 2047, 2048, 5000, 8191])
def test_fuzz_long_parameters_and_shapes(host, oracle, qmax):
    """Random scoring (bwa matrices and asymmetric general ones), gaps, band, z-drop, clipping, band tries, variant and seed
    shapes, Ns as codes 4 - 7, under KERNEL_AUTO and KERNEL_WAVE.  Query sides from qmax / 2 (from 1 000 below 2 048: the
    register kernels' last class beside the long kernel) to qmax."""
    rng = np.random.default_rng(31000 + qmax)
    nseed = max(6, 40000 // qmax)
    with host.BswContext(device=0, kernel=host.KERNEL_AUTO) as actx, host.BswContext(device=0, kernel=host.KERNEL_WAVE) as wctx:
        for it in range(4):
            def pen():
                return int(rng.choice([0, int(rng.integers(1, 13))])), int(rng.integers(1, 5))
            (od, ed), (oi, ei) = pen(), pen()
            over = dict(o_del=od, e_del=ed, o_ins=oi, e_ins=ei, w=int(rng.choice([1, 10, 100, 2000])),
                        zdrop=int(rng.choice([0, 1, 10, 100])), pen_clip5=int(rng.integers(0, 15)),
                        pen_clip3=int(rng.integers(0, 15)), max_band_try=int(rng.integers(1, 4)), variant=(it >> 1) & 1)
            p = host.default_params(**over)
            p["mat"][0] = _asym_matrix(rng) if it & 1 else host.bwa_matrix(a=int(rng.integers(1, 4)), b=int(rng.integers(1, 6)),
                                                                          n=-int(rng.integers(0, 3)))
            seeds = _gen.random_seeds(rng, nseed, qmin=qmax // 2 if qmax > 2000 else 1000, qmax=qmax, tfac=float(rng.choice([0.6, 1.0, 1.3])),
                                      sub=float(rng.choice([0.0, 0.01, 0.05])), indel=float(rng.choice([0.0, 0.002, 0.01])),
                                      junk=0.15, h0max=int(rng.choice([60, 3000])))
            for s in seeds:
                for k in ("lq", "lt", "rq", "rt"):
                    if k in s:
                        s[k] = _n_codes(rng, s[k], 0.005)
            tasks, clean, keep = _tasks(host, seeds)
            assert (np.maximum(tasks["lqlen"], tasks["rqlen"]) > 1023).any()
            want = oracle.pair_batch(p, clean, nthreads=8)
            assert_same(actx.extend_pairs(p, tasks), want, tasks)
            assert_same(wctx.extend_pairs(p, tasks), want, tasks)


# ---- b. one mechanism at a time, at EDGE lengths --------------------------------------------------------------------------

def _full_band_cells(qlen, tlen, w):
    """cells of one side whose band never loses a column (every H > 0, zdrop 0, no retry)"""
    c = 0
    for i in range(tlen):
        beg, end = max(0, i - w), min(i + w + 1, qlen)
        if end <= beg:
            break
        c += end - beg
    return c


@pytest.mark.parametrize("w", [31, 32, 62, 63, 64, 127, 128])
def test_live_band_across_chunk_edges(host, oracle, ctx, w):
    """Near-identical reads, h0 large, zdrop 0: the band stays full, so [beg, end] holds 2w + 1 columns at offsets beg that
    are not multiples of 64 (and w + 1 .. 2w columns while it opens at the start)."""
    rng = np.random.default_rng(500 + w)
    seeds = []
    for k, L in enumerate(EDGE):
        t = _seq(rng, L + w + 40)
        s = dict(rq=_read(rng, t, L, 0.02), rt=t, h0=3000)
        if k % 2:
            lt = _seq(rng, L + 7)
            s["lq"], s["lt"] = _read(rng, lt, L - 300, 0.02), lt
        seeds.append(s)
    tasks, arena = host.make_tasks(seeds)
    for variant in (0, 1):
        p = host.default_params(variant=variant, w=w, zdrop=0)
        want = _check(ctx, oracle, p, tasks)
        for k, s in enumerate(seeds):                   # the construct: no column of the band is ever lost
            assert want["right"]["cells"][k] == _full_band_cells(len(s["rq"]), len(s["rt"]), w), (k, variant)
            if "lq" in s:
                assert want["left"]["cells"][k] == _full_band_cells(len(s["lq"]), len(s["lt"]), w), (k, variant)


def _gapped(rng, L, gap, kind, at):
    """(query, target): the query of L bases copies the target except for `gap` bases inserted into it (kind 'ins') or
    missing from it ('del') at `at`."""
    if kind == "ins":
        t = _seq(rng, L - gap + 30)
        q = np.concatenate([t[:at], _seq(rng, gap), t[at:L - gap]])
    else:
        t = _seq(rng, L + gap + 30)
        q = np.concatenate([t[:at], t[at + gap:L + gap]])
    return q.astype(np.uint8), t


@pytest.mark.parametrize("gap", [65, 130, 300])
def test_long_gaps_across_chunks(host, oracle, ctx, gap):
    """Query insertions (F carried across 64-column chunks) and deletions (E carried across rows) of 65 - 300 bases, o small
    and e = 1, on both sides of the seed."""
    rng = np.random.default_rng(700 + gap)
    seeds, kinds = [], []
    for L in EDGE:
        for kind in ("ins", "del"):
            rq, rt = _gapped(rng, L, gap, kind, L // 3 + 5)
            lq, lt = _gapped(rng, L, gap, kind, L // 4 - 11)
            seeds.append(dict(lq=lq, lt=lt, rq=rq, rt=rt, h0=400))         # (h0 > the gap's cost: the band lives through it)
            kinds.append(kind)
    tasks, arena = host.make_tasks(seeds)
    ins = np.array(kinds) == "ins"
    for variant in (0, 1):
        p = host.default_params(variant=variant, o_del=3, e_del=1, o_ins=1, e_ins=1, w=gap + 20, zdrop=0, max_band_try=1)
        want = _check(ctx, oracle, p, tasks)
        for side in ("left", "right"):                  # the construct: every alignment crosses its gap to the query's end
            e = want[side]
            assert (e["qle"][ins] - e["tle"][ins] == gap).all() and (e["tle"][~ins] - e["qle"][~ins] == gap).all(), (side, variant)


def test_target_refill(host, oracle, ctx):
    """Targets crossing 1 024, 2 048 and 4 096 rows (one coalesced refill per 1 024 rows), the longest target there is
    (BSW_MAX_TLEN = 65 535, small band: cheap), and targets of 0 and 1 bases under long queries."""
    rng = np.random.default_rng(1024)
    TL = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
    seeds = []
    for k, L in enumerate(EDGE):
        for T in TL:
            t = _seq(rng, T)
            n = min(L, T)
            q = np.concatenate([_read(rng, t, n, 0.01), _seq(rng, L - n)]).astype(np.uint8)
            s = dict(rq=q, rt=t, h0=int(rng.integers(30, 200)))
            if (k + T) % 3 == 0:
                s["lq"], s["lt"] = q[::-1].copy(), t[::-1].copy()
            seeds.append(s)
    t = _seq(rng, 65535)
    seeds.append(dict(rq=_read(rng, t, 8191, 0.01), rt=t, h0=100))
    seeds.append(dict(lq=_read(rng, t, 8000, 0.01), lt=t, rq=_read(rng, t[::-1], 1025, 0.0), rt=t[::-1].copy(), h0=90))
    for L in (1025, 2049, 8191):
        seeds.append(dict(rq=_seq(rng, L), rt=np.zeros(0, np.uint8), h0=40))
        seeds.append(dict(lq=_seq(rng, L), lt=_seq(rng, 1), rq=_seq(rng, L), rt=_seq(rng, 1), h0=40))
    tasks, arena = host.make_tasks(seeds)
    for variant, w in ((0, 40), (1, 5)):
        p = host.default_params(variant=variant, w=w, zdrop=0)
        want = _check(ctx, oracle, p, tasks)
        tle = want["right"]["tle"]
        for T in TL:                                    # the construct: alignments end on the target's last row
            assert (tle == T).any(), (T, variant)
        assert (tle > 8000).any()


@pytest.mark.parametrize("variant", [0, 1])
def test_first_row(host, oracle, ctx, variant):
    """The closed-form first row: alive over all 8 191 columns (h0 > o_ins + 8 191 e_ins, a band that covers them), and
    dying exactly at column 63, 64, 65 or 128 (h0 = o_ins + e_ins + (c - 1) e_ins: H(-1, c - 1) = e_ins, H(-1, c) = 0)."""
    rng = np.random.default_rng(63 + variant)
    p = host.default_params(variant=variant, w=8200, zdrop=0)
    oe, e = int(p["o_ins"][0]) + int(p["e_ins"][0]), int(p["e_ins"][0])
    seeds = []
    for L in (8190, 8191, 2049, 1024):
        t = _seq(rng, 150)
        seeds.append(dict(rq=np.concatenate([_read(rng, t, 100, 0.05), _seq(rng, L - 100)]).astype(np.uint8), rt=t, h0=9000))
    tasks, arena = host.make_tasks(seeds)
    want = _check(ctx, oracle, p, tasks)
    assert 9000 - oe - 8190 * e > 0
    assert (want["right"]["cells"] == tasks["rqlen"] * tasks["rtlen"]).all()      # the construct: every row is the whole query
    seeds, dies = [], []
    for c in (63, 64, 65, 128):
        for dh in (-1, 0, 1):
            h0 = oe + (c - 1) * e + dh
            first = [max(h0 - oe - (j - 1) * e, 0) for j in range(1, 300)]          # H(-1, j - 1) of columns j = 1 ..
            dies.append(next(j for j, x in zip(range(1, 300), first) if x == 0))
            for L in EDGE:
                t = _seq(rng, 400)
                q = _read(rng, t, L, 0.03) if L % 2 else np.concatenate([_seq(rng, 3), _read(rng, t, L - 3, 0.03)]).astype(np.uint8)
                seeds.append(dict(rq=q, rt=t, h0=h0))
    assert {63, 64, 65, 128} <= set(dies)
    tasks, arena = host.make_tasks(seeds)
    for w in (200, 64):
        _check(ctx, oracle, host.default_params(variant=variant, w=w, zdrop=0), tasks)


@pytest.mark.parametrize("variant", [0, 1])
def test_wide_scores_and_limits(host, oracle, ctx, variant):
    """int32 scores: matrix entries at the int8 extremes, h0 + (lqlen + rqlen) max(mat) = 2^20 - 1 accepted and bit-exact
    (2^20: BSW_E_LIMIT), o + e = 4 096 accepted at 8 191 columns (4 097: BSW_E_LIMIT), the 1 023-column register class
    above 65 535."""
    rng = np.random.default_rng(127 + variant)
    m = host.bwa_matrix(a=127, b=128, n=-1)
    assert m.min() == -128 and m.max() == 127
    seeds = []
    for L in EDGE:
        t = _seq(rng, L + 40)
        q = t[:L].copy() if L % 2 else _read(rng, t, L, 0.01, 0.002)
        seeds.append(dict(rq=q, rt=t, h0=MAX_SCORE - 1 - L * 127))
        if L <= 4096:
            lt = _seq(rng, L + 3)
            seeds.append(dict(lq=lt[:L].copy(), lt=lt, rq=q, rt=t, h0=MAX_SCORE - 1 - 2 * L * 127))
    tasks, arena = host.make_tasks(seeds)
    for over in (dict(), dict(o_del=96, e_del=4000, o_ins=4000, e_ins=96), dict(o_del=0, e_del=4096, o_ins=4095, e_ins=1, zdrop=100)):
        p = host.default_params(variant=variant, w=50, **over)
        p["mat"][0] = m
        want = _check(ctx, oracle, p, tasks)
        assert (want["score"] == MAX_SCORE - 1).any()                                  # the construct: the limit is reached
        big = want["score"][(tasks["rqlen"] == 1023) & (tasks["lqlen"] == 0)]
        assert (big > 65535).all()                                                    # ... and the register class is wide
    p = host.default_params(variant=variant, w=50)
    p["mat"][0] = m
    over, _a = host.make_tasks([dict(rq=seeds[0]["rq"], rt=seeds[0]["rt"], h0=seeds[0]["h0"] + 1)])
    with pytest.raises(host.BswError) as ei:
        ctx.extend_pairs(p, over)
    assert ei.value.code == E_LIMIT
    for bad in (dict(o_del=4096, e_del=1), dict(o_ins=1, e_ins=4096)):
        with pytest.raises(host.BswError) as ei:
            ctx.extend_pairs(host.default_params(variant=variant, **bad), tasks[:1])
        assert ei.value.code == E_LIMIT


def _tandem(rng, period, shift, L, tlen):
    """(query of L bases, target of tlen) of one repeat unit: the target is the query's repeat shifted by `shift` bases."""
    unit = _seq(rng, period)
    while any((unit == np.roll(unit, d)).all() for d in range(1, period)):       # a unit of its own period: no diagonal between
        unit = _seq(rng, period)
    rep = np.tile(unit, (max(L, tlen) + shift) // period + 2)
    return rep[:L].copy(), rep[shift:shift + tlen].copy()


@pytest.mark.parametrize("period", [1, 2, 3, 4, 16, 64])
def test_ties(host, oracle, ctx, period):
    """Homopolymers and tandem repeats.  With the target shifted by s bases the diagonals +s and -(p - s) both match, and gap
    penalties with o_del = o_ins + s - 2 (p - s) (e = 1, a = 1) make their cells EQUAL in every row: row-maximum ties between
    lanes and, at w = 64 (columns i - 1 and i + 1 of p = 2 in two chunks), between chunks.  A target shorter than the query
    keeps both diagonals alive to its last row, where the maximum is taken: ties go to the later column.  Ns scoring 0 after
    the repeat hold the last column's value down the rows: gscore ties go to the later row."""
    rng = np.random.default_rng(90 + period)
    s = period // 2 if period > 1 else 0
    o_ins = 40
    o_del = o_ins + s - 2 * (period - s) if period > 1 else 6
    seeds = []
    for k, L in enumerate(EDGE):
        q, t = _tandem(rng, period, s, L, L - s - 5 - k)
        seeds.append(dict(rq=q, rt=t, h0=100 + 7 * k))
        q2, t2 = _tandem(rng, period, (s + 1) % period, L, L + 200)
        seeds.append(dict(lq=q2, lt=t2, rq=q2[:L // 2 + 1].copy(), rt=np.concatenate([q2[:L // 2 + 1], t2[:50]]), h0=60))
    tasks, arena = host.make_tasks(seeds)
    for variant in (0, 1):
        for w in (64, 100):
            p = host.default_params(variant=variant, w=w, zdrop=0, o_del=o_del, e_del=1, o_ins=o_ins, e_ins=1)
            want = _check(ctx, oracle, p, tasks)
            if period > 1:                              # the construct: the maximum ends on the tie's later column (+s)
                r = want["right"][::2]
                assert (r["qle"] - r["tle"] == s).all(), (variant, w, r["qle"] - r["tle"])
    p = host.default_params(zdrop=100)
    p["mat"][0] = host.bwa_matrix(n=0)                  # N scores 0: a run of Ns holds a column's value down the rows
    seeds = []
    for L in EDGE:
        q = _tandem(rng, period, 0, L, L)[0]
        seeds.append(dict(rq=np.concatenate([q[:-1], [4]]).astype(np.uint8), rt=np.concatenate([q, np.full(70, 4, np.uint8)]), h0=30))
    tasks, arena = host.make_tasks(seeds)
    want = _check(ctx, oracle, p, tasks)
    assert (want["right"]["gtle"] > want["right"]["tle"]).all()                  # the construct: the later row of the tie


@pytest.mark.parametrize("n", [1, 2, 3, 5, 23])
def test_lds_rows_shared_by_four_wavefronts(host, oracle, ctx, n):
    """The 2 048-column class: four wavefronts per workgroup, each on its own LDS row; seeds of 1 025 - 2 047 bases mixed,
    a ragged last workgroup, and sides that reuse a row with a smaller query (left long / right short and the reverse)."""
    rng = np.random.default_rng(2048 + n)
    seeds = []
    for k in range(n):
        L = int(rng.integers(1025, 2048))
        t = _seq(rng, L + 60)
        s = dict(rq=_read(rng, t, L, 0.02, 0.003), rt=t, h0=int(rng.integers(20, 300)))
        if k % 3 != 2:
            L2 = int(rng.integers(1025, 2048)) if k % 3 == 0 else int(rng.integers(1, 1024))
            lt = _seq(rng, L2 + 30)
            s["lq"], s["lt"] = _read(rng, lt, L2, 0.02, 0.003), lt
            if k % 2:
                s["lq"], s["rq"], s["lt"], s["rt"] = s["rq"], s["lq"], s["rt"], s["lt"]
        seeds.append(s)
    seeds.append(dict(lq=_seq(rng, 8000), lt=_seq(rng, 8100), rq=_seq(rng, 1100), rt=_seq(rng, 1200), h0=9000))   # 8 192 class
    tasks, arena = host.make_tasks(seeds)
    for variant in (0, 1):
        _check(ctx, oracle, host.default_params(variant=variant, w=300, zdrop=0 if variant else 100), tasks)
    assert ((tasks["lqlen"] > 1024) & (tasks["rqlen"] < tasks["lqlen"]) & (tasks["rqlen"] > 0)).any()
    if n > 2:
        assert ((tasks["rqlen"] > 1024) & (tasks["lqlen"] < tasks["rqlen"]) & (tasks["lqlen"] > 0)).any()


@pytest.mark.parametrize("variant", [0, 1])
def test_band_retry_in_the_kernel(host, oracle, ctx, variant):
    """Indels beyond w with max_band_try 2 and 3: one gap of 0.8 w (crossed at w, max_off >= 0.75 w: a retry at 2w) and a
    second one that takes the offset to 1.8 w (crossed at 2w only: a retry at 4w)."""
    rng = np.random.default_rng(40 + variant)
    w = 40
    seeds = []
    for L in EDGE:
        for kind in ("ins", "del"):
            for two in (False, True):
                g1, g2 = 32, 40
                q, t = _gapped(rng, L, g1, kind, L // 4 + 3)
                if two:
                    a2 = L // 2 + 9
                    if kind == "ins":
                        q = np.concatenate([q[:a2], _seq(rng, g2), q[a2:len(q) - g2]]).astype(np.uint8)
                    else:
                        tt = _seq(rng, len(t) + g2)
                        tt[:a2 + g1] = t[:a2 + g1]
                        tt[a2 + g1 + g2:] = t[a2 + g1:]
                        t = tt
                seeds.append(dict(rq=q, rt=t, h0=40) if len(seeds) % 2 else dict(lq=q, lt=t, h0=40))
    tasks, arena = host.make_tasks(seeds)
    for tries in (2, 3):
        p = host.default_params(variant=variant, w=w, zdrop=0, max_band_try=tries)
        want = _check(ctx, oracle, p, tasks)
        ext, ql = _sides(want, tasks)
        assert (ext["aw"] == 2 * w).sum() >= 5, tries                                  # the construct: retries happen
        if tries == 3:
            assert (ext["aw"] == 4 * w).sum() >= 5


# ---- c. every entry point that can hand the kernel a long seed ------------------------------------------------------------

def _mixed(host, oracle, rng):
    """Long and short seeds, Ns as codes 4 - 7, with non-default parameters: z-drop 100, asymmetric gaps, an asymmetric
    general matrix."""
    seeds = []
    for k, L in enumerate([1100, 30, 8191, 131, 2047, 4000, 60, 1025, 2048, 250, 5000, 1023, 3000, 90, 2049, 7000]):
        t = _n_codes(rng, _seq(rng, int(L * 1.2) + 30), 0.003)
        s = dict(rq=_n_codes(rng, _read(rng, t, L, 0.03, 0.004), 0.003), rt=t, h0=int(rng.integers(20, 400)))
        if k % 3:
            lt = _seq(rng, int(L * 0.9) + 20)
            s["lq"], s["lt"] = _n_codes(rng, _read(rng, lt, max(L * 2 // 3, 1), 0.03, 0.004), 0.003), lt
        seeds.append(s)
    p = host.default_params(zdrop=100, o_del=5, e_del=2, o_ins=3, e_ins=1, w=120)
    p["mat"][0] = _asym_matrix(rng)
    tasks, clean, keep = _tasks(host, seeds)
    return p, tasks, oracle.pair_batch(p, clean, nthreads=8), keep


def test_long_seeds_through_the_staged_path(host, oracle, ctx):
    """upload_raw + run_staged: the device packs and bins the seeds; the 2 048- and 8 192-column lists (segments 6 and 7)
    hold what bsw_plan_batch promises."""
    p, tasks, want, keep = _mixed(host, oracle, np.random.default_rng(61))
    b = ctx.upload_raw(p, tasks)
    try:
        ctx.run_staged(b)
        ctx.sync()
        assert_same(ctx.download(b), want, tasks)
        order, seg = ctx.batch_order(b)
    finally:
        b.free()
    want_order, want_seg, _ = host.plan_batch(p, tasks)
    assert (seg == want_seg).all()
    for s in (6, 7):
        lo, hi = int(seg[s]), int(seg[s + 1])
        assert hi > lo, s
        assert sorted(order[lo:hi]) == sorted(want_order[lo:hi]), s
    pt, pa = host.pack_tasks(tasks)
    assert_same(ctx.extend_pairs_packed(p, pt), want, tasks)


def test_long_seeds_streaming_and_tickets(host, oracle):
    """Streaming submits whose chunks cut the long seeds apart, several streams, and four tickets in flight."""
    p, tasks, want, keep = _mixed(host, oracle, np.random.default_rng(62))
    for streams, chunk in ((1, 3), (3, 5), (2, 7)):
        with host.BswContext(device=0, streams=streams, chunk_tasks=chunk, pack_threads=2) as c:
            assert_same(c.extend_pairs(p, tasks), want, tasks)
    with host.BswContext(device=0, streams=4) as c:
        outs, tickets = [], []
        for k in range(host.MAX_INFLIGHT):
            sub = tasks[k:]
            outs.append(c.submit(p, sub))
            tickets.append(c.last_ticket)
        for k in reversed(range(host.MAX_INFLIGHT)):
            c.wait_ticket(tickets[k])
            assert_same(outs[k], want[k:], tasks[k:])


def test_long_seeds_through_extend_batch(host, oracle, ctx):
    """bsw_extend_batch with per-task w, end_bonus and h0 on queries of 1 024 - 8 191 bases (and some short ones)."""
    rng = np.random.default_rng(63)
    n = 40
    et = np.zeros(n, dtype=host.EXT_TASK)
    keep = []
    for i in range(n):
        ql = int(rng.integers(1024, 8192)) if i % 4 else int(rng.integers(1, 300))
        t = _n_codes(rng, _seq(rng, int(ql * rng.choice([0.5, 1.1]))), 0.002)
        q = _n_codes(rng, _read(rng, t, ql, 0.03, 0.003), 0.002)
        keep.append((q, t))
        et[i]["query"], et[i]["target"], et[i]["qlen"], et[i]["tlen"] = q.ctypes.data, t.ctypes.data, ql, len(t)
        et[i]["w"], et[i]["end_bonus"], et[i]["h0"] = int(rng.choice([3, 50, 400, 3000])), int(rng.choice([0, 5, 100])), int(rng.integers(1, 2000))
    ec = et.copy()                                      # the oracle's copy: N = 4
    for i in range(n):
        qc, tc = np.minimum(keep[i][0], 4), np.minimum(keep[i][1], 4)
        keep.append((qc, tc))
        ec[i]["query"], ec[i]["target"] = qc.ctypes.data, tc.ctypes.data
    for variant in (0, 1):
        p = host.default_params(variant=variant, zdrop=int(rng.choice([0, 100])), o_del=4, e_del=2, o_ins=7, e_ins=1)
        p["mat"][0] = _asym_matrix(rng)
        got, want = ctx.extend_batch(p, et), oracle.ext_batch(p, ec, nthreads=8)
        for f in want.dtype.names:
            assert (got[f] == want[f]).all(), f


def test_drop_in_ksw_extend_on_long_queries(host, oracle):
    """The drop-in ksw_extend2 / ksw_extend at 1 024 - 8 191 bases with random parameters, both variants."""
    L = host.lib()
    rng = np.random.default_rng(64)
    try:
        for it in range(16):
            variant = it & 1
            L.bsw_set_default_variant(variant)
            ql = int(rng.choice([1024, 1025, 2047, 2048, 2049, int(rng.integers(1024, 8192)), 8191]))
            t = _n_codes(rng, _seq(rng, int(ql * rng.choice([0.3, 1.0, 1.2]))), 0.003)
            q = _n_codes(rng, _read(rng, t, ql, 0.03, 0.004), 0.003)
            m = _asym_matrix(rng) if it % 3 else host.bwa_matrix()
            od, ed, oi, ei = int(rng.integers(0, 10)), int(rng.integers(1, 4)), int(rng.integers(0, 10)), int(rng.integers(1, 4))
            w, eb, zd, h0 = int(rng.choice([10, 100, 1000])), int(rng.integers(0, 8)), int(rng.choice([0, 10, 100])), int(rng.integers(1, 3000))
            outs = [C.c_int(0) for _ in range(5)]
            if it % 4 < 2:
                sc = L.ksw_extend2(ql, q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, od, ed, oi, ei, w, eb, zd, h0,
                                   *[C.addressof(o) for o in outs])
                ref = oracle.extend2(np.minimum(q, 4), np.minimum(t, 4), m, od, ed, oi, ei, w, eb, zd, h0, variant=variant)
            else:
                sc = L.ksw_extend(ql, q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, od, ed, w, eb, zd, h0,
                                  *[C.addressof(o) for o in outs])
                ref = oracle.extend2(np.minimum(q, 4), np.minimum(t, 4), m, od, ed, od, ed, w, eb, zd, h0, variant=variant)
            got = dict(score=sc, qle=outs[0].value, tle=outs[1].value, gtle=outs[2].value, gscore=outs[3].value, max_off=outs[4].value)
            ref.pop("cells")
            assert got == ref, (it, ql, variant)
    finally:
        L.bsw_set_default_variant(0)


def _long_reads(host, rng, genome, n, rl):
    """Reads of rl bases from both strands of `genome` (never across the strand boundary), substitutions and Ns outside the
    seed, one seed of 19 - 60 bases each (at the read's start, its end or between)."""
    lp = len(genome)
    both = np.concatenate([genome, 3 - genome[::-1]])
    reads, seeds = [], np.zeros(n, dtype=host.SEED)
    for i in range(n):
        pos = int(rng.integers(1000, lp - rl - 1000)) + (i % 2) * lp
        read = both[pos:pos + rl].copy()
        sl = int(rng.integers(19, 60))
        qb = (0, rl - sl, int(rng.integers(0, rl - sl + 1)))[i % 3]
        for x in np.nonzero(rng.random(rl) < 0.02)[0]:
            if not (qb <= x < qb + sl):
                read[x] = 4 if rng.random() < 0.1 else (read[x] + 1 + rng.integers(0, 3)) % 4
        reads.append(read.astype(np.uint8))
        seeds[i] = (pos + qb, qb, sl)
    return reads, seeds


@pytest.mark.parametrize("rl", [1100, 2500, 8000])
def test_long_reads_against_the_resident_reference(host, oracle, rl):
    """extend_ref and submit_ref with long reads: left flanks read backwards from the seed, long targets fetched on the
    device, the same results as the oracle on the host-extracted tasks."""
    rng = np.random.default_rng(rl)
    lp = 200_000
    genome = rng.integers(0, 4, lp).astype(np.uint8)
    pac = host.pack_pac(genome)
    n = 24
    reads, seeds = _long_reads(host, rng, genome, n, rl)
    p = host.default_params(zdrop=100, o_del=6, e_del=1, o_ins=4, e_ins=2)
    tasks, keep = host.seeds_to_tasks(p, pac, lp, reads, seeds)
    assert (np.maximum(tasks["lqlen"], tasks["rqlen"]) > 1023).sum() >= 2 * n // 3       # (a seed inside the read: two shorter sides)
    want = oracle.pair_batch(p, tasks, nthreads=8)
    rt = np.zeros(n, dtype=host.REF_TASK)
    rmax = np.zeros(2, dtype=np.int64)
    for i in range(n):
        host.lib().bsw_chain_window(p.ctypes.data, seeds[i:i + 1].ctypes.data, 1, rl, lp, rmax.ctypes.data)
        rt[i]["query"], rt[i]["l_query"], rt[i]["init_score"] = reads[i].ctypes.data, rl, -1
        rt[i]["seed"] = seeds[i]
        rt[i]["rmax0"], rt[i]["rmax1"], rt[i]["tag"] = rmax[0], rmax[1], i
    with host.BswContext(device=0, chunk_tasks=7, streams=2) as c:
        ref = c.ref_upload(pac, lp)
        try:
            assert_same(c.extend_ref(p, ref, rt), want, tasks)
            got = c.submit_ref(p, ref, rt)
            c.wait()
            assert_same(got, want, tasks)
        finally:
            c.ref_free(ref)


# ---- d. task 0 as a long seed in front of lane seeds ----------------------------------------------------------------------

def task0_batch(host, read_len, n_lane):
    """Task 0: a 5 000 / 3 000-base two-sided seed.  Behind it n_lane (not a multiple of 128) lane seeds of read_len-base
    reads, with Ns: unused lane slots of the last wavefront and the N list's unused tails borrow task 0's record."""
    rng = np.random.default_rng(5000 + read_len)
    lt, rt = _seq(rng, 5200), _seq(rng, 3300)
    head, ha = host.make_tasks([dict(lq=_read(rng, lt, 5000, 0.02, 0.002), lt=lt, rq=_read(rng, rt, 3000, 0.02, 0.002), rt=rt,
                                     h0=40, tag=777)])
    lane, la = host.synth_tasks(n_lane, seed=read_len, read_len=read_len, seed_len_min=19, seed_len_max=60, seed_at_start=0,
                                sub_rate=0.02, indel_rate=0.004, junk_frac=0.05, n_rate=0.002)
    assert n_lane % 128 and (lane["lqlen"] <= 255).all() and (lane["rqlen"] <= 255).all()
    return np.concatenate([head, lane]), (ha, la)


TASK0_SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as g
host, orc = g.load_package().host, g.load_oracle()
from test_gpu_parity import assert_same
from test_gpu_long import task0_batch
for read_len, n in ((150, 40077), (250, 30077)):
    tasks, keep = task0_batch(host, read_len, n)
    for variant in (0, 1):
        p = host.default_params(variant=variant)
        want = orc.pair_batch(p, tasks, nthreads=8)
        for kernel in (host.KERNEL_AUTO, host.KERNEL_LANE):
            with host.BswContext(device=0, kernel=kernel) as c:
                assert_same(c.extend_pairs(p, tasks), want, tasks)
print("ok")
"""


@pytest.mark.parametrize("read_len, n", [(150, 40077), (250, 30077)])
def test_task0_is_a_long_seed(host, oracle, read_len, n):
    """150 bp lane seeds (lane kernels) and 250 bp ones (group and lane2l kernels), under KERNEL_AUTO and KERNEL_LANE."""
    tasks, keep = task0_batch(host, read_len, n)
    for variant in (0, 1):
        p = host.default_params(variant=variant)
        want = oracle.pair_batch(p, tasks, nthreads=8)
        for kernel in (host.KERNEL_AUTO, host.KERNEL_LANE):
            with host.BswContext(device=0, kernel=kernel) as c:
                assert_same(c.extend_pairs(p, tasks), want, tasks)


def test_task0_is_a_long_seed_with_the_n_list():
    """The same batches with BSW_NSPLIT=1 (the lane seeds with an N go to their own list; the lists' unused tails are slots
    that borrow task 0).  The switch is read once per process: own process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TASK0_SNIPPET % dict(root=root)], env=dict(os.environ, BSW_NSPLIT="1"),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- e. several devices -----------------------------------------------------------------------------------------------------

def test_long_seeds_on_two_slot_sets_of_one_device(host, oracle):
    p, tasks, want, keep = _mixed(host, oracle, np.random.default_rng(65))
    with host.BswContext(devices=[0, 0], streams=2, chunk_tasks=3) as c:
        assert_same(c.extend_pairs(p, tasks), want, tasks)


def test_long_seeds_on_every_device(host, oracle):
    """The long kernel's dynamic-LDS limit is set on each device it runs on (needs two GPUs)."""
    nd = int(host.lib().bsw_device_count())
    if nd < 2:
        pytest.skip("one GPU visible")
    p, tasks, want, keep = _mixed(host, oracle, np.random.default_rng(66))
    with host.BswContext(devices=list(range(min(nd, host.MAX_DEVICES))), streams=1, chunk_tasks=2) as c:
        assert_same(c.extend_pairs(p, tasks), want, tasks)
