"""ksw_align2's two kernels (bsw_align_kernel: the row in registers; bsw_align_long_kernel under bsw_set_align_long(2): the row in
LDS) on the same inputs, where no test with a bwa matrix of a <= 3, b <= 6 goes: matrices that no symmetry protects and raw base
codes above 4 (a), the 8-bit shift 256 - min(mat) at both sides of its cap for shifts 0, 1, 100 and 128 (b), 16-bit scores at and
beyond 32 767 (c), the low 16 bits of xtra at their ends and at the task's own score (d), gap penalties up to the limit (e), and
what the hosts reject in 8-bit mode.  Every family runs on the register kernel with the switch off and on the LDS-row kernel under
mode 2, where each class the tasks belong to must have been launched exactly once; all seven fields against the oracle.
DESIGN.md 4.5c."""
import ctypes as C

import numpy as np
import pytest

import _gen
import test_gpu_align as ta
import test_gpu_align_long as tl

pytestmark = pytest.mark.gpu
XB, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
SCORE, TE, QE, SCORE2, TE2, TB, QB = range(7)
E_INVAL, E_LIMIT = -2, -3

# (seed, largest off-diagonal base entry, o_del, e_del, o_ins, e_ins): two matrices over the whole of [-9, 9] (mismatches that
# score, alignments that run on through anything and saturate the 8-bit mode) and three whose mismatches cost (8-bit runs that end
# below 255)
GENERAL = [(0, 9, 5, 2, 7, 1), (1, 9, 7, 1, 5, 2), (2, 0, 3, 1, 9, 3), (3, -1, 11, 2, 4, 1), (4, -4, 6, 1, 5, 1)]


def general_params(host, k):
    seed, off_hi, od, ed, oi, ei = GENERAL[k]
    p = host.default_params(o_del=od, e_del=ed, o_ins=oi, e_ins=ei)
    m = _gen.general_matrix(np.random.default_rng(900 + seed), off_hi)
    assert m.min() <= 0                                     # (8-bit mode needs an entry <= 0)
    p["mat"][0] = m.reshape(25)
    return p


def both_routes(host, oracle, ctx, p, pairs, xt, modes=(0, 2)):
    """the tasks on the register kernel (0: switch off) and / or on the LDS-row kernel (1, 2) against ONE oracle run; under 1 and 2
    every class the tasks belong to was launched once and no other -> (tasks, the oracle's int32[n][7])"""
    at, keep = ta.make(host, pairs, xt)
    want = tl.expect(oracle, p, at)
    for mode in modes:
        if mode == 0:
            host.set_align_long(0)
            tl.same(at, ctx.align_batch(p, at), want)
        else:
            got, grew = tl.run_mode(host, ctx, mode, p, at)
            tl.same(at, got, want)
            assert [c for c in range(len(grew)) if grew[c]] == tl.classes_of(at) and grew.max() == 1, (mode, grew)
    return at, want


def bwa_params(host, a, b, n=-1, **pen):
    p = host.default_params(**pen)
    p["mat"][0] = host.bwa_matrix(a, b, n)
    return p


# ---- a. matrices that no symmetry protects ------------------------------------------------------------------------------------
FLAGS = [0, XSTART, XSUBO | 19, XSUBO | XSTART | 19, XSUBO | XSTART | 30, XSTOP | 25]         # test_mate_rescue_shapes' set


@pytest.mark.parametrize("k", range(len(GENERAL)))
def test_a_asymmetric_matrices_and_raw_codes(host, oracle, ctx, k):
    """320 mate-rescue-like pairs (queries up to 300 bases, targets up to 700), both modes, N in queries and in targets (the N row
    and the N column differ), insertion and deletion penalties that differ; then 160 of the pairs with 4 % of the bytes of query
    and target replaced by raw codes 5..255, which the packer and the oracle both read as 4.  The profile is mat[target * 5 +
    query]: the indices swapped read the transposed matrix."""
    rng = np.random.default_rng(5000 + k)
    p = general_params(host, k)
    pairs = ta.rescue_like(rng, 320, 301, 700)
    for i, (q, t) in enumerate(pairs):
        if i % 3 == 0:
            t[rng.random(len(t)) < 0.02] = 4
        if i % 3 == 1:
            q[rng.random(len(q)) < 0.03] = 4
    xt = [int(rng.choice([XB, 0])) | int(rng.choice(FLAGS)) for _ in pairs]
    at, want = both_routes(host, oracle, ctx, p, pairs, xt)
    byte = (at["xtra"] & XB) != 0
    print("a[%d]: %d tasks, score>0 %d, tb>=0 %d, score2>=0 %d, 8-bit: saturated %d, between 1 and 254 %d" % (
        k, len(at), (want[:, SCORE] > 0).sum(), (want[:, TB] >= 0).sum(), (want[:, SCORE2] >= 0).sum(), (want[byte, SCORE] == 255).sum(),
        ((want[byte, SCORE] > 0) & (want[byte, SCORE] < 255)).sum()))
    assert len(at) >= 300 and (want[:, SCORE] > 0).sum() >= 250 and (want[:, TB] >= 0).sum() >= 80 and (want[:, SCORE2] >= 0).sum() >= 20
    assert (want[byte, SCORE] == 255).sum() >= 20 and ((want[byte, SCORE] > 0) & (want[byte, SCORE] < 255)).sum() >= 15
    raw = []
    for q, t in pairs[:160]:
        q, t = q.copy(), t.copy()
        for s in (q, t):
            hit = rng.random(len(s)) < 0.04
            s[hit] = rng.integers(5, 256, int(hit.sum()))
        raw.append((q, t))
    at, want = both_routes(host, oracle, ctx, p, raw, xt[:160])
    assert max(int(q.max()) for q, _ in raw) > 200 and max(int(t.max()) for _, t in raw) > 200 and (want[:, SCORE] > 0).sum() >= 120


# ---- b. the 8-bit shift at its cap --------------------------------------------------------------------------------------------
BYTE_CLASS_LEN = (100, 150, 250, 400, 1000)     # a query length in each 8-bit class of bsw_align_kernel (up to 128, 160, 256, 512, 1 024
#                                                  bases); under mode 2 they fall into the three 8-bit classes it reaches (256, 512, 1 024)


def split_score(v, lmax):
    """(a, m) with a * m == v: the most matching bases m <= lmax that a match score a <= 127 allows; None: no such pair"""
    for m in range(min(v, lmax), 0, -1):
        if v % m == 0 and v // m <= 127:
            return v // m, m
    return None


def shift_edge_pairs(rng, smin):
    """{match score a: pairs}.  The 8-bit run saturates when score + shift reaches 255, shift = -smin.  Per class length L and
    d in -1, 0, 1: a query of L bases that is N but for a piece of m bases, against that piece between two runs of N, with
    a * m == 255 - shift + d (a whole query of L > 255 - shift bases cannot score that little, so the piece is as long as a
    divisor allows); the same with a mismatch in the middle; and, with a * m == 255 - shift + d + 7, with the middle base deleted
    from the target or one inserted there: a one-base gap costs 7 under the default penalties, so E or F carry the alignment to
    the same three scores around the cap."""
    shift = -smin
    groups = {}
    for lc in BYTE_CLASS_LEN:
        for d in (-1, 0, 1):
            for gap in (0, 7):
                am = split_score(255 - shift + d + gap, lc - 1)
                if am is None or (gap and am[1] < 16):
                    continue
                a, m = am
                off = int(rng.integers(0, lc - m + 1))
                piece = rng.integers(0, 4, m).astype(np.uint8)
                q = np.full(lc, 4, np.uint8)
                q[off:off + m] = piece
                mid = m // 2
                if gap:
                    variants = [np.delete(piece, mid), np.insert(piece, mid, (piece[mid] + 2) & 3)]
                else:
                    variants = [piece]
                    if m >= 3:
                        mm = piece.copy()
                        mm[mid] = (mm[mid] + 1) & 3
                        variants.append(mm)
                for v in variants:
                    t = np.concatenate([np.full(7, 4, np.uint8), v, np.full(5, 4, np.uint8)]).astype(np.uint8)
                    groups.setdefault(a, []).append((q, t))
    return groups


@pytest.mark.parametrize("smin", [0, -1, -100, -128])
def test_b_byte_mode_shift_edges(host, oracle, ctx, smin):
    """shift = 0, 1, 100, 128 (the suite's bwa matrices give 1 to 6): scores one below, at and one above hcap = 255 - shift in every
    8-bit class of both kernels, with and without a live E / F.  min(mat) = 0 is the last matrix the hosts accept in 8-bit mode."""
    rng = np.random.default_rng(5100 - smin)
    scores, lens = [], set()
    for a, pairs in sorted(shift_edge_pairs(rng, smin).items()):
        p = host.default_params()
        m = np.full((5, 5), smin, np.int8)
        for k in range(4):
            m[k, k] = a
        p["mat"][0] = m.reshape(25)
        two = [pr for pr in pairs for _ in (0, 1)]
        at, want = both_routes(host, oracle, ctx, p, two, [XB | XSTART, XB | XSUBO | XSTART | 19] * len(pairs))
        scores.append(want[:, SCORE])
        lens |= set(int(x) for x in at["qlen"])
    sc = np.concatenate(scores)
    cap = 255 + smin
    print("b[%d]: %d tasks, score 255: %d, cap - 1 = %d: %d, below that %d" % (smin, len(sc), (sc == 255).sum(), cap - 1, (sc == cap - 1).sum(), (sc < cap - 1).sum()))
    assert lens == set(BYTE_CLASS_LEN) and len(sc) >= 100
    assert (sc == 255).sum() >= 40 and (sc == cap - 1).sum() >= 20 and (sc < cap - 1).sum() >= 10


# ---- c. 16-bit saturation -----------------------------------------------------------------------------------------------------
def saturating_tasks(rng, lengths):
    """per length: flank + query + flank, and the same + query[:200] (a second best; with 600 and 1 024 bases rows at the cap far
    enough from te to be one) x XSTART, XSUBO | XSTART | 1000, XSTOP | 32767"""
    pairs, xt = [], []
    for L in lengths:
        q = rng.integers(0, 4, L).astype(np.uint8)
        t1 = np.concatenate([rng.integers(0, 4, 20), q, rng.integers(0, 4, 20)]).astype(np.uint8)
        t2 = np.concatenate([rng.integers(0, 4, 20), q, rng.integers(0, 4, 20), q[:200]]).astype(np.uint8)
        for t in (t1, t2):
            for x in (XSTART, XSUBO | XSTART | 1000, XSTOP | 32767):
                pairs.append((q, t)); xt.append(x)
    return pairs, xt


def test_c_16_bit_saturation(host, oracle, ctx):
    """a = 127: 258 matches are 32 766, the 259th meets min(h + s, 32767).  Of bsw_align_kernel only <64, word> and <128, word> hold
    such a query (256 x 127 = 32 512).  What saturates: H and E (one dword of the LDS-row kernel: H | E << 16), the uint16 Hmax,
    qe_key's hmax << 16, b[]'s scores, and XSTOP | 32767 of the start pass."""
    rng = np.random.default_rng(5200)
    p = bwa_params(host, 127, 128)
    pairs, xt = saturating_tasks(rng, [257, 258, 259, 300, 511, 600, 1024])
    at, want = both_routes(host, oracle, ctx, p, pairs, xt)
    sat = want[:, SCORE] == 32767
    starts = sat & ((at["xtra"] & XSTART) != 0)
    print("c: %d tasks, 32766: %d, 32767: %d, score2 == 32767: %d, saturated with a start pass %d" % (
        len(at), (want[:, SCORE] == 32766).sum(), sat.sum(), (want[:, SCORE2] == 32767).sum(), starts.sum()))
    assert (want[:, SCORE] == 32766).sum() >= 4 and sat.sum() >= 20 and (want[:, SCORE] < 32766).sum() >= 4
    assert starts.sum() >= 10 and (want[starts, TB] >= 0).all() and (want[starts, QB] >= 0).all()
    assert (want[:, SCORE2] == 32767).sum() >= 1


def test_c_16_bit_saturation_beyond_1024_bases(host, oracle, ctx):
    """mode 1: 1 025 and 1 100 bases with a = 127, and the file's one pair of long tasks: 6 553 and 6 554 bases with a = 5 score
    32 765 and 32 770, the latter capped (targets of query + 2 x 50 bases)."""
    rng = np.random.default_rng(5201)
    pairs, xt = saturating_tasks(rng, [1025, 1100])
    at, want = both_routes(host, oracle, ctx, bwa_params(host, 127, 128), pairs, xt, modes=(1,))
    starts = (at["xtra"] & XSTART) != 0
    assert (want[:, SCORE] == 32767).all() and (want[starts, TB] >= 0).all() and (want[:, SCORE2] == 32767).sum() >= 1
    pairs = []
    for L in (6553, 6554):
        q = rng.integers(0, 4, L).astype(np.uint8)
        pairs.append((q, np.concatenate([rng.integers(0, 4, 50), q, rng.integers(0, 4, 50)]).astype(np.uint8)))
    at, want = both_routes(host, oracle, ctx, bwa_params(host, 5, 4), pairs, [XSTART, XSTART], modes=(1,))
    assert want[:, SCORE].tolist() == [32765, 32767] and want[:, TE].tolist() == [50 + 6552, 50 + 6553] and want[:, TB].tolist() == [50, 50]


# ---- d. the low 16 bits of xtra -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-1] + list(range(len(GENERAL))))
def test_d_xtra_thresholds_at_their_ends_and_at_the_score(host, oracle, ctx, k):
    """Per pair and mode, s = the task's own score from a first oracle run: XSUBO | 0 (every row enters b[], the fullest list the
    tlen-entry slice gets), XSUBO | 0xffff, XSUBO | s and s + 1 (the start pass runs / does not), XSTOP | s and s + 1 (stops at te /
    never), XSTOP | 0, and in 16-bit mode XSTOP | 256 and XSTOP | s - 1: each with and without XSTART.  Default matrix (k = -1)
    and the matrices of (a)."""
    rng = np.random.default_rng(5300 + k)
    p = host.default_params() if k < 0 else general_params(host, k)
    base_pairs = ta.rescue_like(rng, 12, 301, 700, junk=0.1)
    q = rng.integers(0, 4, 290).astype(np.uint8)                       # one pair whose 16-bit score is beyond 256 under every matrix
    base_pairs.append((q, np.concatenate([rng.integers(0, 4, 30), q[:140], q[141:], rng.integers(0, 4, 60), q[40:200]]).astype(np.uint8)))
    first, _ = ta.make(host, [pr for pr in base_pairs for _ in (0, 1)], [XB, 0] * len(base_pairs))
    s0 = tl.expect(oracle, p, first)[:, SCORE]
    pairs, xt = [], []
    for i, pr in enumerate(base_pairs):
        for b, base in enumerate((XB, 0)):
            s = int(s0[2 * i + b])
            xs = [XSUBO | 0, XSUBO | 0xffff, XSUBO | s, XSUBO | (s + 1), XSTOP | s, XSTOP | (s + 1), XSTOP | 0]
            if not base:
                xs += [XSTOP | 256, XSTOP | max(s - 1, 0)]
            for x in xs:
                for st in (0, XSTART):
                    pairs.append(pr); xt.append(base | st | x)
    at, want = both_routes(host, oracle, ctx, p, pairs, xt)
    x = at["xtra"]
    every_row = (x & XSUBO != 0) & (x & 0xffff == 0)
    print("d[%d]: %d tasks, scores beyond 256 %d, XSUBO | 0 with a second best %d, start passes %d" % (
        k, len(at), (want[:, SCORE] > 256).sum(), (want[every_row, SCORE2] >= 0).sum(), (want[:, TB] >= 0).sum()))
    assert 300 <= len(at) <= 500 and (want[:, SCORE] > 256).sum() >= 8 and (want[every_row, SCORE2] >= 0).sum() >= 20
    own = (x & XSUBO != 0) & (x & XSTART != 0) & ((x & 0xffff) == want[:, SCORE]) & (want[:, SCORE] > 0) & (want[:, SCORE] != 255)
    over = (x & XSUBO != 0) & (x & XSTART != 0) & ((x & 0xffff) == want[:, SCORE] + 1)
    assert own.sum() >= 10 and (want[own, TB] >= 0).sum() >= 10 and over.sum() >= 10 and (want[over, TB] == -1).all()


# ---- e. gap penalties -----------------------------------------------------------------------------------------------------------
GAPS = [  # a, b, o_del, e_del, o_ins, e_ins, modes
    (1, 4, 0, 1, 0, 1, (XB, 0)),
    (2, 3, 0, 1, 3, 2, (XB, 0)),
    (1, 4, 250, 5, 254, 1, (XB, 0)),              # o + e = 255: the most an 8-bit lane of bwa holds
    (127, 128, 255, 1, 200, 56, (0,)),            # 256
    (127, 128, 4000, 96, 4095, 1, (0,)),          # 4 096 = check_params' limit; a gap pays from 33 matches a side
    (127, 128, 7, 1, 4090, 6, (0,)),
]


@pytest.mark.parametrize("g", range(len(GAPS)))
def test_e_gap_penalties_up_to_the_limits(host, oracle, ctx, g):
    a, b, od, ed, oi, ei, bases = GAPS[g]
    rng = np.random.default_rng(5400 + g)
    p = bwa_params(host, a, b, o_del=od, e_del=ed, o_ins=oi, e_ins=ei)
    pairs = ta.rescue_like(rng, 150, 301, 700, junk=0.1)
    for L in (100, 200, 300):                      # one clean gap of 1, 2, 5 bases either way in the middle of a perfect match
        for glen in (1, 2, 5):
            q = rng.integers(0, 4, L).astype(np.uint8)
            fl = [rng.integers(0, 4, 15).astype(np.uint8) for _ in range(4)]
            pairs.append((q, np.concatenate([fl[0], q[:L // 2], q[L // 2 + glen:], fl[1]]).astype(np.uint8)))
            pairs.append((q, np.concatenate([fl[2], q[:L // 2], (q[L // 2:L // 2 + glen] + 1) & 3, q[L // 2:], fl[3]]).astype(np.uint8)))
    xt = [int(rng.choice(bases)) | int(rng.choice([XSTART, XSUBO | XSTART | 19, XSUBO | 19, 0])) for _ in pairs]
    at, want = both_routes(host, oracle, ctx, p, pairs, xt)
    assert (want[:, SCORE] > 0).sum() >= 120 and (want[:, TB] >= 0).sum() >= 50


def test_e_gap_penalties_beyond_the_limits_are_errors(host, oracle, ctx):
    rng = np.random.default_rng(5450)
    pairs = ta.rescue_like(rng, 20, 151, 400)
    for over in (dict(o_del=4096, e_del=1), dict(o_ins=4000, e_ins=97)):
        with pytest.raises(host.BswError) as ex:
            ctx.align_batch(host.default_params(**over), ta.make(host, pairs, [XSTART] * len(pairs))[0])
        assert ex.value.code == E_LIMIT
    # 8-bit mode: bwa's ksw_u8 keeps o + e in a byte lane, so 256 would act as 0 there; the task is rejected, the same in 16-bit mode runs
    for over in (dict(o_del=255, e_del=1), dict(o_ins=200, e_ins=56)):
        p = host.default_params(**over)
        for mode in (0, 2):
            host.set_align_long(mode)
            try:
                with pytest.raises(host.BswError) as ex:
                    ctx.align_batch(p, ta.make(host, pairs, [XSTART] * (len(pairs) - 1) + [XB | XSTART])[0])
            finally:
                host.set_align_long(0)
            assert ex.value.code == E_LIMIT and "KSW_XBYTE" in str(ex.value) and "task %d" % (len(pairs) - 1) in str(ex.value), str(ex.value)
        both_routes(host, oracle, ctx, p, pairs, [XSTART] * len(pairs))
    both_routes(host, oracle, ctx, host.default_params(o_del=254, e_del=1, o_ins=200, e_ins=55), pairs, [XB | XSTART] * len(pairs))


# ---- what the hosts reject in 8-bit mode ----------------------------------------------------------------------------------------
class KSWR(C.Structure):
    _fields_ = [(f, C.c_int) for f in ta.FIELDS]


def test_byte_mode_with_a_matrix_minimum_above_zero_is_rejected(host, oracle, ctx):
    """ksw_qinit's shift 256 - min(mat) wraps when min(mat) > 0: the SSE2 code then adds the wrapped profile byte (every H stays 0),
    the kernels keep the unwrapped score under hcap = 255 - shift and answered score 255.  The hosts reject such a task in 8-bit
    mode with BSW_E_INVAL and a text that says why; the same matrix in 16-bit mode runs and equals the oracle; a minimum of 0 is
    accepted."""
    rng = np.random.default_rng(5500)
    pairs = ta.rescue_like(rng, 40, 151, 400)
    n = len(pairs)
    L = host.lib()
    L.ksw_align2.restype = KSWR
    L.ksw_align2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.ksw_align.restype = KSWR
    L.ksw_align.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]
    for lo in (2, 1):
        p = host.default_params()
        p["mat"][0] = rng.integers(lo, 8, 25).astype(np.int8)
        p["mat"][0][7] = lo
        for mode in (0, 2):
            host.set_align_long(mode)
            try:
                with pytest.raises(host.BswError) as ex:
                    ctx.align_batch(p, ta.make(host, pairs, [XSTART] * (n - 1) + [XB | XSTART])[0])
            finally:
                host.set_align_long(0)
            assert ex.value.code == E_INVAL and "KSW_XBYTE" in str(ex.value) and "smallest entry is %d" % lo in str(ex.value), str(ex.value)
            assert "task %d" % (n - 1) in str(ex.value)
        at, want = both_routes(host, oracle, ctx, p, pairs, [int(rng.choice([XSTART, XSUBO | XSTART | 19])) for _ in pairs])
        assert (want[:, SCORE] > 100).sum() >= n // 2 and (want[:, TB] >= 0).sum() >= n // 2
        # the scalar ABI: the call's failure (score -1, the text on stderr), and the 16-bit call's answer
        m =np.ascontiguousarray(p["mat"][0])
        q, t = pairs[0]
        assert L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, XB | XSTART, None).score == -1
        assert L.ksw_align(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, XB | XSTART, None).score == -1
        r = L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, XSTART, None)
        w = oracle.align2(q, t, m, 6, 1, 6, 1, XSTART)
        assert [getattr(r, f) for f in ta.FIELDS] == [w[f] for f in ta.FIELDS]
    p["mat"][0][7] = 0                                       # smallest entry 0: shift 0, accepted in 8-bit mode
    at, want = both_routes(host, oracle, ctx, p, pairs, [XB | XSTART] * n)
    assert (want[:, SCORE] == 255).sum() >= n // 2
    m = np.ascontiguousarray(p["mat"][0])
    q, t = pairs[0]
    r = L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, XB | XSTART, None)
    w = oracle.align2(q, t, m, 6, 1, 6, 1, XB | XSTART)
    assert [getattr(r, f) for f in ta.FIELDS] == [w[f] for f in ta.FIELDS]
    assert L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 255, 1, 6, 1, XB | XSTART, None).score == -1
    r = L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 254, 1, 6, 1, XB | XSTART, None)
    w = oracle.align2(q, t, m, 254, 1, 6, 1, XB | XSTART)
    assert [getattr(r, f) for f in ta.FIELDS] == [w[f] for f in ta.FIELDS]
