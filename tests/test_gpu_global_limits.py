"""GPU parity for bwa's banded global alignment (ksw_global2) under general matrices, binding bands and at the value limits,
on BOTH kernels with the same inputs: bsw_global_kernel<1|2|4|8|16> (query lengths 40, 100, 200, 400, 900: one per register
class, qlen + 1 <= 64 C) and bsw_global_long_kernel (1 024 and 1 500; the short lengths once more in a child process under
BSW_GLOBAL_LONG=1).  Every comparison is exact: against the CPU oracle through test_gpu_global.check (score with and without
CIGAR, CIGAR operation by operation), against the independent banded DP full_dp.banded_global_dp wherever the band reaches
the last cell, and against closed forms.  DESIGN.md 4.5d lists the families and the wrong lines each caught."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _gen
from test_gpu_global import check, make_gtasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
import full_dp  # noqa: E402

pytestmark = pytest.mark.gpu

SHORT = [40, 100, 200, 400, 900]          # the register kernel's classes C = 1, 2, 4, 8, 16
LONG = [1024, 1500]                       # the LDS ring kernel
LIMIT_PENS = [(4000, 96, 4095, 1), (0, 4096, 4095, 1)]       # o + e = 4 096 on either side: check_params' limit


def params(host, mat=None, pen=None):
    p = host.default_params(**(dict(zip(("o_del", "e_del", "o_ins", "e_ins"), pen)) if pen else {}))
    if mat is not None:
        p["mat"][0] = np.asarray(mat, dtype=np.int8).ravel()
    return p


def check_dp(host, oracle, ctx, p, pairs, ws, max_cigar, dp=True):
    """check() against the oracle, then the score of every task whose band reaches the last cell against the banded DP.
    Returns the GPU's scores."""
    check(host, oracle, ctx, p, pairs, ws, max_cigar=max_cigar)
    gt, keep = make_gtasks(host, pairs, ws)
    res, _ = ctx.global_batch(p, gt, want_cigar=False)
    pen = (int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0]))
    if dp:
        for i, ((q, t), w) in enumerate(zip(pairs, ws)):
            if w >= abs(len(q) - len(t)):
                assert res["score"][i] == full_dp.banded_global_dp(q, t, p["mat"][0], *pen, w), (i, len(q), len(t), w)
    return [int(s) for s in res["score"]]


# ---- a. general matrices x binding bands ----------------------------------------------------------------------------------
def family_a(host, oracle, ctx, draw, qlen, dp=True):
    """40 pairs under a general matrix and penalties with insertion != deletion, N in queries and targets, each pair under
    w = |d| + 0..3 and under w = 500.  The band must change the score of at least 20 % of the pairs."""
    rng = np.random.default_rng(9100 + 10000 * draw + qlen)
    p = params(host, _gen.general_matrix(rng), _gen.GLOBAL_PENS[(draw + qlen) % 4])
    pairs, ws = [], []
    n = 40
    for k in range(n):
        q, t = _gen.global_pair(rng, qlen, indel=min(0.25, 8 / qlen))      # about 8 indels per read at every length
        pairs += [(q, t), (q, t)]
        ws += [abs(len(q) - len(t)) + k % 4, 500]
    sc = check_dp(host, oracle, ctx, p, pairs, ws, 2 * qlen + 32, dp)
    bound = sum(sc[2 * k] != sc[2 * k + 1] for k in range(n))
    print("family a draw %d qlen %d: the band binds on %d of %d" % (draw, qlen, bound, n))
    assert 5 * bound >= n, bound


def family_a_raw_codes(host, oracle, ctx, draw, lengths, dp=True):
    """40 pairs with raw codes 5..255 in queries and targets: they read as N, so the results are those of the same pairs
    with code 4 in their place (the oracle indexes the 5 x 5 matrix with the code and cannot be given them)."""
    rng = np.random.default_rng(9200 + draw)
    p = params(host, _gen.general_matrix(rng), _gen.GLOBAL_PENS[draw % 4])
    raw, clean, ws = [], [], []
    for k in range(40):
        q, t = _gen.global_pair(rng, lengths[k % len(lengths)])
        rq, rt = q.copy(), t.copy()
        for x, r in ((q, rq), (t, rt)):
            at = rng.random(len(x)) < 0.05
            r[at] = rng.integers(5, 256, int(at.sum()))
            x[at] = 4
        raw.append((rq, rt))
        clean.append((q, t))
        ws.append(abs(len(q) - len(t)) + k % 4 if k % 3 else 500)
    mc = 2 * max(lengths) + 32
    check_dp(host, oracle, ctx, p, clean, ws, mc, dp)
    res, cig = ctx.global_batch(p, make_gtasks(host, clean, ws)[0], max_cigar=mc)
    gt, keep = make_gtasks(host, raw, ws)
    res_raw, cig_raw = ctx.global_batch(p, gt, max_cigar=mc)
    assert res_raw.tobytes() == res.tobytes()
    for i in range(40):
        assert (cig_raw[i, :res["n_cigar"][i]] == cig[i, :res["n_cigar"][i]]).all(), i


# ---- b. matrix extremes on every class ------------------------------------------------------------------------------------
def family_b(host, oracle, ctx, qlen, dp=True):
    """entries from {-128, -127, -1, 0, 1, 126, 127}, N in queries and targets, under w = qlen and under a narrow band"""
    rng = np.random.default_rng(9300 + qlen)
    p = params(host, _gen.extremes_matrix(rng))
    pairs = [_gen.global_pair(rng, qlen, sub=0.04, indel=0.03) for _ in range(6)]
    check_dp(host, oracle, ctx, p, pairs + pairs, [qlen] * 6 + [20] * 6, 2 * qlen + 32, dp)


def family_b_known_answers(host, oracle, ctx, L):
    """a = 127, everything else -128: L bases against themselves score 127 L under any band; all-N under w = 0 (the diagonal
    alone) scores -128 L.  129 921 and -130 944 at 1 023 bases, 8 001 and -8 064 at 63."""
    rng = np.random.default_rng(9400 + L)
    s = rng.integers(0, 4, L).astype(np.uint8)
    n = np.full(L, 4, np.uint8)
    pairs, ws = [(s, s), (s, s), (s, s), (n, n)], [0, 20, L, 0]
    for pen in [None] + LIMIT_PENS:
        sc = check_dp(host, oracle, ctx, params(host, _gen.limit_matrix(), pen), pairs, ws, 8)
        assert sc == [127 * L, 127 * L, 127 * L, -128 * L], (L, pen, sc)


# ---- c. gap penalties at check_params' limit on every class ------------------------------------------------------------
def family_c(host, oracle, ctx, qlen, dp=True):
    """(4000, 96, 4095, 1) and (0, 4096, 4095, 1) with a = 127 so that a gap can pay, (0, 1, 0, 1) with bwa's matrix: clean
    gaps of 1, 2, 5 bases either way, in the middle, in front and at the end, under w = the gap (behind it the path runs on the
    band's edge; in front it takes the last cell of the first row or column that the band holds), score and CIGAR in closed
    form; then pairs whose alignments choose their gaps themselves"""
    rng = np.random.default_rng(9500 + qlen)
    for pen, mat, a in [(LIMIT_PENS[0], _gen.limit_matrix(), 127), (LIMIT_PENS[1], _gen.limit_matrix(), 127), ((0, 1, 0, 1), None, 1)]:
        p = params(host, mat, pen)
        pairs, ws, want = [], [], []
        for gap in (1, 2, 5):
            for deletion in (True, False):
                n = qlen if deletion else qlen - gap             # the query has qlen bases either way
                for at in (n // 2, 0, n):                        # 0: down the first column / along the first row to the band's edge
                    pairs.append(_gen.clean_gap_pair(rng, n, gap, deletion, at))
                    ws.append(gap)
                    o, e = pen[0:2] if deletion else pen[2:4]
                    want.append((a * n - (o + e * gap), _gen.clean_gap_cigar(n, gap, deletion, at)))
        sc = check_dp(host, oracle, ctx, p, pairs, ws, 8, dp)
        assert sc == [w[0] for w in want], (pen, sc)
        res, cig = ctx.global_batch(p, make_gtasks(host, pairs, ws)[0], max_cigar=8)
        for i, (_, cg) in enumerate(want):
            assert [(int(x) & 0xf, int(x) >> 4) for x in cig[i, :res["n_cigar"][i]]] == cg, (pen, i)
        pairs = [_gen.global_pair(rng, qlen, sub=0.03, indel=0.02, nrate=0.005, junk=0.0) for _ in range(4)]
        ws = [abs(len(q) - len(t)) + 1 for q, t in pairs]
        check_dp(host, oracle, ctx, p, pairs + pairs, ws + [500] * 4, 2 * qlen + 32, dp)


@pytest.mark.parametrize("qlen", SHORT + LONG)
@pytest.mark.parametrize("draw", [0, 1, 2])
def test_general_matrices_and_binding_bands(host, oracle, ctx, draw, qlen):
    family_a(host, oracle, ctx, draw, qlen)


@pytest.mark.parametrize("draw", [0, 1, 2])
def test_raw_codes_read_as_n(host, oracle, ctx, draw):
    family_a_raw_codes(host, oracle, ctx, draw, SHORT + LONG[:1])


@pytest.mark.parametrize("qlen", SHORT + LONG)
def test_matrix_extremes(host, oracle, ctx, qlen):
    family_b(host, oracle, ctx, qlen)


@pytest.mark.parametrize("L", [63, 100, 200, 400, 1023, 1024])
def test_matrix_extremes_known_answers(host, oracle, ctx, L):
    family_b_known_answers(host, oracle, ctx, L)


@pytest.mark.parametrize("qlen", SHORT + LONG)
def test_gap_penalties_at_the_limit(host, oracle, ctx, qlen):
    family_c(host, oracle, ctx, qlen)


def test_gap_penalties_beyond_the_limit_are_refused(host, oracle, ctx):
    """o + e = 4 097 on either side: BSW_E_LIMIT from bsw_global_batch; the drop-in reports its failure contract (a message on
    stderr, -1, *n_cigar = 0, no CIGAR) and serves the next call"""
    rng = np.random.default_rng(96)
    q, t = _gen.global_pair(rng, 100, junk=0.0)
    q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
    gt, keep = make_gtasks(host, [(q, t)], [50])
    L = host.lib()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    m = host.bwa_matrix()
    for pen in [(4001, 96, 6, 1), (6, 1, 4096, 1), (0, 4097, 6, 1), (6, 1, 1, 4096)]:
        with pytest.raises(host.BswError) as err:
            ctx.global_batch(params(host, None, pen), gt)
        assert err.value.code == -3 and host.ERRORS[-3] == "BSW_E_LIMIT", pen
        ncg, cg = C.c_int(7), C.POINTER(C.c_uint32)()
        assert L.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, *pen, 50, C.addressof(ncg), C.addressof(cg)) == -1
        assert ncg.value == 0 and not cg, pen
    for pen in LIMIT_PENS:                                       # 4 096 is served, by both entry points
        check(host, oracle, ctx, params(host, None, pen), [(q, t)], [50], max_cigar=256)
        ncg, cg = C.c_int(0), C.POINTER(C.c_uint32)()
        want = oracle.global2(q, t, m, *pen, 50)
        assert L.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, *pen, 50, C.addressof(ncg), C.addressof(cg)) == want["score"]
        assert [(int(cg[i]) & 0xf, int(cg[i]) >> 4) for i in range(ncg.value)] == want["cigar"]
        libc.free(cg)


# ---- d. a target of 65 535 rows on the register kernel -----------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "extremes"])
def test_target_of_65535_on_the_register_kernel(host, oracle, ctx, case):
    """qlen 60 (class 1) and 1 000 (class 16) against 65 535 target bases: under w = 65 535 every column is in the band on every
    row (h1_init = -(o_del + e_del (i + 1)) down to -2^28 with e_del = 4 096, E chains of 65 535 rows below MINUS_INF); under
    w = 100 the band leaves the query (end < beg for most rows: the score only, as check arranges)"""
    rng = np.random.default_rng(97)
    t = rng.integers(0, 4, 65535).astype(np.uint8)
    q1 = _gen.mutate(rng, t[:80], 60, 0.03, 0.02)
    q2 = _gen.mutate(rng, t[:1100], 1000, 0.03, 0.01)
    if case == "default":
        p = params(host)
    else:
        p = params(host, _gen.extremes_matrix(rng), LIMIT_PENS[1])
        q2[rng.integers(0, 1000, 20)] = 4
        t[rng.integers(0, 65535, 1300)] = 4
    check(host, oracle, ctx, p, [(q1, t), (q2, t), (q1, t), (q2, t)], [65535, 65535, 100, 100], max_cigar=2048)


# ---- e. the long kernel sees the short shapes ---------------------------------------------------------------------------
SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as g
host, orc = g.load_package().host, g.load_oracle()
import test_gpu_global_limits as lim
with host.BswContext(device=0) as ctx:
    # the scores of these inputs are compared with the banded DP in the parent, against the same oracle values: not again
    for qlen in lim.SHORT:
        for draw in (0, 1, 2):
            lim.family_a(host, orc, ctx, draw, qlen, dp=False)
        lim.family_b(host, orc, ctx, qlen, dp=False)
        lim.family_c(host, orc, ctx, qlen, dp=False)
    for draw in (0, 1, 2):
        lim.family_a_raw_codes(host, orc, ctx, draw, lim.SHORT, dp=False)
    for L in (63, 100, 200, 400, 1023):
        lim.family_b_known_answers(host, orc, ctx, L)
print("ok")
"""


def test_short_shapes_on_the_long_kernel():
    """families a to c at the five short lengths under BSW_GLOBAL_LONG=1.  The host exposes no launch or class statistic for the
    global path, so that the tests above ran the register classes rests on the route (global_route, bsw_f4_host.h) and on this
    process not carrying the switch, which is asserted."""
    assert os.environ.get("BSW_GLOBAL_LONG", "0") in ("", "0"), "the parent's short lengths must run on the register kernel"
    env = dict(os.environ, BSW_GLOBAL_LONG="1")
    out = subprocess.run([sys.executable, "-c", SNIPPET % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- f. the drop-in ABI ------------------------------------------------------------------------------------------------
def test_dropin_under_general_and_extreme_matrices(host, oracle):
    """ksw_global2 with m = 5: 12 calls of 150 and 1 100 bases (either kernel) under a general matrix and the extremes matrix"""
    rng = np.random.default_rng(98)
    L = host.lib()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for k in range(12):
        m = np.ascontiguousarray(_gen.general_matrix(rng).ravel() if k % 2 else _gen.extremes_matrix(rng))
        pen = _gen.GLOBAL_PENS[k % 4]
        q, t = _gen.global_pair(rng, 1100 if k % 3 == 0 else 150, junk=0.0)
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        w = abs(len(q) - len(t)) + (k % 4 if k < 8 else 500)
        ncg, cg = C.c_int(0), C.POINTER(C.c_uint32)()
        sc = L.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, *pen, w, C.addressof(ncg), C.addressof(cg))
        want = oracle.global2(q, t, m, *pen, w)
        assert sc == want["score"] == full_dp.banded_global_dp(q, t, m, *pen, w), (k, w)
        assert [(int(cg[i]) & 0xf, int(cg[i]) >> 4) for i in range(ncg.value)] == want["cigar"], k
        libc.free(cg)
