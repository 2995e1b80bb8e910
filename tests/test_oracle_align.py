"""ksw_align2 oracle (oracle/ksw_align_ref.c, the literal emulation of bwa's striped local alignment): analytic known
answers, agreement with an independent numpy local DP, and re-scoring of the reported end points.  CPU only."""
import os
import sys

import numpy as np
import pytest

import _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
import full_dp  # noqa: E402


def bwa_mat(a=1, b=4, n=-1):
    m = np.full((5, 5), -b, dtype=np.int8)
    np.fill_diagonal(m, a)
    m[4, :] = n
    m[:, 4] = n
    return m


XB, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000


@pytest.mark.parametrize("byte", [True, False])
def test_known_answers(oracle, byte):
    rng = np.random.default_rng(3)
    mat = bwa_mat()
    xb = XB if byte else 0
    q = rng.integers(0, 4, 60).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 100), q, rng.integers(0, 4, 80)]).astype(np.uint8)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, xb | XSTART)
    assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (60, 159, 59, 100, 0)
    # three mismatches inside: 60 - 3*(1+4) = 45 for the whole read is beaten by the best clipped piece or not; re-derive with numpy
    q2 = q.copy()
    q2[[10, 30, 50]] = (q2[[10, 30, 50]] + 1) % 4
    r = oracle.align2(q2, t, mat, 6, 1, 6, 1, xb | XSTART)
    want = full_dp.local_dp(q2, t, mat, 6, 1, 6, 1)
    assert r["score"] == want["score"] == 45 and (r["te"], r["qe"]) in want["ends"]
    # one base deleted from the read: 59 matches and a 1-base gap along the query
    q3 = np.delete(q, 25)
    r = oracle.align2(q3, t, mat, 6, 1, 6, 1, xb | XSTART)
    assert r["score"] == 59 - 7 and (r["te"], r["qe"], r["tb"], r["qb"]) == (159, 58, 100, 0)
    # nothing aligns: score 0, te -1, qe 0 (first maximum of an all-zero column), start pass gives 0/0
    r = oracle.align2(np.zeros(20, np.uint8), np.full(50, 3, np.uint8), mat, 6, 1, 6, 1, xb | XSTART)
    assert (r["score"], r["te"], r["qe"], r["score2"], r["te2"]) == (0, -1, 0, -1, -1)
    # empty target
    r = oracle.align2(q, np.zeros(0, np.uint8), mat, 6, 1, 6, 1, xb)
    assert (r["score"], r["te"]) == (0, -1)


def test_byte_version_saturates_and_word_version_does_not(oracle):
    rng = np.random.default_rng(4)
    mat = bwa_mat()
    q = rng.integers(0, 4, 255).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30), q, rng.integers(0, 4, 30)]).astype(np.uint8)
    assert oracle.align2(q, t, mat, 6, 1, 6, 1, XB)["score"] == 255                 # gmax + shift reached 255: "try 16 bits"
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XSTART)
    assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (255, 284, 254, 30, 0)
    r = oracle.align2(q[:250], t, mat, 6, 1, 6, 1, XB | XSTART)                     # 250 + shift 4 = 254 < 255: still exact
    assert (r["score"], r["qe"], r["qb"]) == (250, 249, 0)


def test_second_best_and_stop(oracle):
    rng = np.random.default_rng(5)
    mat = bwa_mat()
    q = rng.integers(0, 4, 80).astype(np.uint8)
    q_bad = q.copy()
    q_bad[[5, 40, 70]] = (q_bad[[5, 40, 70]] + 2) % 4                               # a second, worse copy of the read
    t = np.concatenate([rng.integers(0, 4, 50), q_bad, rng.integers(0, 4, 120), q, rng.integers(0, 4, 40)]).astype(np.uint8)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XB | XSUBO | XSTART | 19)
    assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (80, 50 + 80 + 120 + 79, 79, 250, 0)
    want2 = full_dp.local_dp(q, t[:140], mat, 6, 1, 6, 1)                           # the worse copy alone
    assert r["score2"] == want2["score"] and 50 <= r["te2"] < 140
    # without KSW_XSUBO there is no list: score2 stays -1
    assert oracle.align2(q, t, mat, 6, 1, 6, 1, XB | XSTART)["score2"] == -1
    # KSW_XSUBO with a threshold above the score: no start pass (tb, qb stay -1)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XB | XSUBO | XSTART | 200)
    assert (r["score"], r["tb"], r["qb"]) == (80, -1, -1)
    # KSW_XSTOP ends the scan at the first row that reaches the threshold
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XB | XSTOP | 30)
    assert 30 <= r["score"] <= 31 and r["te"] < 140


@pytest.mark.parametrize("seed", range(6))
def test_random_pairs_against_the_numpy_local_dp(oracle, seed):
    rng = np.random.default_rng(100 + seed)
    a, b = [(1, 4), (1, 4), (2, 3), (1, 1), (3, 5), (1, 6)][seed]
    o, e = [(6, 1), (4, 2), (5, 1), (3, 1), (10, 2), (0, 1)][seed]
    mat = bwa_mat(a, b, -1)
    n_eq = n = 0
    for k in range(60):
        ql, tl = int(rng.integers(1, 200)), int(rng.integers(1, 400))
        t = rng.integers(0, 4, tl).astype(np.uint8)
        if k % 3:
            src = t[int(rng.integers(0, max(1, tl - ql))):][:ql]
            q = _gen.mutate(rng, src, len(src), 0.05, 0.03)
        else:
            q = rng.integers(0, 5, ql).astype(np.uint8)
        if len(q) == 0:
            continue
        want = full_dp.local_dp(q, t, mat, o, e, o, e)
        for xb in (XB, 0):
            if xb and want["score"] + b >= 255:
                continue
            r = oracle.align2(q, t, mat, o, e, o, e, xb | XSTART)
            n += 1
            assert r["score"] <= want["score"]                                      # never above the unrestricted optimum
            if r["score"] == want["score"]:
                n_eq += 1
                if r["score"] > 0:
                    assert (r["te"], r["qe"]) in want["ends"]
            if r["score"] > 0:
                # the reported box [qb, qe] x [tb, te] really holds an alignment of that score
                assert 0 <= r["tb"] <= r["te"] and 0 <= r["qb"] <= r["qe"]
                box = full_dp.local_dp(q[r["qb"]:r["qe"] + 1], t[r["tb"]:r["te"] + 1], mat, o, e, o, e)
                assert box["score"] >= r["score"]
    assert n_eq >= 0.97 * n                                                          # the I->D restriction almost never binds


def general_pairs(seed, n=50):
    """n pairs of 1..120 x 1..250 codes 0..4 under a matrix of _gen.general_matrix and gap penalties that differ between
    insertion and deletion: two thirds mutated pieces of the target, one third random"""
    rng = np.random.default_rng(700 + seed)
    mat = _gen.general_matrix(rng)
    pen = [(5, 2, 7, 1), (7, 1, 5, 2), (3, 1, 9, 3), (11, 2, 4, 1)][seed]         # o_del, e_del, o_ins, e_ins
    pairs = []
    while len(pairs) < n:
        ql, tl = int(rng.integers(1, 121)), int(rng.integers(1, 251))
        t = rng.integers(0, 5 if len(pairs) % 4 == 0 else 4, tl).astype(np.uint8)
        if len(pairs) % 3:
            src = t[int(rng.integers(0, max(1, tl - ql))):][:ql]
            q = _gen.mutate(rng, src, len(src), 0.05, 0.03)
            if len(q):
                q[rng.random(len(q)) < 0.03] = 4
        else:
            q = rng.integers(0, 5, ql).astype(np.uint8)
        if len(q):
            pairs.append((q, t))
    return mat, pen, pairs


@pytest.mark.parametrize("seed", range(4))
def test_general_matrices_against_the_numpy_local_dp(oracle, seed):
    """The relations of test_random_pairs_against_the_numpy_local_dp under matrices that are not symmetric (4 x 50 pairs, both
    modes; an 8-bit run only where it cannot saturate): an oracle that read mat[query][target], or used the insertion
    penalties for deletions, would not stay at or below the DP and equal to it on 97 % of the runs."""
    mat, (od, ed, oi, ei), pairs = general_pairs(seed)
    shift = max(0, -int(mat.min()))
    n_eq = n = 0
    for q, t in pairs:
        want = full_dp.local_dp(q, t, mat, od, ed, oi, ei)
        for xb in (XB, 0):
            if xb and want["score"] + shift >= 255:
                continue
            r = oracle.align2(q, t, mat, od, ed, oi, ei, xb | XSTART)
            n += 1
            assert r["score"] <= want["score"]
            if r["score"] == want["score"]:
                n_eq += 1
                if r["score"] > 0:
                    assert (r["te"], r["qe"]) in want["ends"]
            if r["score"] > 0:
                assert 0 <= r["tb"] <= r["te"] and 0 <= r["qb"] <= r["qe"]
                box = full_dp.local_dp(q[r["qb"]:r["qe"] + 1], t[r["tb"]:r["te"] + 1], mat, od, ed, oi, ei)
                assert box["score"] >= r["score"]
    assert n >= 50 and n_eq >= 0.97 * n


def test_the_transposed_reading_of_a_general_matrix_scores_differently(oracle):
    """The guard of the test above: the same 200 pairs scored by the DP under the transposed reading (query and target swapped,
    so mat[query][target], with the insertion and deletion penalties swapped along) differ from the oracle's 16-bit score on
    188 of 200 pairs (0.94, measured); half of that is asserted.  Were the share small, agreement with the DP would not tell
    the two readings apart."""
    differ = n = 0
    for seed in range(4):
        mat, (od, ed, oi, ei), pairs = general_pairs(seed)
        for q, t in pairs:
            r = oracle.align2(q, t, mat, od, ed, oi, ei, 0)
            tr = full_dp.local_dp(t, q, mat, oi, ei, od, ed)
            n += 1
            differ += r["score"] != tr["score"]
    print("transposed reading differs on %d of %d pairs" % (differ, n))
    assert n == 200 and differ >= 0.47 * n


def flanked(rng, L):
    q = rng.integers(0, 4, L).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 20), q, rng.integers(0, 4, 20)]).astype(np.uint8)
    return q, t


def test_known_answers_at_16_bit_saturation(oracle):
    """a = 127, b = 128: 258 matching bases score 32 766, the 259th reaches the cap of _mm_adds_epi16.  Past the cap only the score
    and the row that first holds it are analytic (qe is the first 32 767 of the kept column in memory order, and a gap-extended
    value just below the cap plus one match saturates too): the reported box is re-scored without a cap instead."""
    rng = np.random.default_rng(8)
    mat = bwa_mat(127, 128, -1)
    q, t = flanked(rng, 258)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XSTART)
    assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (32766, 277, 257, 20, 0)
    q, t = flanked(rng, 259)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XSTART)
    assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (32767, 278, 258, 20, 0)
    q, t = flanked(rng, 300)
    r = oracle.align2(q, t, mat, 6, 1, 6, 1, XSTART)
    assert r["score"] == 32767 and r["te"] == 278
    assert 0 <= r["tb"] <= r["te"] and 0 <= r["qb"] <= r["qe"] < 300
    box = full_dp.local_dp(q[r["qb"]:r["qe"] + 1], t[r["tb"]:r["te"] + 1], mat, 6, 1, 6, 1)
    assert box["score"] >= 32767


@pytest.mark.parametrize("smin", [0, -1, -100, -128])
@pytest.mark.parametrize("a", [1, 5])
def test_known_answers_for_the_byte_mode_shift(oracle, smin, a):
    """ksw_qinit's shift is -min(mat).  A query against itself scores a L exactly (no base matches twice) while a L + shift < 255;
    from there on the 8-bit run reports 255, at the first row whose H reaches the cap 255 - shift."""
    rng = np.random.default_rng(10)
    mat = np.full((5, 5), smin, dtype=np.int8)
    for k in range(4):
        mat[k, k] = a
    shift = -smin
    lo = (254 - shift) // a
    for L in (lo, lo + 1):
        q = rng.integers(0, 4, L).astype(np.uint8)
        r = oracle.align2(q, q.copy(), mat, 6, 1, 6, 1, XB | XSTART)
        if a * L + shift < 255:
            assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (a * L, L - 1, L - 1, 0, 0), (L, r)
        else:
            assert (r["score"], r["te"], r["qe"], r["tb"], r["qb"]) == (255, -(-(255 - shift) // a) - 1, -1, -1, -1), (L, r)
        w = oracle.align2(q, q.copy(), mat, 6, 1, 6, 1, XSTART)                     # the 16-bit run has no such limit
        assert (w["score"], w["te"], w["qe"], w["tb"], w["qb"]) == (a * L, L - 1, L - 1, 0, 0), (L, w)
    assert a * lo + shift < 255 <= a * (lo + 1) + shift


def test_batch_equals_single_calls(oracle, host):
    rng = np.random.default_rng(9)
    mat = bwa_mat()
    seqs, at = [], np.zeros(40, dtype=host.ATASK)
    for i in range(40):
        t = rng.integers(0, 4, int(rng.integers(20, 300))).astype(np.uint8)
        q = _gen.mutate(rng, t[5:5 + int(rng.integers(10, 120))], 60, 0.04, 0.02)
        seqs.append((q, t))
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"] = q.ctypes.data, t.ctypes.data, len(q), len(t)
        at[i]["xtra"] = XB | XSUBO | XSTART | 19
    out, cells = oracle.align2_batch(mat, 6, 1, 6, 1, at, nthreads=3)
    assert cells > 0
    for i, (q, t) in enumerate(seqs):
        r = oracle.align2(q, t, mat, 6, 1, 6, 1, int(at[i]["xtra"]))
        assert [r[k] for k in oracle.ALIGN_FIELDS] == out[i].tolist()
