"""mem_patch_reg without a GPU: the two host-only halves of bsw_patch_ref_batch (bsw_patch_pretest, bsw_patch_decide) against
tests/_patch_ref.py on random region pairs and at hand-made boundaries, and the ABI of the new calls with its Python mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _patch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_PAC = 10_000_000


def preg(host, r):
    a = np.zeros(1, dtype=host.PREG)
    for k in ("rb", "re", "qb", "qe", "score", "w"):
        a[k] = r[k]
    return a


def params_w(host, w):
    p = host.default_params()
    p["w"] = w
    return p


def lib_pretest(host, opt_w, a, b, l_pac=L_PAC):
    return host.patch_pretest(params_w(host, opt_w), l_pac, preg(host, a), preg(host, b))


def lib_decide(host, a, b, gscore):
    return host.patch_decide(preg(host, a), preg(host, b), gscore)


def draw_pair(rng):
    """two regions of one read the way chains leave them: b behind a by a few bases, sometimes by many, sometimes out of order"""
    la, lb = int(rng.integers(30, 121)), int(rng.integers(30, 121))
    aqb = int(rng.integers(0, 50))
    aqe = aqb + la
    dq = int(rng.integers(-20, 31))
    bqb = max(aqe + dq, aqb + 1)
    bqe = bqb + lb
    rev = rng.random() < 0.5
    arb = int(rng.integers(1000, L_PAC - 5000)) + (L_PAC if rev else 0)
    are = arb + la + int(rng.integers(-3, 4))
    u = rng.random()
    extra = int(rng.integers(-12, 13)) if u < 0.5 else int(rng.integers(-60, 61)) if u < 0.75 else int(rng.integers(-600, 601))
    brb = max(are + (bqb - aqe) + extra, arb)
    bre = brb + lb + int(rng.integers(-3, 4))
    v = rng.random()
    if v < 0.04:                         # the other strand
        if not rev:
            brb += L_PAC
            bre += L_PAC
    elif v < 0.06:                       # not colinear on the read
        bqb, bqe = aqb, aqb + lb
    elif v < 0.08:                       # ... or b ends inside a (on the read, on the reference)
        if rng.random() < 0.5:
            bqe = min(bqe, aqe)
            bqb = min(bqb, bqe - 1)
        else:
            bre = are
            brb = min(brb, bre - 1)
    a = P.reg(arb, are, aqb, aqe, la - int(rng.integers(0, 12)), int(rng.integers(0, 30)))
    b = P.reg(brb, bre, bqb, bqe, lb - int(rng.integers(0, 12)), int(rng.integers(0, 30)))
    return a, b


def test_pretest_and_decide_against_the_restatement(host):
    rng = np.random.default_rng(20260)
    params = {w: params_w(host, w) for w in (8, 25, 100)}
    why = {}
    gap = {True: 0, False: 0}
    kept = rejected = 0
    for k in range(24000):
        a, b = draw_pair(rng)
        opt_w = (100, 100, 25, 8)[k % 4]
        want = P.pretest(opt_w, L_PAC, a, b)
        got = host.patch_pretest(params[opt_w], L_PAC, preg(host, a), preg(host, b))
        assert got == want[:2], (k, a, b, opt_w, got, want)
        why[want[2]] = why.get(want[2], 0) + 1
        if want[2] not in (P.STRAND, P.COLINEAR):
            gap[a["re"] < b["rb"] or a["qe"] < b["qb"]] += 1
        q_s, r_s = P.expected_scores(a, b)
        m = max(q_s, r_s)
        u = rng.random()
        gscore = int(0.9 * m) + int(rng.integers(-3, 4)) if u < 0.6 else int(rng.integers(-50, m + 20))
        ret = P.decide(a, b, gscore)
        assert host.patch_decide(preg(host, a), preg(host, b), gscore) == ret, (k, a, b, gscore)
        if want[0]:
            kept += ret > 0
            rejected += ret == 0
    for name in (P.STRAND, P.COLINEAR, P.GAP_W, P.GAP_R, P.OVL_W, P.OVL_R, P.RUNS):
        assert why.get(name, 0) >= 100, why
    assert gap[True] >= 100 and gap[False] >= 100, gap
    assert kept >= 100 and rejected >= 100, (kept, rejected)    # the fifth early return (the 0.90f ratio), and its other side


# two regions of 10 000 bases: long enough that a band of 4 * 100 bases still passes the ratio test
def long_pair(q_step, r_step):
    """b starts q_step bases behind a's end on the read and r_step bases behind it on the reference (negative: they overlap)"""
    a = P.reg(100000, 110000, 0, 10000, 9000, 0)
    b = P.reg(110000 + r_step, 120000 + r_step, 10000 + q_step, 20000 + q_step, 9000, 0)
    return a, b


@pytest.mark.parametrize("q_step,r_step,runs,w,why", [
    (10, 210, 1, 200, P.RUNS),           # a gap between them: w == opt->w << 1 still runs ...
    (10, 211, 0, 0, P.GAP_W),            # ... one more does not
    (-10, -410, 1, 400, P.RUNS),         # they overlap: w == opt->w << 2 runs ...
    (-10, -411, 0, 0, P.OVL_W),          # ... one more does not
])
def test_band_limits_of_both_branches(host, q_step, r_step, runs, w, why):
    a, b = long_pair(q_step, r_step)
    assert P.pretest(100, L_PAC, a, b) == (runs, w, why)
    assert lib_pretest(host, 100, a, b) == (runs, w)


def test_band_handed_over_adds_the_regions_bands_and_is_capped(host):
    a, b = long_pair(10, 210)
    a["w"], b["w"] = 50, 70
    assert P.pretest(100, L_PAC, a, b)[:2] == lib_pretest(host, 100, a, b) == (1, 320)
    a["w"] = 500
    assert P.pretest(100, L_PAC, a, b)[:2] == lib_pretest(host, 100, a, b) == (1, 400)


def test_ratio_limits_are_float_constants(host):
    # r == 0.05 exactly, the issue's figures (a.re - b.rb = 10, b.re - a.rb = 200, a.qe == b.qb)
    a, b = P.reg(1000, 1100, 0, 100, 90), P.reg(1090, 1200, 100, 200, 90)
    assert P.pretest(100, L_PAC, a, b) == (1, 10, P.RUNS) and lib_pretest(host, 100, a, b) == (1, 10)
    # ... and where 0.05 is the limit: a gap of 10 on the reference, none on the read.  0.05 < 0.05f, so it runs
    a, b = P.reg(1000, 1095, 0, 95, 90), P.reg(1105, 1200, 95, 190, 90)
    assert (a["re"] - b["rb"]) / (b["re"] - a["rb"]) == -0.05
    assert P.pretest(100, L_PAC, a, b) == (1, 10, P.RUNS) and lib_pretest(host, 100, a, b) == (1, 10)
    b = P.reg(1105, 1199, 95, 190, 90)                       # a little above
    assert P.pretest(100, L_PAC, a, b) == (0, 0, P.GAP_R) and lib_pretest(host, 100, a, b) == (0, 0)
    # r == 0.1 exactly where they overlap: 0.1 < 0.05f * 2
    a, b = P.reg(1000, 1100, 0, 100, 90), P.reg(1080, 1200, 100, 200, 90)
    assert (a["re"] - b["rb"]) / (b["re"] - a["rb"]) == 0.1
    assert P.pretest(100, L_PAC, a, b) == (1, 20, P.RUNS) and lib_pretest(host, 100, a, b) == (1, 20)
    b = P.reg(1079, 1200, 100, 200, 90)
    assert P.pretest(100, L_PAC, a, b) == (0, 0, P.OVL_R) and lib_pretest(host, 100, a, b) == (0, 0)


def test_strands_and_order(host):
    a, b = P.reg(L_PAC - 200, L_PAC - 100, 0, 100, 90), P.reg(L_PAC, L_PAC + 100, 100, 200, 90)
    assert P.pretest(100, L_PAC, a, b)[2] == P.STRAND and lib_pretest(host, 100, a, b) == (0, 0)
    a = P.reg(L_PAC + 10, L_PAC + 110, 0, 100, 90)           # both on the reverse strand
    b = P.reg(L_PAC + 110, L_PAC + 210, 100, 200, 90)
    assert P.pretest(100, L_PAC, a, b) == (1, 0, P.RUNS) and lib_pretest(host, 100, a, b) == (1, 0)
    for bad in (dict(qb=0), dict(qe=100), dict(re=L_PAC + 110, rb=L_PAC + 20)):
        b2 = dict(b, **bad)
        assert P.pretest(100, L_PAC, a, b2)[2] == P.COLINEAR and lib_pretest(host, 100, a, b2) == (0, 0)


def test_expected_scores_round_at_499(host):
    """q_s and r_s are (int)(x + .499): x = k + .501 reaches k + 1, x = k + .5 does not.  Seen through the return value: the
    smallest gscore that is kept is the first with gscore / max(q_s, r_s) >= 0.90f."""
    edges = 0
    for span, total in ((1001, 1000), (999, 1000), (1003, 1000)):
        for s in range(2, 1400, 3):
            # the regions' own lengths add up to `total` on both sides, the joined spans are `span`
            a = P.reg(5000, 5000 + total // 2, 0, total // 2, s // 2)
            b = P.reg(5000 + span - total // 2, 5000 + span, span - total // 2, span, s - s // 2)
            q_s, r_s = P.expected_scores(a, b)
            x = span / total * s
            edges += abs((x + .499) - round(x + .499)) < 2e-3
            m = max(q_s, r_s)
            for g in range(int(0.9 * m) - 2, int(0.9 * m) + 3):
                assert lib_decide(host, a, b, g) == P.decide(a, b, g), (span, s, g)
    assert edges >= 3
    # 1001 / 1000 * 501 = 501.501: with .499 it is 502 or a hair below, as IEEE double has it; both sides agree above.  By hand:
    a, b = P.reg(5000, 5500, 0, 500, 250), P.reg(5500, 6000, 500, 1000, 250)
    assert P.expected_scores(a, b) == (500, 500)
    a, b = P.reg(5000, 5500, 0, 500, 250), P.reg(5501, 6001, 500, 1000, 251)     # r_s = (int)(1001 / 1000 * 501 + .499), q_s = 501
    assert P.expected_scores(a, b)[0] == 501 and P.expected_scores(a, b)[1] in (501, 502)


def test_ratio_either_side_of_090(host):
    a, b = P.reg(5000, 5050, 0, 50, 50), P.reg(5050, 5100, 50, 100, 50)          # q_s = r_s = 100
    assert P.expected_scores(a, b) == (100, 100)
    for g, want in ((91, 91), (90, 90), (89, 0), (1, 0), (0, 0), (-7, 0), (-(1 << 30), 0), (250, 250)):
        assert P.decide(a, b, g) == want and lib_decide(host, a, b, g) == want, g
    # 0.90f is a little BELOW 0.9: 9 / 10 and 90 / 100 are kept; just under them is not
    a, b = P.reg(5000, 5500, 0, 500, 500), P.reg(5500, 6000, 500, 1000, 500)    # 1 000
    for g, want in ((900, 900), (899, 0)):
        assert P.decide(a, b, g) == want and lib_decide(host, a, b, g) == want


# ---- the ABI and its mirror ----
NEW = ["bsw_patch_ref_batch", "bsw_patch_ref_submit_t", "bsw_patch_reads_submit_t", "bsw_patch_pretest", "bsw_patch_decide"]


def test_struct_sizes(host, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwa_sw_mi355.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(bsw_preg),sizeof(bsw_ptask),sizeof(bsw_rd_ptask),sizeof(bsw_presult),offsetof(bsw_ptask,a),'
                   'offsetof(bsw_ptask,b),offsetof(bsw_rd_ptask,b));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [32, 80, 72, 16, 16, 48, 40]
    assert [host.PREG.itemsize, host.PTASK.itemsize, host.RD_PTASK.itemsize, host.PRESULT.itemsize] == sizes[:4]
    assert [host.PTASK.fields["a"][1], host.PTASK.fields["b"][1], host.RD_PTASK.fields["b"][1]] == sizes[4:]


def test_symbols_version_and_threads(host):
    L = C.CDLL(host.lib_path())
    for n in NEW:
        assert hasattr(L, n), n
        assert n in host.EXPORTS, n
    assert L.bsw_abi_version() == 6
    text = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")].split("every other call")[0]
    assert "bsw_patch_ref_submit_t" in threads and "bsw_patch_reads_submit_t" in threads
    assert "bsw_patch_ref_batch" not in threads                 # the synchronous call needs the context to itself
    assert re.search(r"mem_patch_reg", text)
