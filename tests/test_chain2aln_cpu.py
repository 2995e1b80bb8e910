"""bsw_chain2aln_plan / bsw_chain2aln_replay without a GPU: hand-derived cases for every branch of mem_chain2aln's skip test (the
results are literal bsw_pair records, no DP runs), the differential against the sequential restatement (tests/_chain2aln_ref.py,
which extends a seed through the CPU oracle only when bwa's loop reaches it), what that workload exercises, every error code of the
plan, and the ABI side.

Default scoring (a = 1, o = 6, e = 1, w = 100): cal_max_gap(q) = min(max(q - 5, 1), 200)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _chain2aln_ref as R
import _rtl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ = 100
A = (1000, 40, 20, 50)                 # the first seed of most cases: on the diagonal rbeg - qbeg = 960, visited first
P = dict(rb=960, re=1060, qb=0, qe=100, w=10)          # the region it grows into: the whole read, no gap


def pair_for(host, seed, reg):
    """the record whose region (bsw_result_to_alnreg's arithmetic, by hand) is reg"""
    r = np.zeros(1, dtype=host.PAIR)
    rbeg, qbeg, ln = seed[:3]
    r["qb"], r["qe"] = reg["qb"], reg["qe"] - (qbeg + ln)
    r["rb"], r["re"] = reg["rb"] - rbeg, reg["re"] - (rbeg + ln)
    r["score"], r["truesc"], r["w"] = reg.get("score", 77), reg.get("truesc", 78), reg["w"]
    return r[0]


def replay(host, chains, regs_of, lens=(LQ,), opt=None, full=False):
    """chains: [(read, [seeds])]; regs_of: {(chain, index): region} (default: the seed itself, w = 10) -> (CREG, extended)"""
    ch = np.zeros(len(chains), dtype=host.CHAIN)
    sd, res, at = [], [], 0
    for c, (read, seeds) in enumerate(chains):
        ch[c] = (read, len(seeds), at, 0, 0, 7 + c, 0.25 * (c + 1))
        for i, s in enumerate(seeds):
            own = dict(rb=s[0], re=s[0] + s[2], qb=s[1], qe=s[1] + s[2], w=10)
            sd.append((s[0], s[1], s[2], s[3], 0))
            res.append(pair_for(host, s, regs_of.get((c, i), own)))
            res[-1]["tag"] = at
            at += 1
    sd = np.array(sd, dtype=host.CSEED)
    res = np.array(res, dtype=host.PAIR)
    if full:
        f = np.zeros(len(res), dtype=host.RESULT)
        for n in host.PAIR.names:
            f[n] = res[n]
        f["left"]["cells"] = 0xdeadbeef
        res = f
    regs, ext, start = host.chain2aln_replay(host.default_params(), ch, sd, np.array(lens, dtype=np.int32), res, opt=opt)
    assert int(start[-1]) == len(regs) and int(ext.sum()) == len(regs)
    return regs, [int(x) for x in ext]


def one(host, s, region=P, first=A, opt=None):
    """is s (visited second) extended beside the region of `first`?"""
    _, ext = replay(host, [(0, [first, s])], {(0, 0): region}, opt=opt)
    assert ext[0] == 1
    return ext[1]


def test_region_fields_and_a_contained_seed(host):
    for full in (False, True):
        regs, ext = replay(host, [(0, [A, (990, 30, 10, 40), (1070, 90, 10, 30)])], {(0, 0): dict(P, re=1058, qe=98, score=91, truesc=93)}, full=full)
        assert ext == [1, 0, 1]                    # the second lies on the region's diagonal; the third ends behind it (1080 > 1058)
        a = regs[0]
        assert (a["rb"], a["re"], a["qb"], a["qe"], a["score"], a["truesc"], a["w"]) == (960, 1058, 0, 98, 91, 93, 10)
        assert (a["seedlen0"], a["rid"], float(a["frac_rep"]), a["read"], a["chain"], a["seed"]) == (20, 7, 0.25, 0, 0, 0)
        assert a["seedcov"] == 20 + 10             # the skipped seed counts, the one outside does not
        assert (regs[1]["seed"], regs[1]["seedlen0"], regs[1]["seedcov"]) == (2, 10, 10)


def test_not_contained_on_each_of_the_four_sides(host):
    p = dict(rb=965, re=1055, qb=5, qe=95, w=10)
    assert one(host, (975, 15, 10, 40), p) == 0            # inside on all four: skipped
    assert one(host, (964, 5, 10, 40), p) == 1             # rbeg < rb
    assert one(host, (1046, 85, 10, 40), p) == 1           # rbeg + len > re
    assert one(host, (965, 4, 10, 40), p) == 1             # qbeg < qb
    assert one(host, (1045, 86, 10, 40), p) == 1           # qbeg + len > qe
    assert one(host, (965, 5, 10, 40), p) == 0 and one(host, (1045, 85, 10, 40), p) == 0        # flush with the region: contained


def test_seedlen0_test_at_its_boundary(host):
    assert .1 * LQ == 10.0
    assert one(host, (970, 10, 30, 40)) == 0               # 30 - 20 == 0.1 * 100: not "more than": explained
    assert one(host, (970, 10, 31, 40)) == 1               # 31 - 20 > 10: this seed may give a better alignment
    assert one(host, (970, 10, 31, 40), opt=dict(seedlen0_frac=-1.0)) == 0     # the 0.7.8 behaviour
    assert one(host, (970, 10, 25, 40), opt=dict(seedlen0_frac=.04)) == 1      # 5 > 4


def test_ahead_and_behind(host):
    p = dict(rb=960, re=1064, qb=0, qe=100, w=2)           # four more reference bases than query bases; band 2
    assert one(host, (1030, 70, 10, 40), p) == 0           # on the diagonal of the region's start: the test ahead hits
    assert one(host, (1031, 70, 10, 40), p) == 0           # one off (1 < 2)
    assert one(host, (1034, 70, 10, 40), p) == 0           # on the diagonal of its end: ahead misses (4 >= 2), behind hits
    assert one(host, (1033, 70, 10, 40), p) == 0
    assert one(host, (1032, 70, 10, 40), p) == 1           # two off either way: neither hits


def test_band_bounded_by_the_region_or_by_cal_max_gap(host):
    p = dict(rb=960, re=1180, qb=0, qe=100, w=50)          # 120 more reference bases
    # 7 bases ahead of the seed: cal_max_gap(7) = 2 < 50
    assert one(host, (968, 7, 10, 40), p) == 0             # 1 < 2
    assert one(host, (969, 7, 10, 40), p) == 1             # 2 >= 2 (2 < 50 would have hit); behind: 118 >= min(cal_max_gap(83), 50)
    # 60 bases ahead: cal_max_gap(60) = 55 > 50 = p.w
    assert one(host, (1069, 60, 10, 40), p) == 0           # 49 < 50
    assert one(host, (1072, 60, 10, 40), p) == 1           # 52 >= 50 (52 < 55 would have hit); behind: 68 >= cal_max_gap(30) = 25


def test_overlap_rescue_by_either_condition(host):
    assert one(host, (990, 30, 20, 45)) == 0               # same diagonal as A: explained, and A cannot un-skip it
    assert one(host, (983, 30, 20, 45)) == 1               # s in front of A, 10 >= 20 >> 2 bases over it, 10 != 17: first condition
    assert one(host, (1003, 50, 20, 45)) == 1              # A in front of s, 10 bases over it, 10 != 3: second condition
    assert one(host, (1023, 56, 20, 45)) == 0 and one(host, (1022, 55, 20, 45)) == 1     # 4 < 5 bases over A; 5 >= 5


def test_rescue_needs_a_long_enough_seed(host):
    assert .95 * 20 == 19.0
    s = (1003, 50, 20, 45)
    assert one(host, s, first=(1000, 40, 19, 50)) == 1     # 19 < 0.95 * 20 is false
    assert one(host, s, first=(1000, 40, 18, 50)) == 0
    assert one(host, s, first=(1000, 40, 18, 50), opt=dict(ovl_len_frac=.9)) == 1


def test_rescue_ignores_a_seed_marked_zero(host):
    b, c = (1030, 70, 20, 45), (1033, 75, 20, 40)          # b on the region's diagonal; c two off, 15 bases over b, out of A's reach
    _, ext = replay(host, [(0, [A, b, c])], {(0, 0): P})
    assert ext == [1, 0, 0]                                # b is skipped and marked, so it cannot un-skip c
    _, ext = replay(host, [(0, [A, (b[0], b[1], b[2], 60), c])], {(0, 0): P})
    assert ext == [1, 1, 1]                                # b visited first and extended: now it does


def test_score_zero_at_index_zero(host):
    # srt[] of (score 0, index 0) is the skip mark itself; it sorts first, is visited last, and nothing reads it afterwards
    _, ext = replay(host, [(0, [(990, 30, 10, 0), A])], {(0, 1): P})
    assert ext == [0, 1]
    regs, ext = replay(host, [(0, [(959, 30, 10, 0), A, (1003, 50, 20, 0)])], {(0, 1): P})       # 959 < rb: not contained
    assert ext == [1, 1, 1] and [int(x) for x in regs["seed"]] == [1, 2, 0]       # index 2 before index 0 among the zero scores


def test_equal_scores_visit_the_larger_index_first(host):
    s0, s1 = (1000, 40, 20, 50), (1005, 45, 20, 50)
    regs, ext = replay(host, [(0, [s0, s1])], {(0, 0): P, (0, 1): P})
    assert ext == [0, 1] and int(regs[0]["seed"]) == 1 and int(regs[0]["seedcov"]) == 40
    regs, ext = replay(host, [(0, [s0, (1005, 45, 20, 49)])], {(0, 0): P, (0, 1): P})
    assert ext == [1, 0]


def test_a_second_chains_seed_explained_by_the_first_chains_region(host):
    s = (990, 30, 10, 40)
    regs, ext = replay(host, [(0, [A]), (0, [s]), (1, [s])], {(0, 0): P}, lens=(LQ, LQ))
    assert ext == [1, 0, 1]                                # the list is the read's, not the chain's; the next read starts empty
    assert [int(x) for x in regs["chain"]] == [0, 2] and [int(x) for x in regs["read"]] == [0, 1]
    assert (int(regs[1]["rid"]), float(regs[1]["frac_rep"])) == (9, 0.75)


def test_reg_start_with_reads_without_chains(host):
    s = (990, 30, 10, 40)
    ch = np.zeros(2, dtype=host.CHAIN)
    ch[0], ch[1] = (1, 1, 0, 0, 0, 0, 0), (3, 1, 1, 0, 0, 0, 0)
    sd = np.array([s + (0,), s + (0,)], dtype=host.CSEED)
    res = np.zeros(2, dtype=host.PAIR)
    regs, ext, start = host.chain2aln_replay(host.default_params(), ch, sd, np.full(5, LQ, dtype=np.int32), res)
    assert [int(x) for x in start] == [0, 0, 1, 1, 2, 2] and len(regs) == 2


# ---- the differential ----------------------------------------------------------------------------------------------------------------

N_READS = 2000


@pytest.fixture(scope="module")
def wl():
    return R.make_workload(N_READS, seed=11)


@pytest.fixture(scope="module")
def planned(host, wl):
    ch, sd, lens = R.arrays(host, wl)
    rdt, rft = host.chain2aln_plan(host.default_params(), wl["l_pac"], ch, sd, lens, reads=wl["reads"])
    items = [(int(t["read"]), int(t["seed"]["rbeg"]), int(t["seed"]["qbeg"]), int(t["seed"]["len"]), int(t["rmax0"]), int(t["rmax1"]), int(t["tag"])) for t in rdt]
    tasks, keep = R.build_tasks(host, R.pen_of(host.default_params()), wl["reads"], wl["both"], items)
    return ch, sd, lens, rdt, rft, tasks, keep


@pytest.fixture(scope="module")
def reference(host, oracle, wl):
    """the sequential restatement, once per variant"""
    out = {}
    for v in (0, 1, 2):
        p = host.default_params(variant=v)
        ex = R.Extender(host, oracle, _rtl_ref, p, wl)
        regs, extended, cnt = R.chain2aln(ex, p, wl)
        assert ex.calls == cnt["extended"] == len(regs)    # a skipped seed never reached the oracle
        out[v] = (regs, extended, cnt)
    return out


def test_plan_lays_out_bwas_tasks(host, wl, planned):
    ch, sd, lens, rdt, rft, tasks, _ = planned
    pen = R.pen_of(host.default_params())
    assert (rdt["tag"] == np.arange(len(sd))).all() and (rdt["init_score"] == -1).all() and (rft["init_score"] == -1).all()
    at = 0
    for c in wl["chains"]:
        r0, r1, _, _ = R.chain_window(pen, c["seeds"], len(wl["reads"][c["read"]]), wl["l_pac"], c["rlo"], c["rhi"])
        n = len(c["seeds"])
        assert (rdt["rmax0"][at:at + n] == r0).all() and (rdt["rmax1"][at:at + n] == r1).all() and (rdt["read"][at:at + n] == c["read"]).all()
        assert (rft["query"][at:at + n] == wl["reads"][c["read"]].ctypes.data).all() and (rft["l_query"][at:at + n] == lens[c["read"]]).all()
        at += n
    for f in ("rbeg", "qbeg", "len"):
        assert (rdt["seed"][f] == sd[f]).all() and (rft["seed"][f] == sd[f]).all()
    assert (rft["rmax0"] == rdt["rmax0"]).all() and (rft["rmax1"] == rdt["rmax1"]).all() and (rft["tag"] == rdt["tag"]).all()


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("pair", [False, True])
def test_plan_oracle_replay_equals_the_sequential_reference(host, oracle, wl, planned, reference, variant, pair):
    ch, sd, lens, rdt, rft, tasks, _ = planned
    p = host.default_params(variant=variant)
    res = R.run_oracle(oracle, _rtl_ref, p, tasks, nthreads=8)
    assert (res["tag"] == np.arange(len(sd))).all()
    if pair:
        q = np.zeros(len(res), dtype=host.PAIR)
        for f in host.PAIR.names:
            q[f] = res[f]
        res = q
    regs, ext, start = host.chain2aln_replay(p, ch, sd, lens, res)
    want, wext, _ = reference[variant]
    assert R.same_regions(regs, want) is None, R.same_regions(regs, want)
    assert [int(x) for x in ext] == [int(x) for x in wext]
    counts = np.bincount([a["read"] for a in want], minlength=len(lens))
    assert (np.diff(start.astype(np.int64)) == counts).all()


def test_the_workload_exercises_what_it_claims(wl, reference):
    _, _, c = reference[0]
    print(c)
    assert 0.10 <= 1 - c["extended"] / c["seeds"] <= 0.90
    for k in ("rescued", "cross_chain_skips", "seedlen0_exempt", "clamped", "bridged", "qbeg0", "qend"):
        assert c[k] >= 1, k
    per = np.bincount([ch["read"] for ch in wl["chains"]], minlength=N_READS)
    assert per.min() >= 1 and per.max() == 5 and 100 <= min(len(r) for r in wl["reads"]) and max(len(r) for r in wl["reads"]) <= 250
    assert 9 * N_READS <= c["seeds"] <= 14 * N_READS           # 3 - 4 k seeds per 300 reads


# ---- the plan's error codes -----------------------------------------------------------------------------------------------------------

def plan_rc(host, chains, seeds, lens, l_pac=200003, params=None, reads=None, **kw):
    try:
        host.chain2aln_plan(params if params is not None else host.default_params(), l_pac, np.array(chains, dtype=host.CHAIN),
                            np.array(seeds, dtype=host.CSEED), np.array(lens, dtype=np.int32), reads=reads)
    except host.BswError as e:
        assert str(e).count("bsw_chain2aln_plan") == 1, str(e)
        return e.code
    return 0


def test_every_error_code_of_the_plan(host):
    INVAL, LIMIT = -2, -3
    good_c, good_s = [(0, 2, 0, 0, 0, 0, 0)], [(1000, 40, 20, 20, 0), (1030, 70, 30, 30, 0)]
    assert plan_rc(host, good_c, good_s, [100]) == 0
    assert plan_rc(host, good_c, [(1000, 40, 20, 20, 0), (1030, 70, 31, 30, 0)], [100]) == INVAL         # the seed ends behind its read
    assert plan_rc(host, good_c, [(1000, -1, 20, 20, 0), good_s[1]], [100]) == INVAL
    assert plan_rc(host, good_c, [(1000, 40, 0, 20, 0), good_s[1]], [100]) == INVAL
    assert plan_rc(host, good_c, [(1000, 40, 20, -1, 0), good_s[1]], [100]) == INVAL                    # a negative score
    assert plan_rc(host, good_c, [(-1, 40, 20, 20, 0), good_s[1]], [100]) == INVAL
    assert plan_rc(host, good_c, [(400000, 40, 20, 20, 0), good_s[1]], [100]) == INVAL                  # rbeg + len > 2 * l_pac
    assert plan_rc(host, [(1, 2, 0, 0, 0, 0, 0)], good_s, [100]) == INVAL                               # read >= n_reads
    assert plan_rc(host, [(0, 0, 0, 0, 0, 0, 0)], good_s, [100]) == INVAL                               # a chain without a seed
    assert plan_rc(host, [(0, 1, 0, 0, 0, 0, 0)], good_s, [100]) == INVAL                               # a seed no chain holds
    assert plan_rc(host, [(0, 1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0)], good_s, [100]) == INVAL         # first_seed does not follow
    assert plan_rc(host, [(0, 3, 0, 0, 0, 0, 0)], good_s, [100]) == INVAL
    three = [(0, 1, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0, 0), (0, 1, 2, 0, 0, 0, 0)]
    assert plan_rc(host, three, good_s + [good_s[0]], [100, 100]) == INVAL                              # the chains of read 0 are not contiguous
    assert plan_rc(host, [three[0], three[1], (1, 1, 2, 0, 0, 0, 0)], good_s + [good_s[0]], [100, 100]) == 0
    assert plan_rc(host, [(0, 2, 0, -5, 3000, 0, 0)], good_s, [100]) == INVAL                           # a contig interval outside [0, 2 * l_pac)
    assert plan_rc(host, [(0, 2, 0, 1010, 3000, 0, 0)], good_s, [100]) == INVAL                         # a seed outside its chain's contig
    assert plan_rc(host, [(0, 2, 0, 1000, 1060, 0, 0)], good_s, [100]) == 0
    assert plan_rc(host, good_c, good_s, [100], l_pac=0) == INVAL
    bad = host.default_params()
    bad["e_del"] = 0
    assert plan_rc(host, good_c, good_s, [100], params=bad) == INVAL
    # a window side beyond BSW_MAX_TLEN: 35 000 read bases ahead of the seed, and a band that lets the gap grow as long
    wide = host.default_params(w=40000)
    long_s = [(100000, 35000, 20, 20, 0)]
    assert plan_rc(host, [(0, 1, 0, 0, 0, 0, 0)], long_s, [36000], params=wide) == LIMIT
    assert plan_rc(host, [(0, 1, 0, 0, 0, 0, 0)], long_s, [36000]) == 0                                 # w = 100: 35 000 + 200 bases
    assert plan_rc(host, [(0, 1, 0, 100000 - 65535, 150000, 0, 0)], long_s, [36000], params=wide) == 0      # the contig clamp brings it to the limit
    assert plan_rc(host, [(0, 1, 0, 100000 - 65536, 150000, 0, 0)], long_s, [36000], params=wide) == LIMIT
    # NULL arrays, and pointer tasks without reads
    L = host.lib()
    p = host.default_params()
    ch, sd, ln = np.array(good_c, dtype=host.CHAIN), np.array(good_s, dtype=host.CSEED), np.array([100], dtype=np.int32)
    rft = np.zeros(2, dtype=host.REF_TASK)
    err = C.create_string_buffer(400)
    assert L.bsw_chain2aln_plan(p.ctypes.data, 200003, ch.ctypes.data, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, None, None, rft.ctypes.data, err, 400) == INVAL
    assert L.bsw_chain2aln_plan(None, 200003, ch.ctypes.data, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, None, None, None, None, 0) == INVAL
    assert L.bsw_chain2aln_plan(p.ctypes.data, 200003, None, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, None, None, None, err, 400) == INVAL and err.value
    assert L.bsw_chain2aln_plan(p.ctypes.data, 200003, ch.ctypes.data, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, None, None, None, None, 0) == 0      # a dry run
    assert L.bsw_chain2aln_plan(p.ctypes.data, 200003, None, 0, None, 0, None, 0, None, None, None, None, 0) == 0
    n = C.c_size_t(9)
    assert L.bsw_chain2aln_replay(p.ctypes.data, None, None, 0, None, 0, None, 0, None, 0, None, C.byref(n), None, None) == 0 and n.value == 0
    assert L.bsw_chain2aln_replay(p.ctypes.data, None, ch.ctypes.data, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, None, 0, None, C.byref(n), None, None) == INVAL
    res = np.zeros(2, dtype=host.RESULT)
    regs = np.zeros(2, dtype=host.CREG)
    assert L.bsw_chain2aln_replay(p.ctypes.data, None, ch.ctypes.data, 1, sd.ctypes.data, 2, ln.ctypes.data, 1, res.ctypes.data, 2, regs.ctypes.data, C.byref(n), None, None) == INVAL


# ---- the ABI side --------------------------------------------------------------------------------------------------------------------

NAMES = ["bsw_c2a_default_opt", "bsw_chain2aln_plan", "bsw_chain2aln_replay", "bsw_chain2aln_ref_start", "bsw_chain2aln_reads_start",
         "bsw_chain2aln_test", "bsw_chain2aln_finish", "bsw_chain2aln_stats"]


def test_exports_header_and_abi(built, host, tmp_path):
    syms = subprocess.check_output(["nm", "-D", "--defined-only", built.lib_path()], text=True)
    hdr = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    for f in NAMES:
        assert " T %s\n" % f in syms, f
        assert re.search(r"\b%s\(" % f, hdr), f
        assert f in host.EXPORTS, f
    assert host.lib().bsw_abi_version() == 6 and "#define BSW_ABI_VERSION 6" in hdr
    assert "as recalled" in hdr.lower()
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwa_sw_mi355.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(bsw_cseed),sizeof(bsw_chain),sizeof(bsw_creg),sizeof(bsw_c2a_opt),sizeof(bsw_c2a_stats),sizeof(bsw_alnreg),'
                   'offsetof(bsw_creg,seedcov),offsetof(bsw_chain,rlo));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [host.CSEED.itemsize, host.CHAIN.itemsize, host.CREG.itemsize, host.C2A_OPT.itemsize, host.C2A_STATS.itemsize,
                     host.ALNREG.itemsize, host.CREG.fields["seedcov"][1], host.CHAIN.fields["rlo"][1]]
    o = host.c2a_opt()
    assert (float(o["seedlen0_frac"][0]), float(o["ovl_len_frac"][0])) == (.1, .95)
