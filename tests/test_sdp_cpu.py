"""bsw_sdp_* without a GPU: the engine of bsw_sdp.c driven through host.py's SdpEngine, with tests/_patch_ref.py::patch_reg standing
in for the GPU in the needs / feed loop, against the sequential restatement in tests/_sdp_ref.py: every field of every surviving
region, out_start and the counts; what the workload must contain is asserted on the restatement first.  Then the rounds, the
speculation, stale results, presorted, patch = 0, every refusal of open, bsw_sdp_from_cregs, the ABI, and the regions of
bsw_chain2aln_replay through the engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _chain2aln_ref as CR
import _patch_ref as P
import _sdp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL = -2


@pytest.fixture(scope="module")
def params(host):
    return host.default_params()


@pytest.fixture(scope="module")
def work(host, oracle, params):
    """the workload, its arrays, the oracle behind mem_patch_reg and the restatement's answer: computed once, left unchanged"""
    wl = S.make_workload()
    patcher = S.Patcher(host, oracle, params, wl)
    want = S.sdp(wl, patcher)
    patcher.reached = set(patcher.memo)                        # (read, 12 values) of every pair the sequential loop aligned
    return wl, S.arrays(host, wl), patcher, want


def answer(host, patcher, tasks, wrong=None):
    """what the patch ticket would write for these RD_PTASK records; wrong(read, a, b) -> True: a deliberately wrong merge"""
    res = np.zeros(len(tasks), dtype=host.PRESULT)
    for k, t in enumerate(tasks):
        a, b = ({f: int(t[nm][f]) for f in S.PREG} for nm in ("a", "b"))
        r = patcher(int(t["read"]), a, b)
        res[k] = (r["score"], r["w"], r["gscore"], r["status"])
        if wrong is not None and wrong(int(t["read"]), a, b):
            res[k] = (4000, 1, 4000, 0)
    return res


def run_engine(host, patcher, params, wl, arrs, opt=None, on_round=None):
    """-> (regions, out_start, stats, tasks per round)"""
    regs, start, lens = arrs
    per_round = []
    with host.SdpEngine(params, wl["l_pac"], regs, start, lens, opt=opt) as e:
        while True:
            t = e.needs()
            if not len(t):
                break
            per_round.append(t)
            e.feed(on_round(len(per_round), t) if on_round else answer(host, patcher, t))
        return e.collect() + (per_round,)


def test_the_workload_holds_every_case(work):
    wl, _, _, (out, start, cnt, rounds) = work
    assert 300 <= len(wl["reads"]) <= 400
    assert cnt["merges"] >= 20, cnt
    for r in (1, 2, 3):
        assert rounds.count(r) >= 5, (r, [rounds.count(k) for k in range(6)])
    assert cnt["kills_p"] >= 5 and cnt["kills_q"] >= 5, cnt
    assert cnt["float_edge_mr100"] >= 1, cnt
    assert cnt["rid_hidden"] >= 1 and cnt["equal_re"] >= 2 and cnt["dups"] >= 3 and cnt["dup_runs3"] >= 1, cnt
    assert cnt["noaln"] >= 1 and cnt["not_merged"] >= 1, cnt
    for why in (P.STRAND, P.COLINEAR, P.GAP_W, P.GAP_R, P.OVL_W, P.OVL_R, P.RUNS):
        assert cnt["why"].get(why, 0) >= 1, (why, cnt["why"])
    n_regs = [len(r) for r in wl["regs"]]
    assert n_regs.count(0) >= 1 and n_regs.count(1) >= 1
    one = [i for i, r in enumerate(wl["regs"]) if len(r) == 1 and r[0]["n_comp"] == 7]
    assert one and all(out[start[i]]["n_comp"] == 7 and start[i + 1] == start[i] + 1 for i in one)
    assert sum(1 for r in out if r["rb"] >= wl["l_pac"] and r["n_comp"] > 1) >= 5          # merges on the reverse strand


def test_engine_equals_the_restatement(host, params, work):
    wl, arrs, patcher, (want, want_start, cnt, rounds) = work
    out, start, st, per_round = run_engine(host, patcher, params, wl, arrs)
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert list(start) == want_start
    assert S.same_stats(st, cnt, len(wl["reads"]), len(arrs[0]), len(want)) is None, S.same_stats(st, cnt, len(wl["reads"]), len(arrs[0]), len(want))
    assert len(per_round) == max(rounds) == 3 and st["rounds"] == 3
    # the reads that ask in round k are the reads the restatement gives k or more rounds
    for k, t in enumerate(per_round):
        assert sorted(set(int(x) for x in t["read"])) == [i for i, r in enumerate(rounds) if r > k]


def test_first_round_is_the_enumeration_on_unmodified_regions(host, params, work):
    wl, arrs, patcher, _ = work
    regs, start, lens = arrs
    want = []
    for ri, mine in enumerate(wl["regs"]):
        a = sorted(mine, key=lambda r: r["re"]) if len(mine) > 1 else []
        want += [(ri,) + S.key12(a[j], a[i]) for j, i in S.first_round(a, patcher)]
    with host.SdpEngine(params, wl["l_pac"], regs, start, lens) as e:
        t = e.needs()
    got = [(int(x["read"]),) + tuple(int(x[nm][f]) for nm in ("a", "b") for f in S.PREG) for x in t]
    assert sorted(got) == sorted(want) and len(got) >= 100


def test_a_stale_result_is_never_used(host, params, work):
    """every task whose q or p a merge has rewritten by the time the loop reaches the pair gets a wrong answer (a merge with a
    huge score): none of them may show.  The stale pairs are the round-1 tasks of (q, p) in their first states where the
    restatement reached the pair in another state, or never."""
    wl, arrs, patcher, (want, want_start, cnt, _) = work
    reached = patcher.reached
    fed_wrong = []

    def wrong(read, a, b):
        stale = (read,) + S.key12(a, b) not in reached
        if stale:
            fed_wrong.append(read)
        return stale
    memo = dict(patcher.memo)
    try:
        out, start, st, _ = run_engine(host, patcher, params, wl, arrs, on_round=lambda k, t: answer(host, patcher, t, wrong))
    finally:
        patcher.memo.clear()
        patcher.memo.update(memo)
    assert len(fed_wrong) >= 20
    assert S.same_regions(out, want) is None and list(start) == want_start


def test_the_smallest_staleness_the_loop_can_make(host, params):
    """X, Q, P in a row.  X merges into Q with a score and a band equal to Q's own, so Q changes in rb and qb ONLY (a merge always
    moves both: the pre-tests want a.qb < b.qb and the loop q.rb < p.rb).  The result held for (Q, P) is a wrong merge: the engine
    must ask for (Q', P) instead of using it."""
    x = S.region(1000, 1050, 0, 50, 3, 0, 0, 3)                 # (so low a score that Q's own passes the 0.90 ratio of the join)
    q = S.region(1052, 1110, 50, 108, 45, 0, 0, 4)
    p = S.region(1112, 1170, 108, 166, 50, 0, 0, 5)
    regs, start, lens = one_read(host, [x, q, p])
    q2 = dict(q, rb=x["rb"], qb=x["qb"])
    with host.SdpEngine(params, 200003, regs, start, lens) as e:
        t = e.needs()
        keys = [tuple(int(r[n_][k]) for n_ in ("a", "b") for k in S.PREG) for r in t]
        assert sorted(keys) == sorted([S.key12(x, q), S.key12(q, p), S.key12(x, p)])
        res = np.zeros(len(t), dtype=host.PRESULT)
        for k, key in enumerate(keys):
            res[k] = (q["score"], q["w"], q["score"], 0) if key == S.key12(x, q) else (777, 9, 777, 0)
        e.feed(res)
        t = e.needs()
        assert [tuple(int(r[n_][k]) for n_ in ("a", "b") for k in S.PREG) for r in t] == [S.key12(q2, p)]
        e.feed(np.array([(0, 6, 20, 2)], dtype=host.PRESULT))
        assert len(e.needs()) == 0
        out, _, st = e.collect()
    assert st["merges"] == 1 and st["rounds"] == 2 and st["alns_bwa"] == 2 and 777 not in list(out["score"])
    assert sorted(int(v) for v in out["src"]) == [1, 2] and int(out[out["src"] == 1]["n_comp"][0]) == 3


def test_presorted(host, params, work):
    wl, arrs, patcher, (want, want_start, _, _) = work
    regs, start, lens = arrs
    srt = regs.copy()
    for r in range(len(lens)):
        lo, hi = int(start[r]), int(start[r + 1])
        srt[lo:hi] = regs[lo:hi][np.argsort(regs[lo:hi]["re"], kind="stable")]
    out, ostart, _, _ = run_engine(host, patcher, params, wl, (srt, start, lens), opt=dict(presorted=1))
    # the same regions; src names the caller's array, which is another now
    for f in S.FIELDS[:-1]:
        assert np.array_equal(out[f], np.array([w[f] for w in want], dtype=out.dtype[f])), f
    assert all(tuple(srt[int(o["src"])][k] for k in ("re", "rid", "read")) == (o["re"], o["rid"], o["read"]) for o in out)
    # among equal re the caller's order holds: the other order of an equal-re pair gives the other survivor
    ties = [r for r in range(len(lens)) if start[r + 1] - start[r] == 2 and srt[int(start[r])]["re"] == srt[int(start[r]) + 1]["re"]]
    assert ties
    flip = srt.copy()
    for r in ties:
        lo = int(start[r])
        flip[lo], flip[lo + 1] = srt[lo + 1].copy(), srt[lo].copy()
    out2, _, _, _ = run_engine(host, patcher, params, wl, (flip, start, lens), opt=dict(presorted=1))
    for r in ties:
        lo = int(start[r])
        a, b = out[out["read"] == r], out2[out2["read"] == r]
        assert len(a) == len(b) == 1 and tuple(a[0])[:4] == tuple(srt[lo + 1])[:4] and tuple(b[0])[:4] == tuple(flip[lo + 1])[:4]
    bad = next(r for r in range(len(lens)) if start[r + 1] - start[r] >= 2 and regs[int(start[r])]["re"] != regs[int(start[r]) + 1]["re"])
    lo = int(start[bad])
    down = srt.copy()
    down[lo], down[lo + 1] = srt[lo + 1].copy(), srt[lo].copy()
    with pytest.raises(host.BswError) as ei:
        host.SdpEngine(params, wl["l_pac"], down, start, lens, opt=dict(presorted=1))
    assert ei.value.code == INVAL and "region %d" % (lo + 1) in str(ei.value) and "presorted" in str(ei.value)
    host.SdpEngine(params, wl["l_pac"], down, start, lens).close()      # without the option the order is the engine's business


def test_patch_0_needs_nothing(host, params, work):
    wl, arrs, patcher, _ = work
    calls = patcher.calls
    want, want_start, cnt, rounds = S.sdp(wl, patcher, patch=False)
    out, start, st, per_round = run_engine(host, patcher, params, wl, arrs, opt=dict(patch=0))
    assert per_round == [] and patcher.calls == calls and max(rounds) == 0
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert list(start) == want_start and st["merges"] == 0 and st["tasks"] == 0 and st["rounds"] == 0 and st["alns_bwa"] == 0
    assert S.same_stats(st, cnt, len(wl["reads"]), len(arrs[0]), len(want)) is None
    assert (out["sub"] != 0).sum() >= 100 and (out["csub"] != 0).sum() >= 100
    assert cnt["kills_p"] >= 5 and cnt["kills_q"] >= 5 and cnt["dups"] >= 3


def test_max_chain_gap_100_and_a_pair_only_a_merge_brings_in_reach(host, params, work):
    wl, arrs, patcher, _ = work
    want, want_start, cnt, rounds = S.sdp(wl, patcher, gap=100)
    assert cnt["reach_after_merge"] >= 3 and cnt["merges"] >= 20, cnt
    out, start, st, per_round = run_engine(host, patcher, params, wl, arrs, opt=dict(max_chain_gap=100))
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert list(start) == want_start and len(per_round) == max(rounds)
    assert S.same_stats(st, cnt, len(wl["reads"]), len(arrs[0]), len(want)) is None


def test_another_mask_level_redun(host, params, work):
    wl, arrs, patcher, _ = work
    want, want_start, cnt, _ = S.sdp(wl, patcher, mlr=.5)
    out, start, st, _ = run_engine(host, patcher, params, wl, arrs, opt=dict(mask_level_redun=.5))
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert S.same_stats(st, cnt, len(wl["reads"]), len(arrs[0]), len(want)) is None


def test_reads_with_many_regions_either_side_of_the_sort_threshold(host, params):
    """the engine sorts up to 24 regions of a read by insertion and more with qsort: 23, 24, 25 and 60 regions with equal re,
    equal (score, rb, qb) and redundant neighbours among them, patch = 0 (the sorts, the kills and the duplicates alone)"""
    rng = np.random.default_rng(11)
    reads, regs = [], []
    for ri, n in enumerate((23, 24, 25, 60)):
        mine = []
        for _ in range(n):
            rb, ln, qb = 1000 + 7 * int(rng.integers(0, 40)), 40 + 5 * int(rng.integers(0, 4)), int(rng.integers(0, 3)) * 10
            mine.append(S.region(rb, rb + ln, qb, qb + ln, 30 + int(rng.integers(0, 3)), ri, int(rng.integers(0, 2)), 0, rng))
        reads.append(np.zeros(100, np.uint8))
        regs.append(mine)
    wl = dict(l_pac=200003, reads=reads, regs=regs)
    want, want_start, cnt, _ = S.sdp(wl, None, patch=False)
    assert cnt["equal_re"] >= 10 and cnt["dups"] >= 3 and cnt["kills_p"] >= 3 and cnt["kills_q"] >= 3, cnt
    out, start, st, _ = run_engine(host, None, params, wl, S.arrays(host, wl), opt=dict(patch=0))
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert list(start) == want_start and S.same_stats(st, cnt, 4, 132, len(want)) is None


def one_read(host, regs, l_read=200):
    wl = dict(reads=[np.zeros(l_read, np.uint8)], regs=[regs])
    return S.arrays(host, wl)


@pytest.mark.parametrize("change,text", [
    (dict(rb=1100, re=1100), "rb"), (dict(qb=-1), "qb"), (dict(qb=60, qe=60), "qe"), (dict(qe=201), "qe"), (dict(w=-1), "w"),
    (dict(score=0), "score"), (dict(score=-3), "score"), (dict(read=1), "read"),
])
def test_open_refuses(host, params, change, text):
    good = S.region(1000, 1060, 0, 60, 50, 0, 0, 3)
    regs, start, lens = one_read(host, [good, dict(good, **change)])
    with pytest.raises(host.BswError) as ei:
        host.SdpEngine(params, 200003, regs, start, lens)
    assert ei.value.code == INVAL and "region 1" in str(ei.value) and text in str(ei.value), str(ei.value)
    host.SdpEngine(params, 200003, regs[:1], np.array([0, 1], dtype=np.uint64), lens).close()


def test_open_refuses_a_bad_reg_start_and_null(host, params):
    good = S.region(1000, 1060, 0, 60, 50, 0, 0, 3)
    regs, start, lens = one_read(host, [good, good])
    for bad in ([1, 2], [0, 1], [0, 3]):
        with pytest.raises(host.BswError) as ei:
            host.SdpEngine(params, 200003, regs, np.array(bad, dtype=np.uint64), lens)
        assert ei.value.code == INVAL and "reg_start" in str(ei.value)
    two = np.array([10, 10], dtype=np.int32)
    with pytest.raises(host.BswError) as ei:
        host.SdpEngine(params, 200003, regs, np.array([0, 2, 1], dtype=np.uint64), two)
    assert ei.value.code == INVAL
    L = host.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(400)
    assert L.bsw_sdp_open(None, None, 200003, regs.ctypes.data, 2, start.ctypes.data, lens.ctypes.data, 1, C.byref(h), err, 400) == INVAL and err.value
    assert L.bsw_sdp_open(params.ctypes.data, None, 200003, regs.ctypes.data, 2, start.ctypes.data, lens.ctypes.data, 1, None, None, 0) == INVAL
    n, t = C.c_size_t(0), C.c_void_p()
    assert L.bsw_sdp_needs(None, C.byref(t), C.byref(n)) == INVAL and L.bsw_sdp_feed(None, None, 0) == INVAL
    assert L.bsw_sdp_collect(None, None, C.byref(n), None, None) == INVAL
    L.bsw_sdp_close(None)
    with host.SdpEngine(params, 200003, regs, start, lens) as e:
        with pytest.raises(host.BswError):                      # collect before the engine has finished
            e.collect()
        t = e.needs()
        with pytest.raises(host.BswError):                      # not the results of exactly those tasks
            e.feed(np.zeros(len(t) + 1, dtype=host.PRESULT))
    zero = np.zeros(1, dtype=np.uint64)
    with host.SdpEngine(params, 200003, regs[:0], zero, lens[:0]) as e:      # no read at all
        assert len(e.needs()) == 0
        out, ostart, st = e.collect()
        assert len(out) == 0 and list(ostart) == [0] and st["reads"] == 0


def test_from_cregs(host):
    c = np.zeros(5, dtype=host.CREG)
    rng = np.random.default_rng(3)
    for f in host.CREG.names:
        c[f] = rng.integers(1, 1000, 5)
    s = host.sdp_from_cregs(c)
    for f in ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "rid", "read"):
        assert np.array_equal(s[f], c[f]), f
    assert not s["sub"].any() and not s["csub"].any() and not s["n_comp"].any() and list(s["src"]) == [0, 1, 2, 3, 4]
    assert host.lib().bsw_sdp_from_cregs(None, 3, s.ctypes.data) == INVAL and host.lib().bsw_sdp_from_cregs(None, 0, None) == 0


NEW = ["bsw_sdp_default_opt", "bsw_sdp_from_cregs", "bsw_sdp_open", "bsw_sdp_needs", "bsw_sdp_feed", "bsw_sdp_collect", "bsw_sdp_close",
       "bsw_sdp_ref_start", "bsw_sdp_reads_start", "bsw_sdp_test", "bsw_sdp_finish", "bsw_sdp_job_stats"]


def test_struct_sizes_symbols_and_defaults(host, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwa_sw_mi355.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(bsw_sreg),sizeof(bsw_sdp_opt),sizeof(bsw_sdp_stats),offsetof(bsw_sreg,sub),offsetof(bsw_sreg,read),'
                   'offsetof(bsw_sdp_stats,alns_bwa),BSW_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [64, 16, 88, 40, 56, 80, 6]
    assert [host.SREG.itemsize, host.SDP_OPT.itemsize, host.SDP_STATS.itemsize, host.SREG.fields["sub"][1], host.SREG.fields["read"][1],
            host.SDP_STATS.fields["alns_bwa"][1]] == sizes[:6]
    L = C.CDLL(host.lib_path())
    for n in NEW:
        assert hasattr(L, n) and n in host.EXPORTS, n
    assert L.bsw_abi_version() == 6
    o = host.sdp_opt()[0]
    assert (float(o["mask_level_redun"]), int(o["max_chain_gap"]), int(o["patch"]), int(o["presorted"])) == (float(np.float32(.95)), 10000, 1, 0)
    text = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")].split("every other call")[0]
    for n in NEW[7:]:
        assert n in threads, n
    assert "mem_sort_dedup_patch" in text and "AS RECALLED" in text and "STABLE" in text


def test_the_regions_of_chain2aln_replay_through_the_engine(host, oracle, params):
    """bsw_chain2aln_replay's regions (the oracle's extension records of every seed) -> bsw_sdp_from_cregs -> the engine, against
    the restatement on the same regions"""
    import _rtl_ref
    wl = CR.make_workload(120, 99)
    ch, sd, lens = CR.arrays(host, wl)
    rdt, _ = host.chain2aln_plan(params, wl["l_pac"], ch, sd, lens)
    pen = CR.pen_of(params)
    items = [(int(t["read"]), int(t["seed"]["rbeg"]), int(t["seed"]["qbeg"]), int(t["seed"]["len"]), int(t["rmax0"]), int(t["rmax1"]), k)
             for k, t in enumerate(rdt)]
    tasks, keep = CR.build_tasks(host, pen, wl["reads"], wl["both"], items)
    res = CR.run_oracle(oracle, _rtl_ref, params, tasks)
    cregs, _, start = host.chain2aln_replay(params, ch, sd, lens, res)
    sregs = host.sdp_from_cregs(cregs)
    wl["regs"] = [[{f: int(sregs[k][f]) for f in S.FIELDS[:-1]} for k in range(int(start[r]), int(start[r + 1]))] for r in range(len(lens))]
    patcher = S.Patcher(host, oracle, params, wl)
    want, want_start, cnt, rounds = S.sdp(wl, patcher)
    out, ostart, st, per_round = run_engine(host, patcher, params, wl, (sregs, start, lens))
    assert S.same_regions(out, want) is None, S.same_regions(out, want)
    assert list(ostart) == want_start and len(per_round) == max(rounds)
    assert S.same_stats(st, cnt, len(lens), len(sregs), len(want)) is None
    assert st["regs_out"] < st["regs_in"] and st["kills_p"] + st["kills_q"] + st["merges"] >= 10, st
