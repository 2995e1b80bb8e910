"""bsw_rescue_* without a GPU: the engine of bsw_rescue.c driven through host.py's RescueEngine, with tests/_matesw_ref.py::matesw
standing in for the GPU in the needs / feed loop, against the sequential restatement in tests/_rescue_ref.py: every field of every
region, out_start, n_sw and the counts; what the workload must contain is asserted on the restatement first.  Then round 1, the late
case and what a host that stops after round 1 returns instead, no (anchor, r) asked twice, no contig table, the configurations
that ask for nothing, every refusal of open, the struct sizes, the symbols and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _rescue_ref as R
import _sdp_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, LIMIT = -2, -3


@pytest.fixture(scope="module")
def params(host):
    return host.default_params()


@pytest.fixture(scope="module")
def work(host, oracle, params):
    """the workload, its arrays, the oracle behind the windows and the restatement's answer per configuration: computed once"""
    wl = R.make_workload()
    aligner = R.Aligner(oracle, params, wl)
    want = {name: R.rescue(wl, aligner, name) for name in R.CONFIGS}
    return wl, S.arrays(host, wl), aligner, want


def run_engine(host, aligner, params, wl, arrs, name="fr", opt=None, rounds=None):
    """-> (regions, out_start, n_sw, stats, tasks per round); rounds: stop feeding real results after that many (the rest: status 1)"""
    regs, start, lens = arrs
    o, contigs = R.options(name)
    o.update(opt or {})
    per_round = []
    with host.RescueEngine(params, wl["l_pac"], regs, start, lens, contigs=contigs, opt=o) as e:
        while True:
            t = e.needs()
            if not len(t):
                break
            per_round.append(t)
            e.feed(R.answer(host, aligner, t))
        return e.collect() + (per_round,)


def keys(tasks):
    return [tuple(int(t[f]) for f in ("read", "is_rev", "rb", "re", "xtra", "min_score")) for t in tasks]


def test_the_workload_holds_every_case(work):
    wl, _, _, want = work
    n = [len(r) for r in wl["reads"]]
    assert 90 <= n.count(100) // 2 <= 110 and n.count(250) == 16 and len(wl["contigs"]) == 3 and 55000 <= wl["l_pac"] <= 65000
    out, start, n_sw, c = want["fr"]
    assert c["proper_dirs"] >= 10, c                            # the mate is proper already: no task
    assert c["into_empty"] >= 20, c                             # a mate without a region, rescued
    assert c["unused"] >= 5, c                                  # sent in round 1, made needless by an earlier anchor's rescue
    assert c["rounds"] == 2 and c["late"] >= 3 and sorted(set(c["late_pairs"]))[0] == wl["hand"]["late"], c
    assert c["pen_cut"] >= 5 and c["max_cut"] == 0, c
    assert c["clamped"] >= 2 and c["other_contig"] >= 1 and c["short"] >= 1 and c["status1"] == 0, c
    assert c["status2"] >= 10 and c["equal_existing"] >= 1 and c["rev_anchor_push"] >= 10 and c["shrank"] >= 4, c
    assert c["byte_tasks"] >= 60 and c["word_tasks"] >= 6, c    # 100 bases: KSW_XBYTE; 250: the 16-bit path
    assert n_sw[wl["hand"]["other_contig"]] == 0 and n_sw[wl["hand"]["short"]] == 0 and n_sw[wl["hand"]["clamp"]] == 1
    assert n_sw[wl["hand"]["equal"]] == 2 and start[2 * wl["hand"]["equal"] + 2] - start[2 * wl["hand"]["equal"] + 1] == 1
    late = wl["hand"]["late"]
    mate = out[start[2 * late + 1]:start[2 * late + 2]]
    assert n_sw[late] == 2 and [m["src"] >= R.NEW for m in mate] == [True, True] and all(m["score"] == 100 for m in mate)
    assert want["mm1"][3]["max_cut"] >= 10 and want["mm1"][2][wl["hand"]["many"]] == 1 and n_sw[wl["hand"]["many"]] == 1
    assert want["nocontig"][3]["status1"] >= 1 and want["nocontig"][2][wl["hand"]["bridge"]] == 0 and n_sw[wl["hand"]["bridge"]] == 1
    assert want["two"][3]["two_live_push"] >= 5 and want["two"][3]["pushed"] > c["pushed"] and c["two_live_push"] == 0
    assert sum(1 for m in out if m["src"] >= R.NEW) >= 40


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_engine_equals_the_restatement(host, params, work, name):
    wl, arrs, aligner, want = work
    wout, wstart, wn_sw, cnt = want[name]
    out, start, n_sw, st, per_round = run_engine(host, aligner, params, wl, arrs, name)
    assert S.same_regions(out, wout) is None, S.same_regions(out, wout)
    assert list(start) == wstart and list(n_sw) == wn_sw
    assert R.same_stats(st, cnt, len(arrs[0]), len(wout)) is None, R.same_stats(st, cnt, len(arrs[0]), len(wout))
    assert len(per_round) == cnt["rounds"] and sum(len(t) for t in per_round) == cnt["tasks"]
    assert sum(int(v) for v in n_sw) == st["alns_bwa"]


def test_round_1_is_the_enumeration_on_the_initial_regions(host, params, work):
    wl, (regs, start, lens), _, _ = work
    for name in R.CONFIGS:
        opt, contigs = R.options(name)
        src_regs, at = [], 0
        for mine in wl["regs"]:
            src_regs.append([dict(g, src=at + k) for k, g in enumerate(mine)])
            at += len(mine)
        want = R.first_round(wl, opt, contigs, src_regs)
        with host.RescueEngine(params, wl["l_pac"], regs, start, lens, contigs=contigs, opt=opt) as e:
            got = keys(e.needs())
            assert e.out_capacity() == len(regs) + 4 * sum(len(R.anchors_of(r, opt)) for r in src_regs if r)
        assert sorted(got) == sorted(want.values()) and len(got) == len(set(got)) >= 80, name


def test_the_late_case_needs_one_more_round_and_the_old_recipe_drops_an_alignment(host, params, work):
    """the pair built by hand alone: round 1 holds no task of the second anchor; the engine asks for it in round 2.  A host that
    follows the old recipe (one round, the orientation passed over) returns another ma: that recipe was wrong."""
    wl, _, aligner, _ = work
    k = wl["hand"]["late"]
    one = dict(wl, reads=wl["reads"][2 * k:2 * k + 2], regs=[[dict(g, read=i) for g in r] for i, r in enumerate(wl["regs"][2 * k:2 * k + 2])])
    al = R.Aligner(aligner.oracle, params, one)
    wout, wstart, wn_sw, cnt = R.rescue(one, al)
    assert cnt["rounds"] == 2 and cnt["late"] == 1 and cnt["tasks_first"] == 1 and wn_sw == [2]
    out, start, n_sw, st, per_round = run_engine(host, al, params, one, S.arrays(host, one))
    assert [len(t) for t in per_round] == [1, 1] and st["rounds"] == 2 and st["late"] == 1
    a1, a2 = one["regs"][0]
    assert per_round[0][0]["rb"] == a1["rb"] and per_round[1][0]["rb"] == a2["rb"]          # (FR: the window starts at the anchor)
    assert S.same_regions(out, wout) is None and list(n_sw) == [2]
    old, old_start, old_n_sw, _ = R.rescue(one, al, stop_after_round_1=True)
    assert old_n_sw == [1] and len(old) == len(wout) - 1
    assert [m["src"] for m in wout[wstart[1]:]] == [R.NEW | 0, R.NEW | 1] and [m["src"] for m in old[old_start[1]:]] == [R.NEW | 0]


def test_no_anchor_orientation_is_asked_twice(host, params, work):
    wl, arrs, aligner, want = work
    for name in R.CONFIGS:
        _, _, _, st, per_round = run_engine(host, aligner, params, wl, arrs, name)
        asked = [k for t in per_round for k in keys(t)]
        # (read, is_rev, rb, re) names (anchor, r) up to anchors of one read with equal rb, which the workload does not have
        assert len(asked) == len(set(asked)) == st["tasks"] <= 4 * st["anchors"], name


def test_without_a_contig_table_only_the_ticket_keeps_a_window_from_running(host, params, work):
    wl, arrs, aligner, want = work
    out, start, n_sw, st, per_round = run_engine(host, aligner, params, wl, arrs, "nocontig")
    k = wl["hand"]["bridge"]
    bridging = [t for t in per_round[0] if t["rb"] < wl["l_pac"] < t["re"]]
    assert bridging and all(R.answer(host, aligner, np.array([t]))[0]["status"] == 1 for t in bridging) and n_sw[k] == 0
    assert start[2 * k + 2] == start[2 * k + 1]                 # nothing rescued there
    k = wl["hand"]["other_contig"]
    assert n_sw[k] == 1                                         # (and the window in another contig runs)


def test_configurations_that_ask_for_nothing_return_the_input(host, params, work):
    wl, arrs, aligner, _ = work
    regs, start, lens = arrs
    for opt in (dict(R.FR, max_matesw=0), dict(), dict(R.FR, failed=[1, 1, 1, 1])):
        calls = aligner.calls
        with host.RescueEngine(params, wl["l_pac"], regs, start, lens, contigs=R.CONTIGS, opt=opt) as e:
            assert len(e.needs()) == 0
            out, ostart, n_sw, st = e.collect()
        assert aligner.calls == calls and not n_sw.any() and list(ostart) == list(start)
        for f in S.FIELDS[:-1]:
            assert np.array_equal(out[f], regs[f]), f
        assert list(out["src"]) == list(range(len(regs)))
        assert st["rounds"] == st["tasks"] == st["alns_bwa"] == st["pushed"] == 0 and st["regs_out"] == st["regs_in"] == len(regs)
        assert st["anchors"] == (0 if opt.get("max_matesw") == 0 else st["anchors"]) and st["pairs"] == len(lens) // 2
    o = host.rescue_opt()[0]
    assert list(o["failed"]) == [1, 1, 1, 1] and (int(o["pen_unpaired"]), int(o["max_matesw"]), int(o["min_seed_len"]), int(o["a"])) == (17, 50, 19, 1)
    assert (float(o["mask_level_redun"]), int(o["max_chain_gap"])) == (float(np.float32(.95)), 10000)


def two_reads(host, a_regs, m_regs=()):
    wl = dict(reads=[np.zeros(100, np.uint8), np.zeros(100, np.uint8)], regs=[list(a_regs), list(m_regs)])
    return S.arrays(host, wl)


GOOD = dict(rb=1000, re=1060, qb=0, qe=60, score=50, truesc=50, w=3, seedcov=30, sub=0, csub=0, rid=0, n_comp=0, read=0)


@pytest.mark.parametrize("change,text", [
    (dict(rb=1100, re=1100), "rb"), (dict(qb=-1), "qb"), (dict(qb=60, qe=60), "qe"), (dict(qe=101), "qe"), (dict(w=-1), "w"),
    (dict(score=0), "score"), (dict(read=1), "read"), (dict(rid=3), "rid 3 outside the 3 contigs"), (dict(rid=-1), "rid"),
])
def test_open_refuses_a_region(host, params, change, text):
    regs, start, lens = two_reads(host, [GOOD, dict(GOOD, **change)])
    with pytest.raises(host.BswError) as ei:
        host.RescueEngine(params, R.L_PAC, regs, start, lens, contigs=R.CONTIGS, opt=R.FR)
    assert ei.value.code == INVAL and "region 1" in str(ei.value) and text in str(ei.value), str(ei.value)
    host.RescueEngine(params, R.L_PAC, regs[:1], np.array([0, 1, 1], dtype=np.uint64), lens, contigs=R.CONTIGS, opt=R.FR).close()


@pytest.mark.parametrize("opt,contigs,text", [
    (dict(R.FR, low=[0, 600, 0, 0]), R.CONTIGS, "orientation 1: low 600 above high 500"),
    (dict(R.FR, pen_unpaired=-1), R.CONTIGS, "pen_unpaired -1"), (dict(R.FR, max_matesw=-2), R.CONTIGS, "max_matesw -2"),
    (dict(R.FR, min_seed_len=-3), R.CONTIGS, "min_seed_len -3"), (dict(R.FR, a=0), R.CONTIGS, "a 0 below 1"),
    (dict(R.FR, min_seed_len=40000, a=2), R.CONTIGS, "beyond 65535"), (dict(R.FR, max_chain_gap=-1), R.CONTIGS, "max_chain_gap"),
    (R.FR, ((0, 20000), (20000, 21001)), "the contigs end at 41001"), (R.FR, ((0, 20000), (20001, 40000)), "contig 1: offset 20001"),
    (R.FR, ((20000, 40001), (0, 20000)), "contig 0: offset 20000"), (R.FR, ((0, 0), (0, 60001)), "contig 0: offset 0, len 0"),
])
def test_open_refuses_options_and_contigs(host, params, opt, contigs, text):
    regs, start, lens = two_reads(host, [GOOD])
    with pytest.raises(host.BswError) as ei:
        host.RescueEngine(params, R.L_PAC, regs, start, lens, contigs=contigs, opt=opt)
    assert ei.value.code == INVAL and text in str(ei.value), str(ei.value)


def test_open_refuses_the_rest_and_the_calls_on_nothing(host, params):
    regs, start, lens = two_reads(host, [GOOD, GOOD])
    # a low above high of an orientation that has failed is nobody's business
    host.RescueEngine(params, R.L_PAC, regs, start, lens, contigs=R.CONTIGS, opt=dict(R.FR, low=[9, 100, 0, 0])).close()
    with pytest.raises(host.BswError) as ei:                    # an odd number of reads
        host.RescueEngine(params, R.L_PAC, regs, start[:2], lens[:1], opt=R.FR)
    assert ei.value.code == INVAL and "odd" in str(ei.value)
    for bad in ([1, 2, 2], [0, 1, 1], [0, 3, 3], [0, 2, 1]):
        with pytest.raises(host.BswError) as ei:
            host.RescueEngine(params, R.L_PAC, regs, np.array(bad, dtype=np.uint64), lens, opt=R.FR)
        assert ei.value.code == INVAL and "reg_start" in str(ei.value)
    L = host.lib()
    h, err = C.c_void_p(), C.create_string_buffer(400)
    o = host.rescue_opt(**R.FR)
    assert L.bsw_rescue_open(None, o.ctypes.data, R.L_PAC, None, 0, regs.ctypes.data, 2, start.ctypes.data, lens.ctypes.data, 2, C.byref(h), err, 400) == INVAL and err.value
    assert L.bsw_rescue_open(params.ctypes.data, o.ctypes.data, R.L_PAC, None, 3, regs.ctypes.data, 2, start.ctypes.data, lens.ctypes.data, 2, C.byref(h), err, 400) == INVAL
    assert L.bsw_rescue_open(params.ctypes.data, o.ctypes.data, R.L_PAC, None, 0, regs.ctypes.data, 2, start.ctypes.data, lens.ctypes.data, 2, None, None, 0) == INVAL
    assert L.bsw_rescue_open(params.ctypes.data, o.ctypes.data, R.L_PAC, None, 0, regs.ctypes.data, 1 << 31, start.ctypes.data, lens.ctypes.data, 2, C.byref(h), err, 400) == LIMIT
    assert b"2^31 - 1" in err.value
    n, t = C.c_size_t(0), C.c_void_p()
    assert L.bsw_rescue_needs(None, C.byref(t), C.byref(n)) == INVAL and L.bsw_rescue_feed(None, None, 0) == INVAL
    assert L.bsw_rescue_collect(None, None, C.byref(n), None, None, None) == INVAL and L.bsw_rescue_out_capacity(None) == 0
    assert L.bsw_rescue_job_out_capacity(None) == 0 and L.bsw_rescue_test(None) == INVAL and L.bsw_rescue_job_stats(None, None) == INVAL
    assert L.bsw_rescue_finish(None, None, 0, C.byref(n), None, None, None) == INVAL
    L.bsw_rescue_close(None)
    with host.RescueEngine(params, R.L_PAC, regs, start, lens, contigs=R.CONTIGS, opt=R.FR) as e:
        with pytest.raises(host.BswError):                      # collect before the engine has finished
            e.collect()
        t = e.needs()
        assert len(t) == 2 and keys(e.needs()) == keys(t)       # asked again before the feed: the same tasks
        with pytest.raises(host.BswError):                      # not the results of exactly those tasks
            e.feed(np.zeros(len(t) + 1, dtype=host.MRESULT))
    zero = np.zeros(1, dtype=np.uint64)
    with host.RescueEngine(params, R.L_PAC, regs[:0], zero, lens[:0], opt=R.FR) as e:      # no read at all
        assert len(e.needs()) == 0
        out, ostart, n_sw, st = e.collect()
        assert len(out) == 0 and list(ostart) == [0] and st["pairs"] == 0 and len(n_sw) == 0


NEW = ["bsw_rescue_default_opt", "bsw_rescue_open", "bsw_rescue_needs", "bsw_rescue_feed", "bsw_rescue_collect", "bsw_rescue_out_capacity",
       "bsw_rescue_close", "bsw_rescue_ref_start", "bsw_rescue_reads_start", "bsw_rescue_test", "bsw_rescue_finish", "bsw_rescue_job_stats",
       "bsw_rescue_job_out_capacity"]


def test_struct_sizes_symbols_header_and_abi(host, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bwa_sw_mi355.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %u\\n",'
                   'sizeof(bsw_contig),sizeof(bsw_rescue_opt),sizeof(bsw_rescue_stats),offsetof(bsw_rescue_opt,pen_unpaired),'
                   'offsetof(bsw_rescue_opt,mask_level_redun),offsetof(bsw_rescue_stats,late),BSW_ABI_VERSION,BSW_RESCUE_NEW>>31);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [16, 72, 80, 48, 64, 72, 6, 1]
    assert [host.CONTIG.itemsize, host.RESCUE_OPT.itemsize, host.RESCUE_STATS.itemsize, host.RESCUE_OPT.fields["pen_unpaired"][1],
            host.RESCUE_OPT.fields["mask_level_redun"][1], host.RESCUE_STATS.fields["late"][1]] == sizes[:6]
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", host.lib_path()], text=True)
    exported = sorted(ln.split()[-1] for ln in dyn.splitlines() if " T " in ln and "bsw_rescue" in ln)
    assert exported == sorted(NEW)                              # the internal entries (bsw_rescue_peek, bsw_sdp_pass0) are not exported
    assert "bsw_sdp_pass0" not in dyn
    L = C.CDLL(host.lib_path())
    for n in NEW:
        assert hasattr(L, n) and n in host.EXPORTS, n
    assert L.bsw_abi_version() == 6 and host.RESCUE_NEW == 0x80000000
    text = open(os.path.join(ROOT, "include", "bwa_sw_mi355.h")).read()
    threads = text[text.index(" * THREADS."):text.index("#define BSW_MAX_INFLIGHT")].split("every other call")[0]
    for n in NEW[7:]:
        assert n in threads, n
    assert "mem_sam_pe" in text and "bsw_rescue_open" in text and text.count("AS RECALLED") >= 3
