"""mem_sam_pe's mate-rescue loop as a job around the rescue tickets on the GPU: bsw_rescue_ref_start and bsw_rescue_reads_start on
the workload of tests/_rescue_ref.py must hand back the regions, out_start, n_sw and counts of the sequential restatement, which
aligns a window on the CPU oracle only when bwa's loop reaches it.  The path under test is the host's (engine, rounds, submits);
the ksw_align2 kernels behind the rescue tickets are covered by tests/test_gpu_matesw_ref.py and tests/test_gpu_align_long.py."""
import os
import subprocess
import sys
import time

import pytest

import _rescue_ref as R
import _sdp_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params(host):
    return host.default_params()


@pytest.fixture(scope="module")
def work(host, oracle, params):
    """the workload and the restatement's answers: computed once, left unchanged"""
    wl = R.make_workload()
    al = R.Aligner(oracle, params, wl)
    return wl, S.arrays(host, wl), {name: R.rescue(wl, al, name) for name in ("fr", "two", "nocontig")}


def check(got, want, n_in):
    out, start, n_sw, st = got
    wout, wstart, wn_sw, cnt = want
    assert S.same_regions(out, wout) is None, S.same_regions(out, wout)
    assert list(start) == wstart and list(n_sw) == wn_sw
    assert R.same_stats(st, cnt, n_in, len(wout)) is None, R.same_stats(st, cnt, n_in, len(wout))


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]


def start(c, params, ref, wl, regs, reg_start, name="fr", rd=None, reads=None):
    opt, contigs = R.options(name)
    return c.rescue_start(params, ref, regs, reg_start, rd=rd, reads=reads, contigs=contigs, opt=opt)


def forms_body(host, oracle):
    """run by the child process of the test below, under BSW_F4_MATESW_WORK: round 1 is cut into several chunks"""
    params = host.default_params()
    wl = R.make_workload()
    al = R.Aligner(oracle, params, wl)
    want = {name: R.rescue(wl, al, name) for name in ("fr", "two", "nocontig")}
    regs, reg_start, lens = S.arrays(host, wl)
    assert want["fr"][3]["rounds"] == 2 and want["fr"][3]["late"] >= 3 and want["fr"][3]["pushed"] >= 40
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            base = c.host_stats()["chunks"]
            got1 = start(c, params, ref, wl, regs, reg_start, reads=wl["reads"]).finish()
            grew = int(c.host_stats()["chunks"] - base)
            print("rescue: %d tasks in round 1, %d in all, %d chunks over %d rounds" % (got1[3]["tasks_first"], got1[3]["tasks"], grew, got1[3]["rounds"]))
            assert grew >= got1[3]["rounds"] + 2                            # round 1 alone is three chunks or more
            got2 = start(c, params, ref, wl, regs, reg_start, rd=rd).finish()
            assert c.inflight() == 0
            check(got1, want["fr"], len(regs))
            check(got2, want["fr"], len(regs))
            assert same_bytes(got1, got2)
            for name in ("two", "nocontig"):
                a = start(c, params, ref, wl, regs, reg_start, name, rd=rd).finish()
                b = start(c, params, ref, wl, regs, reg_start, name, reads=wl["reads"]).finish()
                check(a, want[name], len(regs))
                assert same_bytes(a, b), name
        finally:
            c.reads_free(rd)
            c.ref_free(ref)
    print("forms ok")


def test_both_forms_equal_the_restatement_with_round_1_in_several_chunks():
    """BSW_F4_MATESW_WORK is read once per process, so this runs in a child"""
    env = dict(os.environ, BSW_F4_MATESW_WORK="2000000")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "forms ok" in r.stdout
    print(r.stdout[-400:])


def test_a_job_driven_by_polls_alone(host, params, work):
    wl, (regs, reg_start, lens), want = work
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            job = start(c, params, ref, wl, regs, reg_start, rd=rd)
            assert c.inflight() == 1 and job.stats()["rounds"] == 1 and job.stats()["tasks"] == want["fr"][3]["tasks_first"]
            assert job.out_capacity() == len(regs) + 4 * want["fr"][3]["anchors"]
            polls, longest, deadline = 0, 0.0, time.monotonic() + 60
            while True:
                t0 = time.monotonic()
                done = job.test()
                longest = max(longest, time.monotonic() - t0)
                polls += 1
                if done or time.monotonic() > deadline:
                    break
            assert done and c.inflight() == 0 and job.test()              # every round's ticket was collected by the polls
            assert job.stats()["rounds"] == 2 and longest < 0.5
            print("polls: %d, the longest took %.1f us" % (polls, longest * 1e6))
            check(job.finish(), want["fr"], len(regs))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_mates_of_1100_bases_need_set_align_long(host, oracle, params):
    """four pairs whose long reads have 1 100 bases: the rescue submit's own limit refuses the job until bsw_set_align_long(1), then
    the windows run on the LDS-row kernel"""
    wl = R.make_workload(n100=0, n_long=4, long_len=1100)
    want = R.rescue(wl, R.Aligner(oracle, params, wl))
    regs, reg_start, lens = S.arrays(host, wl)
    assert list(lens).count(1100) == 8 and want[3]["word_tasks"] >= 3 and sum(1 for m in want[0] if m["src"] >= R.NEW and m["score"] > 1000) >= 2
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            with pytest.raises(host.BswError) as ei:
                start(c, params, ref, wl, regs, reg_start, rd=rd)
            assert ei.value.code == -3 and c.inflight() == 0
            host.set_align_long(1)
            got = start(c, params, ref, wl, regs, reg_start, rd=rd).finish()
            got2 = start(c, params, ref, wl, regs, reg_start, reads=wl["reads"]).finish()
            check(got, want, len(regs))
            assert same_bytes(got, got2)
        finally:
            host.set_align_long(0)
            c.reads_free(rd)
            c.ref_free(ref)


def test_two_jobs_side_by_side_with_an_sdp_job(host, oracle, params, work):
    wl, (regs, reg_start, lens), want = work
    swl = S.make_workload(n_reads=68)
    swant = S.sdp(swl, S.Patcher(host, oracle, params, swl))
    sregs, sstart, _ = S.arrays(host, swl)
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        sref = c.ref_upload(swl["pac"], swl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            j1 = start(c, params, ref, wl, regs, reg_start, rd=rd)
            js = c.sdp_start(params, sref, sregs, sstart, reads=swl["reads"])
            j2 = start(c, params, ref, wl, regs, reg_start, "two", reads=wl["reads"])
            assert c.inflight() == 3
            g2 = j2.finish()
            sout, sst, sstat = js.finish()
            g1 = j1.finish()
            assert c.inflight() == 0
            check(g1, want["fr"], len(regs))
            check(g2, want["two"], len(regs))
            assert S.same_regions(sout, swant[0]) is None and list(sst) == swant[1]
        finally:
            c.reads_free(rd)
            c.ref_free(sref)
            c.ref_free(ref)


def test_the_chained_block(host, oracle, params):
    """bsw_sdp_reads_start -> finish -> bsw_rescue_reads_start -> finish on the sdp test workload, its reads 2k and 2k + 1 taken as
    mates, against the two restatements.  That workload's decoy regions carry rids of no contig, so there is no contig table, and
    one of its reads has 1 040 bases, so bsw_set_align_long(1)."""
    wl = S.make_workload()
    sout, sstart, _, _ = S.sdp(wl, S.Patcher(host, oracle, params, wl))
    mid = dict(wl, regs=[[{f: g[f] for f in S.FIELDS[:-1]} for g in sout[sstart[r]:sstart[r + 1]]] for r in range(len(wl["reads"]))])
    config = (dict(low=[0, 50, 0, 0], high=[0, 1500, 0, 0], failed=[1, 0, 1, 1]), False)
    want = R.rescue(mid, R.Aligner(oracle, params, mid), config)
    opt, _ = R.options(config)
    assert want[3]["tasks"] >= 100 and want[3]["alns"] >= 100 and max(len(r) for r in wl["reads"]) > 1024
    regs, reg_start, lens = S.arrays(host, wl)
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            host.set_align_long(1)
            sregs, start2, _ = c.sdp_start(params, ref, regs, reg_start, rd=rd).finish()
            got = c.rescue_start(params, ref, sregs, start2, rd=rd, opt=opt).finish()
            assert c.inflight() == 0
            check(got, want, len(sregs))
        finally:
            host.set_align_long(0)
            c.reads_free(rd)
            c.ref_free(ref)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft
    forms_body(graft.load_package().host, graft.load_oracle())
