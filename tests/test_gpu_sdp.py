"""mem_sort_dedup_patch as a job around the patch tickets on the GPU: bsw_sdp_ref_start and bsw_sdp_reads_start on the workload of
tests/_sdp_ref.py must hand back the regions, out_start and counts of the sequential restatement, which aligns a pair on the CPU
oracle only when bwa's loop reaches it.  The path under test is the host's (engine, rounds, submits); the global-alignment
kernels behind the patch tickets are covered by tests/test_gpu_patch.py, so there are no long-query shapes here."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _chain2aln_ref as CR
import _rtl_ref
import _sdp_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params(host):
    return host.default_params()


@pytest.fixture(scope="module")
def work(host, oracle, params):
    """the workload and the restatement's answer: computed once, left unchanged"""
    wl = S.make_workload()
    want = S.sdp(wl, S.Patcher(host, oracle, params, wl))
    return wl, S.arrays(host, wl), want


def check(got, want, wl, n_in):
    out, start, st = got
    wout, wstart, cnt, rounds = want
    assert S.same_regions(out, wout) is None, S.same_regions(out, wout)
    assert list(start) == wstart
    assert S.same_stats(st, cnt, len(wl["reads"]), n_in, len(wout)) is None, S.same_stats(st, cnt, len(wl["reads"]), n_in, len(wout))


def forms_body(host, oracle):
    """run by the child process of the test below, under BSW_F4_PATCH_WORK: round 1 is cut into several chunks"""
    params = host.default_params()
    wl = S.make_workload()
    want = S.sdp(wl, S.Patcher(host, oracle, params, wl))
    regs, start, lens = S.arrays(host, wl)
    assert want[2]["merges"] >= 20 and want[2]["rounds"] == 3
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            base = c.host_stats()["chunks"]
            got1 = c.sdp_start(params, ref, regs, start, reads=wl["reads"]).finish()
            grew = int(c.host_stats()["chunks"] - base)
            print("sdp: %d tasks in round 1, %d in all, %d chunks over %d rounds" % (got1[2]["tasks_first"], got1[2]["tasks"], grew, got1[2]["rounds"]))
            assert grew >= got1[2]["rounds"] + 2                            # round 1 alone is three chunks or more
            j2 = c.sdp_start(params, ref, regs, start, rd=rd)
            j1 = c.sdp_start(params, ref, regs, start, reads=wl["reads"])   # two jobs side by side
            got2 = j2.finish()
            got1b = j1.finish()
            assert c.inflight() == 0
            check(got1, want, wl, len(regs))
            check(got2, want, wl, len(regs))
            for a, b in ((got1, got2), (got1, got1b)):
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        finally:
            c.reads_free(rd)
            c.ref_free(ref)
    print("forms ok")


def test_both_forms_equal_the_restatement_with_round_1_in_several_chunks():
    """BSW_F4_PATCH_WORK is read once per process, so this runs in a child"""
    env = dict(os.environ, BSW_F4_PATCH_WORK="300000")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "forms ok" in r.stdout
    print(r.stdout[-400:])


def test_a_job_driven_by_polls_alone(host, params, work):
    wl, (regs, start, lens), want = work
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            job = c.sdp_start(params, ref, regs, start, rd=rd)
            assert c.inflight() == 1 and job.stats()["rounds"] == 1 and job.stats()["tasks"] == want[2]["tasks_first"]
            polls, longest, deadline = 0, 0.0, time.monotonic() + 60
            while True:
                t0 = time.monotonic()
                done = job.test()
                longest = max(longest, time.monotonic() - t0)
                polls += 1
                if done or time.monotonic() > deadline:
                    break
            assert done and c.inflight() == 0 and job.test()              # every round's ticket was collected by the polls
            assert job.stats()["rounds"] == 3 and longest < 0.5
            print("polls: %d, the longest took %.1f us" % (polls, longest * 1e6))
            got = job.finish()
            assert got[2]["rounds"] == 3
            check(got, want, wl, len(regs))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_a_start_beside_four_tickets_is_busy_and_leaves_no_job(host, params, work):
    wl, (regs, start, lens), want = work
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            jobs = [c.sdp_start(params, ref, regs, start, rd=rd) for _ in range(4)]
            assert c.inflight() == 4
            with pytest.raises(host.BswError) as ei:
                c.sdp_start(params, ref, regs, start, rd=rd)
            assert ei.value.code == -6 and c.inflight() == 4 and "BSW_MAX_INFLIGHT" in str(ei.value)
            # a job with nothing to submit starts all the same: it needs no place
            j0 = c.sdp_start(params, ref, regs, start, rd=rd, opt=dict(patch=0))
            assert j0.test() and c.inflight() == 4
            j0.finish()
            # four jobs share the four places; on one thread a follow-up round always finds the place its own ticket has just left
            for j in jobs:
                check(j.finish(), want, wl, len(regs))
            assert c.inflight() == 0
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_patch_0_completes_without_a_ticket(host, oracle, params, work):
    wl, (regs, start, lens), _ = work
    want = S.sdp(wl, S.Patcher(host, oracle, params, wl), patch=False)
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            st0 = c.host_stats()
            job = c.sdp_start(params, ref, regs, start, rd=rd, opt=dict(patch=0))
            assert c.inflight() == 0 and job.test()
            got = job.finish()
            st1 = c.host_stats()
            assert c.inflight() == 0
            for k in ("h2d_bytes", "d2h_bytes", "submits", "chunks"):
                assert st1[k] == st0[k], k
            check(got, want, wl, len(regs))
            assert got[2]["tasks"] == 0 and (got[0]["sub"] != 0).sum() >= 100
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_the_chained_block(host, oracle, params):
    """bsw_chain2aln_reads_start -> finish -> bsw_sdp_from_cregs -> bsw_sdp_reads_start -> finish, against the two restatements"""
    wl = CR.make_workload(300, seed=5)
    ch, sd, lens = CR.arrays(host, wl)
    wregs, _, _ = CR.chain2aln(CR.Extender(host, oracle, _rtl_ref, params, wl), params, wl)
    per = [[] for _ in lens]
    for a in wregs:
        per[a["read"]].append(dict({f: a[f] for f in ("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov", "rid", "read")}, sub=0, csub=0, n_comp=0))
    wl["regs"] = per
    want = S.sdp(wl, S.Patcher(host, oracle, params, wl))
    assert want[2]["kills_p"] + want[2]["kills_q"] >= 10 and len(want[0]) < len(wregs)
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            cregs, _, start, _ = c.chain2aln_start(params, ref, ch, sd, rd=rd).finish()
            sregs = host.sdp_from_cregs(cregs)
            got = c.sdp_start(params, ref, sregs, start, rd=rd).finish()
            assert c.inflight() == 0
            check(got, want, wl, len(sregs))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft
    forms_body(graft.load_package().host, graft.load_oracle())
