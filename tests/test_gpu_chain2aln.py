"""mem_chain2aln as a job of the ticket pipeline on the GPU: bsw_chain2aln_ref_start and bsw_chain2aln_reads_start extend every seed
of the workload of tests/_chain2aln_ref.py and replay bwa's loop; regions, extended[] and the stats must equal the sequential
restatement, which extends a seed on the CPU oracle only when the loop reaches it.  The path under test is the host's (plan,
submit, replay); the kernels are covered elsewhere, so there are no long-query shapes here."""
import time

import numpy as np
import pytest

import _chain2aln_ref as R
import _matesw_ref as mr
import _rtl_ref

pytestmark = pytest.mark.gpu

INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def wl():
    return R.make_workload(300, seed=5)


@pytest.fixture(scope="module")
def arrays(host, wl):
    return R.arrays(host, wl)


@pytest.fixture(scope="module")
def reference(host, oracle, wl):
    out = {}
    for v in (0, 1, 2):
        p = host.default_params(variant=v)
        out[v] = R.chain2aln(R.Extender(host, oracle, _rtl_ref, p, wl), p, wl)
    return out


def check(got, want, n_seeds, n_chains, n_reads):
    regs, ext, start, st = got
    wregs, wext, _ = want
    assert R.same_regions(regs, wregs) is None, R.same_regions(regs, wregs)
    assert [int(x) for x in ext] == [int(x) for x in wext]
    counts = np.bincount([a["read"] for a in wregs], minlength=n_reads)
    assert (np.diff(start.astype(np.int64)) == counts).all()
    assert st == dict(seeds_gpu=n_seeds, seeds_bwa=len(wregs), regs=len(wregs), chains=n_chains, reads=n_reads)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("pair", [False, True])
def test_both_forms_equal_the_sequential_reference(host, wl, arrays, reference, variant, pair):
    ch, sd, lens = arrays
    assert 3000 <= len(sd) <= 4200
    p = host.default_params(variant=variant)
    with host.BswContext(device=0, kernel=host.KERNEL_AUTO, result_format=host.RESULT_PAIR if pair else host.RESULT_FULL) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            j1 = c.chain2aln_start(p, ref, ch, sd, reads=wl["reads"])
            j2 = c.chain2aln_start(p, ref, ch, sd, rd=rd)
            assert c.inflight() == 2 and j1.stats()["seeds_gpu"] == len(sd) and j1.stats()["regs"] == 0
            got2 = j2.finish()
            got1 = j1.finish()
            assert c.inflight() == 0
            check(got1, reference[variant], len(sd), len(ch), len(lens))
            check(got2, reference[variant], len(sd), len(ch), len(lens))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_a_reads_seeds_in_different_chunks(host, oracle):
    """about 20 000 seeds in chunks of 8 192: the replay reads a read's records across chunk boundaries"""
    wl = R.make_workload(1750, seed=6)
    ch, sd, lens = R.arrays(host, wl)
    assert 17000 <= len(sd) <= 24000
    p = host.default_params()
    want = R.chain2aln(R.Extender(host, oracle, _rtl_ref, p, wl), p, wl)
    with host.BswContext(device=0, chunk_tasks=8192) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            chunks0 = c.host_stats()["chunks"]
            got = c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()
            nch = c.host_stats()["chunks"] - chunks0
            assert nch >= 2                                                  # equal chunks, round(n / chunk_tasks) of them
            per = (-(-len(sd) // nch) + 255) & ~255                           # ... each rounded up to 256 seeds
            idx = np.repeat(ch["read"], ch["n_seeds"])
            assert idx[per - 1] == idx[per]                                  # the cut goes through a read's seeds
            check(got, want, len(sd), len(ch), len(lens))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def side_tickets(host, wl, n=200):
    """a rescue and a CIGAR task per chain of the first reads: the read against the reference around its first seed"""
    L = wl["l_pac"]
    mt, ct = np.zeros(n, dtype=host.MTASK), np.zeros(n, dtype=host.CTASK)
    for k, c in enumerate(wl["chains"][:n]):
        r = wl["reads"][c["read"]]
        rbeg, qbeg = c["seeds"][0][0], c["seeds"][0][1]
        lo, hi = (0, L) if rbeg < L else (L, 2 * L)
        mt[k] = (r.ctypes.data, len(r), 0, max(rbeg - 300, lo), min(rbeg + 300, hi), mr.xtra_of(len(r), 1, 19), 19)
        rb = min(max(rbeg - qbeg, lo), hi - len(r))
        ct[k]["query"], ct[k]["l_query"], ct[k]["w"], ct[k]["rb"], ct[k]["re"] = r.ctypes.data, len(r), 10, rb, rb + len(r)
        ct[k]["min_score"], ct[k]["max_tries"] = INT_MIN, 1
    return mt, ct


def test_a_job_between_a_rescue_and_a_cigar_ticket(host, wl, arrays, reference):
    ch, sd, lens = arrays
    p = host.default_params()
    mt, ct = side_tickets(host, wl)
    with host.BswContext(device=0, chunk_tasks=1024) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            t, wm = c.submit_matesw_ref(p, ref, mt)
            c.wait_ticket(t)
            t, wc, wcig, wmd = c.submit_cigar_ref(p, ref, ct)
            c.wait_ticket(t)
            assert (wm["status"] == 0).sum() > 50 and (wc["status"] == 0).sum() > 50
            t_m, rm = c.submit_matesw_ref(p, ref, mt)
            job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
            t_c, rc, rcig, rmd = c.submit_cigar_ref(p, ref, ct)
            job2 = c.chain2aln_start(p, ref, ch, sd, reads=wl["reads"])
            assert c.inflight() == 4
            with pytest.raises(host.BswError) as ei:                       # the fifth submit: refused, and no job is left
                c.chain2aln_start(p, ref, ch, sd, rd=rd)
            assert ei.value.code == -6 and c.inflight() == 4
            c.wait_ticket(t_c)
            got = job.finish()
            c.wait_ticket(t_m)
            got2 = job2.finish()
            assert c.inflight() == 0
            check(got, reference[0], len(sd), len(ch), len(lens))
            check(got2, reference[0], len(sd), len(ch), len(lens))
            assert rm.tobytes() == wm.tobytes() and rc.tobytes() == wc.tobytes()
            assert c.md_strings(rc, rmd) == c.md_strings(wc, wmd)
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_the_poll_reaches_one_without_blocking(host, wl, arrays, reference):
    ch, sd, lens = arrays
    p = host.default_params()
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
            polls, longest, deadline = 0, 0.0, time.monotonic() + 60
            while True:
                t0 = time.monotonic()
                done = job.test()
                longest = max(longest, time.monotonic() - t0)
                polls += 1
                if done or time.monotonic() > deadline:
                    break
            assert done and c.inflight() == 1                                # complete, and still the caller's to collect
            assert job.test() and longest < 0.5
            print("polls: %d, the longest took %.1f us" % (polls, longest * 1e6))
            check(job.finish(), reference[0], len(sd), len(ch), len(lens))
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_an_over_limit_seed_is_the_submits_error_and_leaves_no_job(host, wl):
    g = wl["both"]
    read = g[2000:2000 + 8300].copy()
    ch = np.zeros(1, dtype=host.CHAIN)
    ch[0] = (0, 1, 0, 0, 0, 0, 0)
    sd = np.zeros(1, dtype=host.CSEED)
    sd[0] = (2000 + 8250, 8250, 30, 30, 0)                                   # a left flank of 8 250 bases: beyond BSW_MAX_QLEN
    p = host.default_params()
    host.chain2aln_plan(p, wl["l_pac"], ch, sd, [len(read)])                  # the plan has no objection
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload([read])
        try:
            with pytest.raises(host.BswError) as ei:
                c.chain2aln_start(p, ref, ch, sd, rd=rd)
            assert ei.value.code == -3 and "BSW_MAX_QLEN" in str(ei.value) and c.inflight() == 0
            c.reads_free(rd)                                                 # the refused job does not hold the block
            rd = None
        finally:
            if rd is not None:
                c.reads_free(rd)
            c.ref_free(ref)


def test_a_job_that_is_dropped_gives_its_place_and_its_block_back(host, wl, arrays, reference):
    ch, sd, lens = arrays
    p = host.default_params()
    c = host.BswContext(device=0)
    ref = c.ref_upload(wl["pac"], wl["l_pac"])
    rd = c.reads_upload(wl["reads"])
    with c.chain2aln_start(p, ref, ch, sd, rd=rd) as job:                    # left without finish()
        assert c.inflight() == 1
    assert c.inflight() == 0 and job.handle is None
    job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
    del job                                                                  # collected without finish()
    assert c.inflight() == 0
    c.reads_free(rd)                                                         # no job holds the block
    rd = c.reads_upload(wl["reads"])
    open_job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
    check(c.chain2aln_start(p, ref, ch, sd, rd=rd).finish(), reference[0], len(sd), len(ch), len(lens))
    assert c.inflight() == 1
    c.close()                                                                # releases the job that is still open, then the context
    assert open_job.handle is None
