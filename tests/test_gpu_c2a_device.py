"""mem_chain2aln's seed loop replayed on the GPU (bsw_c2a_replay_kernel in the companion library): bsw_chain2aln_replay_batch, its
ticket and the chain2aln job with the switch on, byte for byte against the host's bsw_chain2aln_replay on the same arrays.  The
sets are synthetic (tests/_c2a_device_gen.py): no DP runs, so the shapes are the smallest at which the kernel can go wrong — chain
sizes at the edges of a 16-lane row and of a wavefront, around the cap of the host route, read counts at the rows of a wavefront
and the edge of a workgroup."""
import os
import time

import numpy as np
import pytest

import _c2a_device_gen as G
import _chain2aln_ref as R
import _rtl_ref

pytestmark = pytest.mark.gpu

EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


@pytest.fixture(scope="module")
def c(host):
    host.c2a_device_load()
    with host.BswContext(device=0) as ctx:
        yield ctx


def both_calls(host, c, p, s, results=None, opt=None, want_extended=True):
    """the synchronous call and the ticket on the same arrays -> their two results, each checked against the host replay"""
    res = s["pairs"] if results is None else results
    want = G.host_replay(host, p, s, results=res, opt=opt)
    got = host.chain2aln_replay_batch(c, p, s["chains"], s["seeds"], s["lens"], res, opt=opt, want_extended=want_extended)
    t, r = c.submit_chain2aln_replay(p, s["chains"], s["seeds"], s["lens"], res, opt=opt, want_extended=want_extended)
    assert c.inflight() == 1
    c.wait_ticket(t)
    assert c.inflight() == 0
    out = []
    for g in (got, r.result()):
        regs, ext, start, st = g
        assert G.same((regs, ext, start), want) is None, G.same((regs, ext, start), want)
        if not want_extended:
            assert ext is None
        n_with_chain = len(np.unique(s["chains"]["read"]))
        assert st["reads_gpu"] + st["reads_host"] == n_with_chain and st["chunks"] >= (1 if n_with_chain else 0)
        n, nr = len(s["seeds"]), n_with_chain
        assert st["d2h_bytes"] <= 64 * len(regs) + 8 * nr + (n if want_extended else 0) + 256 * max(st["chunks"], 1)
        out.append(g)
    return out


@pytest.mark.parametrize("n_reads", [1, 3, 4, 5, 63, 64, 65])
def test_row_and_wavefront_edges(host, c, n_reads):
    """chain sizes at the row and wavefront edges; read counts at the rows of a wavefront and the edge of a workgroup (16 rows)"""
    s = G.make(host, n_reads, EDGES, seed=100 + n_reads)
    (a, _) = both_calls(host, c, host.default_params(), s)
    assert a[3]["reads_host"] == 0 and a[3]["reads_gpu"] == n_reads


def test_every_edge_size_alone_and_mixed(host, c):
    """a read per edge size with that one chain, then reads that mix them: every size is the first, a middle and the last chain"""
    fixed = {r: [n] for r, n in enumerate(EDGES)}
    fixed.update({10 + r: [EDGES[(r + k) % len(EDGES)] for k in range(3)] for r in range(len(EDGES))})
    s = G.make(host, 20, EDGES, seed=7, chain_sizes=fixed)
    both_calls(host, c, host.default_params(), s)


def test_the_cap_and_the_host_route(host, c):
    cap = host.C2A_DEV_MAX_CHAIN
    fixed = {1: [cap - 1, 3], 3: [cap], 4: [2, cap + 1, 5], 6: [cap + 1], 9: [17, cap]}
    s = G.make(host, 12, G.SMALL, seed=21, chain_sizes=fixed)
    for g in both_calls(host, c, host.default_params(), s):
        regs, ext, start, st = g
        assert st["reads_host"] == 2 and st["reads_gpu"] == 10          # exactly the reads that hold a chain ABOVE the cap: 4 and 6
        assert (np.diff(regs["read"].astype(np.int64)) >= 0).all()      # GPU and host reads interleave in read order
        assert {4, 6} <= set(regs["read"].tolist()) and {3, 5, 7} <= set(regs["read"].tolist())


@pytest.mark.parametrize("empty", [(0, 1), (5, 6, 7), (18, 19), (0, 9, 19)])
def test_reads_without_any_chain(host, c, empty):
    s = G.make(host, 20, G.MIDDLE, seed=31, empty=empty)
    (a, _) = both_calls(host, c, host.default_params(), s)
    assert a[3]["reads_gpu"] == 20 - len(empty)
    for r in empty:
        assert a[2][r] == a[2][r + 1]


def test_no_seed_at_all(host, c):
    s = G.make(host, 5, G.SMALL, seed=3, empty=range(5))
    assert len(s["seeds"]) == 0 and len(s["chains"]) == 0
    for regs, ext, start, st in both_calls(host, c, host.default_params(), s):
        assert len(regs) == 0 and (start == 0).all() and st["reads_gpu"] == 0 and st["chunks"] == 0


def test_full_records_with_junk_in_the_tail_and_no_extended(host, c):
    s = G.make(host, 40, G.MIDDLE, seed=41)
    full = G.full_records(host, s["pairs"])
    a = both_calls(host, c, host.default_params(), s, results=full)[0]
    b = both_calls(host, c, host.default_params(), s)[0]
    assert a[0].tobytes() == b[0].tobytes()
    both_calls(host, c, host.default_params(), s, results=full, want_extended=False)
    both_calls(host, c, host.default_params(), s, want_extended=False)


def test_options_and_penalties(host, c):
    s = G.make(host, 40, G.MIDDLE, seed=51)
    seen = set()
    for pen in G.PENALTIES:
        p = G.params(host, **pen)
        for f0 in (.1, -1.0, 1.0 / 3):
            for fo in (.95, 2.0 / 3):
                a = both_calls(host, c, p, s, opt=dict(seedlen0_frac=f0, ovl_len_frac=fo))[0]
                seen.add(a[1].tobytes())
    assert len(seen) >= 6                                               # the options and penalties do change what is extended


def test_positions_beyond_2_to_the_33(host, c):
    s = G.make(host, 30, G.MIDDLE, seed=61, d0_base=1 << 33)
    assert (s["seeds"]["rbeg"] > (1 << 33)).all()
    regs = both_calls(host, c, host.default_params(), s)[0][0]
    assert (regs["rb"] > (1 << 33) - 1000).all()


# ---- chunk cuts ----
@pytest.mark.parametrize("chunk", [1, 256, 4096])
def test_chunk_cuts(host, c, chunk):
    """BSW_C2A_DEV_CHUNK seeds per chunk: a chunk per read, chunks of a few reads, and chunks that a read with more seeds than the
    target keeps whole; with a host-route read among them"""
    cap = host.C2A_DEV_MAX_CHAIN
    s = G.make(host, 90, G.MIDDLE, seed=71, empty=(0, 44, 89), chain_sizes={10: [cap + 1, 4], 50: [300, 300]})
    os.environ["BSW_C2A_DEV_CHUNK"] = str(chunk)
    try:
        for regs, ext, start, st in both_calls(host, c, host.default_params(), s):
            with_chain = 87
            want_chunks = {1: with_chain, 256: None, 4096: None}[chunk]
            assert st["chunks"] > 1 and (want_chunks is None or st["chunks"] == want_chunks)
            assert st["reads_host"] == 1
    finally:
        del os.environ["BSW_C2A_DEV_CHUNK"]


def test_several_tickets_in_flight(host, c):
    s = [G.make(host, 50, G.MIDDLE, seed=80 + k) for k in range(4)]
    p = host.default_params()
    os.environ["BSW_C2A_DEV_CHUNK"] = "512"
    try:
        t = [c.submit_chain2aln_replay(p, x["chains"], x["seeds"], x["lens"], x["pairs"]) for x in s]
        assert c.inflight() == 4
        with pytest.raises(host.BswError) as ei:
            c.submit_chain2aln_replay(p, s[0]["chains"], s[0]["seeds"], s[0]["lens"], s[0]["pairs"])
        assert ei.value.code == -6 and c.inflight() == 4
        with pytest.raises(host.BswError) as ei:                        # the synchronous call while tickets are uncollected
            host.chain2aln_replay_batch(c, p, s[0]["chains"], s[0]["seeds"], s[0]["lens"], s[0]["pairs"])
        assert ei.value.code == -6
        for (tk, r), x in reversed(list(zip(t, s))):
            c.wait_ticket(tk)
            regs, ext, start, st = r.result()
            assert G.same((regs, ext, start), G.host_replay(host, p, x)) is None
        assert c.inflight() == 0
    finally:
        del os.environ["BSW_C2A_DEV_CHUNK"]


def test_bad_arrays_are_refused_as_by_the_host_replay(host, c):
    s = G.make(host, 6, G.SMALL, seed=5)
    bad = dict(s, chains=s["chains"].copy())
    bad["chains"]["first_seed"][1] += 1
    with pytest.raises(host.BswError) as e1:
        G.host_replay(host, host.default_params(), bad)
    with pytest.raises(host.BswError) as e2:
        host.chain2aln_replay_batch(c, host.default_params(), bad["chains"], bad["seeds"], bad["lens"], bad["pairs"])
    with pytest.raises(host.BswError) as e3:
        c.submit_chain2aln_replay(host.default_params(), bad["chains"], bad["seeds"], bad["lens"], bad["pairs"])
    assert e1.value.code == e2.value.code == e3.value.code == -2 and c.inflight() == 0
    assert "do not follow the previous chain's" in str(e3.value)


# ---- the job with the switch on ----
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


def check_job(got, off, want, n_seeds, n_chains, n_reads):
    regs, ext, start, st = got
    for a, b in zip(got[:3], off[:3]):
        assert a.tobytes() == b.tobytes()                                # byte for byte the job with the switch off
    assert st == off[3]
    wregs, wext, _ = want
    assert R.same_regions(regs, wregs) is None, R.same_regions(regs, wregs)
    assert [int(x) for x in ext] == [int(x) for x in wext]
    assert st == dict(seeds_gpu=n_seeds, seeds_bwa=len(wregs), regs=len(wregs), chains=n_chains, reads=n_reads)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("pair", [False, True])
def test_the_job_with_the_switch_on(host, wl, arrays, reference, variant, pair):
    ch, sd, lens = arrays
    p = host.default_params(variant=variant)
    host.c2a_device_load()
    with host.BswContext(device=0, kernel=host.KERNEL_AUTO, result_format=host.RESULT_PAIR if pair else host.RESULT_FULL) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        try:
            off = [c.chain2aln_start(p, ref, ch, sd, reads=wl["reads"]).finish(), c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()]
            host.set_c2a_device(1)
            try:
                for k, kw in enumerate((dict(reads=wl["reads"]), dict(rd=rd))):
                    job = c.chain2aln_start(p, ref, ch, sd, **kw)
                    host.set_c2a_device(0)                                # the job has its snapshot: the switch no longer matters to it
                    assert c.inflight() == 1
                    seen = set()
                    while not job.test():
                        seen.add(c.inflight())
                    seen.add(c.inflight())
                    # collect and re-submit happen inside one test(): the caller only ever sees ONE submit, and the complete job is still its to collect
                    assert seen == {1} and c.inflight() == 1
                    got = job.finish()
                    assert c.inflight() == 0
                    check_job(got, off[k], reference[variant], len(sd), len(ch), len(lens))
                    host.set_c2a_device(1)
                # the blocking form alone
                got = c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()
                assert c.inflight() == 0
                check_job(got, off[1], reference[variant], len(sd), len(ch), len(lens))
            finally:
                host.set_c2a_device(0)
        finally:
            c.reads_free(rd)
            c.ref_free(ref)


def test_the_poll_of_the_two_stage_job_never_blocks(host, wl, arrays, reference):
    ch, sd, lens = arrays
    p = host.default_params()
    host.c2a_device_load()
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(wl["pac"], wl["l_pac"])
        rd = c.reads_upload(wl["reads"])
        host.set_c2a_device(1)
        try:
            off_job = None
            job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
            polls, longest, deadline = 0, 0.0, time.monotonic() + 60
            while True:
                t0 = time.monotonic()
                done = job.test()
                longest = max(longest, time.monotonic() - t0)
                polls += 1
                if done or time.monotonic() > deadline:
                    break
            assert done and c.inflight() == 1
            assert job.test() and longest < 0.5
            print("polls: %d, the longest took %.1f us" % (polls, longest * 1e6))
            got = job.finish()
            host.set_c2a_device(0)
            off_job = c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()
            check_job(got, off_job, reference[0], len(sd), len(ch), len(lens))
        finally:
            host.set_c2a_device(0)
            c.reads_free(rd)
            c.ref_free(ref)


def test_a_dropped_job_gives_its_place_and_its_block_back(host, wl, arrays, reference):
    """with the switch on: dropped while the extension ticket is in flight, dropped once test() has submitted the replay ticket,
    and beside three other tickets (the job is the fourth submit; a fifth is refused)"""
    ch, sd, lens = arrays
    p = host.default_params()
    host.c2a_device_load()
    s = G.make(host, 20, G.SMALL, seed=9)
    c = host.BswContext(device=0)
    ref = c.ref_upload(wl["pac"], wl["l_pac"])
    rd = c.reads_upload(wl["reads"])
    host.set_c2a_device(1)
    try:
        with c.chain2aln_start(p, ref, ch, sd, rd=rd) as job:               # left without finish()
            assert c.inflight() == 1
        assert c.inflight() == 0 and job.handle is None
        job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
        deadline = time.monotonic() + 60
        while not job.test() and time.monotonic() < deadline:             # (the replay ticket is complete and uncollected)
            pass
        assert c.inflight() == 1
        del job
        assert c.inflight() == 0
        c.reads_free(rd)                                                  # no job holds the block
        rd = c.reads_upload(wl["reads"])
        fill = [c.submit_chain2aln_replay(p, s["chains"], s["seeds"], s["lens"], s["pairs"]) for _ in range(3)]
        job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
        assert c.inflight() == 4
        with pytest.raises(host.BswError) as ei:
            c.chain2aln_start(p, ref, ch, sd, rd=rd)
        assert ei.value.code == -6 and c.inflight() == 4
        got = job.finish()                                               # collects the extension ticket, takes the place again for the replay
        assert c.inflight() == 3
        host.set_c2a_device(0)
        for t, r in fill:
            c.wait_ticket(t)
        off = c.chain2aln_start(p, ref, ch, sd, rd=rd).finish()
        check_job(got, off, reference[0], len(sd), len(ch), len(lens))
        open_job = c.chain2aln_start(p, ref, ch, sd, rd=rd)
        assert c.inflight() == 1
    finally:
        host.set_c2a_device(0)
        c.close()                                                        # releases the job that is still open, then the context
    assert open_job.handle is None
