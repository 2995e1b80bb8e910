"""GPU tests of bsw_cigar_ref_submit_t / bsw_matesw_ref_submit_t: the CIGAR and mate-rescue stages as tickets of the slot pipeline.

The submits must equal the restatements of bwa in tests/_gencigar_ref.py / tests/_matesw_ref.py (through the checkers of
test_gpu_cigar_ref.py / test_gpu_matesw_ref.py, which are handed a context whose batch calls submit, poll and collect) and the
synchronous calls bit for bit; on one device, on devices=[0, 0] and [0, 0, 0] (one ordinal listed more than once: more slots on
one GPU) with submits of more chunks than slots, and beside a stream of extension submits on one context.  No test provokes a
GPU fault: the failing submits are malformed arguments, which never reach the device."""
import time

import numpy as np
import pytest

import _gencigar_ref as gc
import test_gpu_cigar_ref as tc
import test_gpu_matesw_ref as tm

pytestmark = pytest.mark.gpu

L_PAC = tc.L_PAC
assert tm.L_PAC == L_PAC


class ViaSubmit:
    """cigar_ref_batch / matesw_ref_batch with the signature of BswContext's, run as ticketed submits: polled with bsw_test until
    complete, then collected."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.polls = 0

    def _collect(self, t):
        t0 = time.perf_counter()
        while not self.ctx.test(t):
            self.polls += 1
            assert time.perf_counter() - t0 < 120
            time.sleep(0.0002)
        self.ctx.wait_ticket(t)

    def cigar_ref_batch(self, p, ref, ct, max_cigar=64, max_md=256, want_cigar=True, want_md=True):
        t, res, cig, md = self.ctx.submit_cigar_ref(p, ref, ct, max_cigar=max_cigar, max_md=max_md, want_cigar=want_cigar, want_md=want_md)
        assert t and self.ctx.inflight() >= 1
        self._collect(t)
        return res, cig, (self.ctx.md_strings(res, md) if want_md else None)

    def matesw_ref_batch(self, p, ref, mt):
        t, res = self.ctx.submit_matesw_ref(p, ref, mt)
        assert t
        self._collect(t)
        return res


def same_cigar_outputs(a, b):
    """(res, cig, md strings) of two calls: every byte of the records, the CIGAR words a record announces, the MD strings"""
    ra, ca, ma = a
    rb, cb, mb = b
    assert ra.tobytes() == rb.tobytes()
    n = np.clip(ra["n_cigar"], 0, ca.shape[1])
    mask = np.arange(ca.shape[1])[None, :] < n[:, None]
    assert (ca[mask] == cb[mask]).all()
    assert ma == mb


@pytest.fixture(scope="module")
def cgenome(ctx):
    rng = np.random.default_rng(2024)
    pac = gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))
    ref = ctx.ref_upload(pac, L_PAC)
    yield pac, ref
    ctx.ref_free(ref)


def rescue_specs(pac, n, seed, lengths=(150, 250), extra=(250, 450)):
    """the shape of test_gpu_matesw_ref.py: both strands, both orientations, junk mates (status 2), windows bwa does not run
    (status 1), 150 and 250 bp"""
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        strand, is_rev = i & 1, (i >> 1) & 1
        l_ms = lengths[(i >> 2) % len(lengths)]
        if i % 41 == 7:
            rb, re = L_PAC - 100, L_PAC + 100                           # bridges l_pac: status 1
        elif i % 97 == 11:
            rb, re = 5000, 5000                                         # empty: status 1
        else:
            rb, re = tm.window(rng, strand, l_ms + int(rng.integers(*extra)))
        specs.append(tm.task(tm.mate_in(rng, pac, rb, re, l_ms, is_rev, junk=0.1, nrate=0.001), is_rev, rb, re))
    return specs


def cigar_specs(pac, n, seed, lengths=(150, 250)):
    """150 and 250 bp reads on both strands with retries, the no-gap shortcut and bwa's no-alignment answers mixed in"""
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(n):
        strand = i & 1
        lq = lengths[(i >> 1) % len(lengths)]
        k = i % 29
        if k == 3:
            q = tc.read_of(rng, pac, 1000, 1100, 100)
            rb, re = [(5000, 5000), (L_PAC - 50, L_PAC + 50), (-20, 80)][(i // 29) % 3]
            specs.append(tc.spec(q, rb, re))                            # status 1
        elif k == 5:
            rb, re = tc.interval(rng, lq, strand)
            specs.append(tc.spec(tc.read_of(rng, pac, rb, re, lq, 0.05, 0.0), rb, re, w=0, w_cap=50 * (i & 2), min_score=1000, max_tries=3))
        elif k in (7, 9):
            rb, _ = tc.interval(rng, 150, strand)
            steps = [6, 6, -12] if k == 7 else [6, -6]
            specs.append(tc.spec(tc.retry_read(rng, pac, rb, steps), rb, rb + 150, w=4, w_cap=64, min_score=1000, max_tries=3))
        else:
            rb, re = tc.interval(rng, lq + int(rng.integers(-6, 7)), strand)
            specs.append(tc.spec(tc.read_of(rng, pac, rb, re, lq, 0.03, 0.01, 0.002), rb, re, w=int(rng.choice([5, 40, 100])),
                                 w_cap=int(rng.choice([0, 200])), min_score=int(rng.integers(100, 240)), max_tries=int(rng.integers(1, 4))))
    return specs


# ---- one device: the session context -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", ["staged", "registered"])
def test_cigar_submit_equals_the_restatement_and_the_batch_call(host, oracle, ctx, cgenome, memory):
    """The mixed batch of test_gpu_cigar_ref.py — reads of 1 to 8 191 bases (the long global kernel runs from a slot), both
    strands, the strand edges, the no-gap shortcut, 1 / 2 / 3 tries, all of bwa's no-alignment answers."""
    pac, ref = cgenome
    specs = tc.build_mixed(pac)
    arena = host.HostArena(sum(len(s["read"]) + 1 for s in specs) + 64) if memory == "registered" else None
    try:
        p = host.default_params()
        via = ViaSubmit(ctx)
        res, cig, md, want = tc.check(host, oracle, via, p, cgenome, specs, arena=arena)
        assert {int(x) for x in res["tries"]} >= {1, 2, 3} and (res["status"] == 1).sum() == 6
        ct, keep = tc.make_ctasks(host, specs, arena)
        same_cigar_outputs((res, cig, md), ctx.cigar_ref_batch(p, ref, ct, max_cigar=64, max_md=4096))
        # CIGAR and MD overflow, and the outputs a caller may leave out
        tc.check(host, oracle, via, p, cgenome, specs[:120], max_cigar=3, max_md=12, arena=arena, want=want[:120])
        r2, c2, m2 = via.cigar_ref_batch(p, ref, ct, want_cigar=False, want_md=False)
        assert c2 is None and m2 is None
        r3, _, _ = ctx.cigar_ref_batch(p, ref, ct, want_cigar=False, want_md=False)
        assert r2.tobytes() == r3.tobytes()
        assert ctx.inflight() == 0
    finally:
        if arena is not None:
            arena.free()


@pytest.mark.parametrize("memory", ["pageable", "registered"])
def test_matesw_submit_equals_the_restatement_and_the_batch_call(host, oracle, ctx, cgenome, memory):
    pac, ref = cgenome
    specs = rescue_specs(pac, 6000, 21)
    arena = host.HostArena(sum(len(s["mate"]) + 1 for s in specs) + 64) if memory == "registered" else None
    try:
        p = host.default_params()
        res, _ = tm.check(host, oracle, ViaSubmit(ctx), p, cgenome, specs, arena=arena)
        assert all((res["status"] == s).any() for s in (0, 1, 2))
        mt, keep = tm.make_mtasks(host, specs, arena)
        assert res.tobytes() == ctx.matesw_ref_batch(p, ref, mt).tobytes()
        # every align class and flag combination through a slot
        rng = np.random.default_rng(4)
        more = []
        for l_ms in tm.class_lengths():
            for is_rev in (0, 1):
                for byte in (0, tm.XBYTE):
                    rb, re = tm.window(rng, is_rev, l_ms + int(rng.integers(50, 600)))
                    more.append(tm.task(tm.mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.02), is_rev, rb, re, xtra=tm.XSUBO | tm.XSTART | 19 | byte, min_score=1))
        tm.check(host, oracle, ViaSubmit(ctx), p, cgenome, more)
    finally:
        if arena is not None:
            arena.free()


def test_empty_submits_and_a_null_ticket(host, ctx, cgenome):
    _, ref = cgenome
    p = host.default_params()
    t, res = ctx.submit_matesw_ref(p, ref, np.zeros(0, dtype=host.MTASK))
    assert t and ctx.test(t) and len(res) == 0
    t2, res2, cig2, md2 = ctx.submit_cigar_ref(p, ref, np.zeros(0, dtype=host.CTASK))
    assert t2 and t2 != t and ctx.test(t2) and ctx.inflight() == 2
    ctx.wait()
    assert ctx.inflight() == 0
    rc = host.lib().bsw_matesw_ref_submit_t(ctx.handle, p.ctypes.data, ref, None, 0, None, None)     # ticket may be NULL
    assert rc == 0 and ctx.inflight() == 1
    ctx.wait()


def test_malformed_submits_make_no_ticket(host, ctx, cgenome):
    """The argument checks of the batch calls, with their codes and texts, in the caller's thread: nothing reaches the device."""
    _, ref = cgenome
    p = host.default_params()
    m = np.zeros(1100, dtype=np.uint8)

    def mtasks(**f):
        mt = np.zeros(3, dtype=host.MTASK)
        for t in mt:
            t["mate"], t["l_ms"], t["rb"], t["re"], t["xtra"] = m.ctypes.data, 100, 0, 500, tm.XSUBO | tm.XSTART | 19
        for k, v in f.items():
            mt[2][k] = v
        return mt

    def ctasks(**f):
        ct = np.zeros(3, dtype=host.CTASK)
        for t in ct:
            t["query"], t["l_query"], t["rb"], t["re"], t["w"], t["max_tries"] = m.ctypes.data, 100, 0, 110, 20, 1
        for k, v in f.items():
            ct[2][k] = v
        return ct

    def both(submit, batch):
        with pytest.raises(host.BswError) as a:
            submit()
        with pytest.raises(host.BswError) as b:
            batch()
        assert ctx.inflight() == 0
        return a.value, b.value

    for f, code in ((dict(l_ms=1025), -3), (dict(rb=1000, re=1000 + 65536), -3), (dict(l_ms=-1), -2), (dict(mate=0), -2), (dict(is_rev=2), -2),
                    (dict(xtra=0x100000), -2)):
        a, b = both(lambda: ctx.submit_matesw_ref(p, ref, mtasks(**f)), lambda: ctx.matesw_ref_batch(p, ref, mtasks(**f)))
        assert a.code == b.code == code and "mate task 2" in str(a) and str(a).split(": ", 1)[1] == str(b).split(": ", 1)[1], (f, str(a), str(b))
    for f, code in ((dict(l_query=8192), -3), (dict(rb=1000, re=1000 + 65536), -3), (dict(w=65536), -3), (dict(l_query=-1), -2), (dict(query=0), -2),
                    (dict(max_tries=4), -2), (dict(w_cap=-1), -2)):
        a, b = both(lambda: ctx.submit_cigar_ref(p, ref, ctasks(**f)), lambda: ctx.cigar_ref_batch(p, ref, ctasks(**f)))
        assert a.code == b.code == code and "cigar task 2" in str(a) and str(a).split(": ", 1)[1] == str(b).split(": ", 1)[1], (f, str(a), str(b))
    with pytest.raises(host.BswError) as e:
        ctx.submit_matesw_ref(p, None, mtasks())
    assert e.value.code == -2
    with pytest.raises(host.BswError) as e:
        ctx.submit_cigar_ref(p, ref, ctasks(), max_cigar=0)
    assert e.value.code == -2
    with pytest.raises(host.BswError) as e:
        ctx.submit_matesw_ref(host.default_params(mat=np.full(25, -1, np.int8)), ref, mtasks())
    assert e.value.code == -2
    # ... and the context goes on working
    t, res = ctx.submit_matesw_ref(p, ref, mtasks())
    ctx.wait_ticket(t)
    assert res.tobytes() == ctx.matesw_ref_batch(p, ref, mtasks()).tobytes()


# ---- one ordinal listed more than once: more slots on one GPU, more chunks than slots --------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_submits_of_more_chunks_than_slots_on_repeated_ordinals(host, oracle, devices):
    """Submits large enough to be cut into more chunks than the context has slots (checked through bsw_host_stats), chunk k on
    "device" k mod n with that entry's copy of the reference.  Every result is compared with the synchronous call bit for bit;
    the restatements of bwa are computed for every 16th task of the CIGAR submit (a Python loop) and for the whole rescue submit."""
    p = host.default_params()
    rng = np.random.default_rng(99)
    pac = gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))
    nslots = 4 * len(devices)
    # Sized from the work targets of a chunk (2^31 cells of rescue, 2^28 of CIGAR: bsw_matesw.hip, bsw_cigar.hip), not from a
    # remainder of the cut: a submit is cut AT the target once it holds more than slots x target.  Rescue: windows of ~2 400
    # bases, ~0.48 M cells a task, 1.3 x slots x target in all; CIGAR: reads of 150, 250 and 1 000 bases, ~0.18 M cells a task.
    n_m, n_c = 24_000 * len(devices), 8_000 * len(devices)
    with host.BswContext(devices=devices) as c:
        ref = c.ref_upload(pac, L_PAC)
        try:
            genome = (pac, ref)
            mspecs = rescue_specs(pac, n_m, 31, extra=(1800, 2600))
            base = c.host_stats()["chunks"]
            res, _ = tm.check(host, oracle, ViaSubmit(c), p, genome, mspecs)
            chunks_m = c.host_stats()["chunks"] - base
            assert chunks_m >= nslots + 2, (chunks_m, nslots)
            assert all((res["status"] == s).any() for s in (0, 1, 2))
            mt, keep = tm.make_mtasks(host, mspecs)
            assert res.tobytes() == c.matesw_ref_batch(p, ref, mt).tobytes()

            cspecs = cigar_specs(pac, n_c, 32, lengths=(150, 250, 1000))
            ct, keep2 = tc.make_ctasks(host, cspecs)
            via = ViaSubmit(c)
            base = c.host_stats()["chunks"]
            got = via.cigar_ref_batch(p, ref, ct, max_cigar=32, max_md=160)
            chunks_c = c.host_stats()["chunks"] - base
            assert chunks_c >= nslots + 2, (chunks_c, nslots)
            assert {int(x) for x in got[0]["tries"]} >= {1, 2, 3} and (got[0]["status"] == 1).any()
            same_cigar_outputs(got, c.cigar_ref_batch(p, ref, ct, max_cigar=32, max_md=160))
            sample = list(range(0, n_c, 16))
            sub = [cspecs[i] for i in sample]
            want = tc.expected(oracle, p, pac, sub)

            class Sampled:
                def cigar_ref_batch(self, *a, **k):
                    return got[0][sample], got[1][sample], [got[2][i] for i in sample]
            tc.check(host, oracle, Sampled(), p, genome, sub, max_cigar=32, max_md=160, want=want)
            st = c.host_stats()
            assert st["seeds"] == 0 and st["submits"] == 2 and st["slot_threads"] == nslots
        finally:
            c.ref_free(ref)


# ---- beside extension ----------------------------------------------------------------------------------------------------------
def test_rescue_and_cigar_in_flight_beside_an_extension_stream(host, oracle):
    """One context: extension submits against the resident reference keep coming while a rescue submit and a CIGAR submit are in
    flight.  Every ticket is polled with bsw_test before it is collected; every result is bit-exact against the oracle (extension)
    and the restatements (rescue, CIGAR).  A fifth submit and the synchronous calls answer BSW_E_BUSY meanwhile and work afterwards."""
    p = host.default_params()
    n, L = 60_000, 150
    arena = host.HostArena(n * L + 64)
    try:
        pac, rt, _ = host.synth_ref_tasks(n, L_PAC, p, arena=arena.u8, seed=11, read_len=L, seed_len_min=19, seed_len_max=60,
                                          seed_at_start=0, sub_rate=0.02, indel_rate=0.004, n_rate=0.002, junk_frac=0.05)
        reads = [arena.u8[i * L:(i + 1) * L] for i in range(n)]
        tasks, keep = host.seeds_to_tasks(p, pac, L_PAC, reads, rt["seed"].copy())
        want_e = oracle.pair_batch(p, tasks, nthreads=8)
        mspecs = rescue_specs(pac, 30_000, 41)
        cspecs = cigar_specs(pac, 6_000, 42)
        want_c = tc.expected(oracle, p, pac, cspecs)
        mt, keep_m = tm.make_mtasks(host, mspecs)
        ct, keep_c = tc.make_ctasks(host, cspecs)
        with host.BswContext(device=0, chunk_tasks=8192) as c:
            ref = c.ref_upload(pac, L_PAC)
            try:
                e1 = c.submit_ref(p, ref, rt); t_e1 = c.last_ticket
                t_m, res_m = c.submit_matesw_ref(p, ref, mt)
                t_c, res_c, cig_c, md_c = c.submit_cigar_ref(p, ref, ct, max_cigar=32, max_md=160)
                e2 = c.submit_ref(p, ref, rt); t_e2 = c.last_ticket
                assert len({t_e1, t_m, t_c, t_e2}) == 4 and c.inflight() == 4
                for fifth in (lambda: c.submit_matesw_ref(p, ref, mt[:100]), lambda: c.submit_cigar_ref(p, ref, ct[:100]), lambda: c.submit_ref(p, ref, rt[:100])):
                    with pytest.raises(host.BswError) as ei:
                        fifth()
                    assert ei.value.code == -6 and c.inflight() == 4
                for sync in (lambda: c.matesw_ref_batch(p, ref, mt[:100]), lambda: c.cigar_ref_batch(p, ref, ct[:100])):
                    with pytest.raises(host.BswError) as ei:
                        sync()
                    assert ei.value.code == -6
                pending = {t_e1, t_m, t_c, t_e2}
                t0 = time.perf_counter()
                while pending:                                          # the status poll, every ticket, before anything is collected
                    pending = {t for t in pending if not c.test(t)}
                    assert time.perf_counter() - t0 < 120
                    time.sleep(0.0005)
                assert c.inflight() == 4
                with pytest.raises(host.BswError) as ei:                # complete, not collected: still busy
                    c.matesw_ref_batch(p, ref, mt[:100])
                assert ei.value.code == -6
                for t in (t_c, t_e2, t_m, t_e1):
                    c.wait_ticket(t)
                assert c.inflight() == 0
                assert e1.tobytes() == want_e.tobytes() and e2.tobytes() == want_e.tobytes()

                class Done:
                    def cigar_ref_batch(self, *a, **k):
                        return res_c, cig_c, c.md_strings(res_c, md_c)

                    def matesw_ref_batch(self, *a, **k):
                        return res_m
                tm.check(host, oracle, Done(), p, (pac, ref), mspecs)
                tc.check(host, oracle, Done(), p, (pac, ref), cspecs, max_cigar=32, max_md=160, want=want_c)
                st = c.host_stats()
                assert st["submits"] == 4 and st["seeds"] == 2 * n
                # both kinds of call work again after the wait
                assert c.matesw_ref_batch(p, ref, mt).tobytes() == res_m.tobytes()
                t, r2 = c.submit_matesw_ref(p, ref, mt)
                c.wait_ticket(t)
                assert r2.tobytes() == res_m.tobytes()
                same_cigar_outputs((res_c, cig_c, c.md_strings(res_c, md_c)), c.cigar_ref_batch(p, ref, ct, max_cigar=32, max_md=160))
            finally:
                c.ref_free(ref)
    finally:
        arena.free()
