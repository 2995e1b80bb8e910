"""Resident read blocks on the GPU: bsw_reads_upload and the three *_reads_* submits.  Their results are compared byte for byte
with the pointer forms (bsw_submit_ref_t, bsw_matesw_ref_submit_t, bsw_cigar_ref_submit_t) given the same read bytes, and with
the CPU references: oracle.pair_batch / _rtl_ref.pair_batch on host-extracted tasks, _matesw_ref.py, _gencigar_ref.reg2aln.

A read of the block starts on a word boundary, so the PHASE at which bsw_pack_kernel's funnel shift starts is the flank's (or
the slice's) first index in its read mod 16: the workloads put every phase, the lengths around a word, reads of 1 base and of
8 210, Ns at the ends, and the first and the last read of the store (the windows that reach into the slack words) on it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _gencigar_ref as gc
import _kernel_ledger
import _matesw_ref as mr
import _rtl_ref as R
import test_gpu_cigar_ref as tc
import test_gpu_matesw_ref as tm

pytestmark = pytest.mark.gpu

L_PAC = tc.L_PAC                       # 300 003: the generators of the two modules above draw their intervals from it
INT_MIN = -(1 << 31)
XBYTE, XSUBO, XSTART = 0x10000, 0x40000, 0x80000


@pytest.fixture(scope="module")
def pac():
    rng = np.random.default_rng(4711)
    return gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))


@pytest.fixture(scope="module")
def both(pac):
    g = gc.unpack_pac(pac, L_PAC)
    return np.concatenate([g, 3 - g[::-1]]).astype(np.uint8)


def same_cigar_outputs(a, b):
    """records byte for byte; the CIGAR words and MD bytes a record announces (what lies behind them in a slot is not defined)"""
    (ra, ca, ma), (rb, cb, mb) = a, b
    nc = np.clip(ra["n_cigar"], 0, ca.shape[1])
    nm = np.clip(ra["md_len"], 0, ma.shape[1] - 1) + 1                 # the NUL included
    cm, mm = np.arange(ca.shape[1])[None, :] < nc[:, None], np.arange(ma.shape[1])[None, :] < nm[:, None]
    return ra.tobytes() == rb.tobytes() and bool((ca[cm] == cb[cm]).all()) and bool((ma[mm] == mb[mm]).all())


class Bound:
    """a context with the reference and one read block on it"""
    def __init__(self, host, pac, reads, **kw):
        self.host, self.ctx = host, host.BswContext(**kw)
        self.ref = self.ctx.ref_upload(pac, L_PAC)
        self.rd = self.ctx.reads_upload(reads)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.reads_free(self.rd)
        self.ctx.ref_free(self.ref)
        self.ctx.close()


# ---- extension ------------------------------------------------------------------------------------------------------------------

EXT_LENS = [1, 15, 16, 17, 31, 32, 33, 150, 151, 250]


def ext_workload(host, both):
    """~300 reads, ~2 000 seeds in shuffled read order -> (reads, RD_TASK, REF_TASK, SEED per task, read index per task)"""
    rng = np.random.default_rng(9)
    lens = [150] + [EXT_LENS[i % len(EXT_LENS)] for i in range(296)] + [3000, 8191 + 19] + [250]
    reads, pos, seeds = [], [], []
    for i, L in enumerate(lens):
        strand = i % 2
        x = int(rng.integers(400, L_PAC - 9000)) + strand * L_PAC
        r = both[x:x + L].copy()
        sub = np.nonzero(rng.random(L) < 0.03)[0]
        r[sub] = (r[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
        if L > 40 and i % 5 == 0:                                   # a deletion in the read
            cut = int(rng.integers(10, L - 10))
            r = np.concatenate([r[:cut], r[cut + 2:], both[x + L:x + L + 2]])
        if i % 6 == 1:
            r[0] = 4                                                # an N at base 0 ...
        if i % 6 == 2:
            r[L - 1] = 4                                            # ... and at the last base
        reads.append(r.astype(np.uint8))
        pos.append(x)
        sl = lambda: int(rng.integers(19, 35))                      # noqa: E731
        mine = []
        if L < 19:
            mine.append((0, L))                                     # the seed is the read: no flank at all
            if L > 1:
                mine += [(0, L - 1), (1, L - 1)]                    # one flank of one base
        elif L < 40:
            mine += [(0, 19), (L - 19, 19), (int(rng.integers(0, L - 19 + 1)), 19)]
        elif L <= 250:
            n1 = sl()
            mine += [(0, n1), (L - sl(), 0)]                        # no left flank; no right flank (length fixed below)
            q0 = 1 + (i * 3) % 16                                   # left flank starts at phase q0 - 1: every phase over the reads
            mine += [(q0, sl()), (q0 + 16, 19 + (i * 5) % 16), (int(rng.integers(1, L - 40)), sl())]
            mine += [(int(rng.integers(1, L - 40)), sl()) for _ in range(10)]
        elif L == 3000:
            mine += [(0, 30), (L - 30, 30), (1000, 40), (2981, 19), (1500, 25)]
        else:
            mine += [(8191, 19), (0, 19), (4000, 30)]               # a left flank of BSW_MAX_QLEN bases, a right flank of as many
        for qb, n in mine:
            if n == 0:
                n = L - qb
            seeds.append((i, qb, n))
    # an N just inside a flank: next to the seed on either side
    for k, (i, qb, n) in enumerate(seeds):
        if k % 23 == 0 and qb > 0:
            reads[i][qb - 1] = 4
        if k % 29 == 0 and qb + n < len(reads[i]):
            reads[i][qb + n] = 4
    order = rng.permutation(len(seeds))
    n = len(order)
    rdt, rft, sd, idx = np.zeros(n, dtype=host.RD_TASK), np.zeros(n, dtype=host.REF_TASK), np.zeros(n, dtype=host.SEED), np.zeros(n, dtype=np.int64)
    rmax = np.zeros(2, dtype=np.int64)
    p = host.default_params()
    for k, o in enumerate(order):
        i, qb, ln = seeds[o]
        sd[k] = (pos[i] + qb, qb, ln)
        host.lib().bsw_chain_window(p.ctypes.data, sd[k:k + 1].ctypes.data, 1, len(reads[i]), L_PAC, rmax.ctypes.data)
        for t in (rdt, rft):
            t[k]["init_score"], t[k]["seed"], t[k]["rmax0"], t[k]["rmax1"], t[k]["tag"] = -1, sd[k], rmax[0], rmax[1], k
        rdt[k]["read"] = i
        rft[k]["query"], rft[k]["l_query"] = reads[i].ctypes.data, len(reads[i])
        idx[k] = i
    return reads, rdt, rft, sd, idx


@pytest.fixture(scope="module")
def ext(host, both):
    return ext_workload(host, both)


@pytest.fixture(scope="module")
def ext_want(host, oracle, pac, ext):
    """the CPU references on host-extracted tasks, once per variant"""
    reads, rdt, rft, sd, idx = ext
    p = host.default_params()
    tasks, keep = host.seeds_to_tasks(p, pac, L_PAC, [reads[i] for i in idx], sd)
    tasks["tag"] = rdt["tag"]
    out = {0: oracle.pair_batch(host.default_params(variant=0), tasks, nthreads=8),
           1: oracle.pair_batch(host.default_params(variant=1), tasks, nthreads=8),
           2: R.pair_batch(host.default_params(variant=2), tasks)}
    return out, keep


def test_extension_workload_covers_what_it_claims(ext):
    reads, rdt, rft, sd, idx = ext
    assert 1900 <= len(rdt) <= 2300 and 290 <= len(reads) <= 310
    L = np.array([len(reads[i]) for i in idx])
    qb, ln = sd["qbeg"], sd["len"]
    assert (qb == 0).sum() > 200 and (qb + ln == L).sum() > 200
    left, right = qb > 0, qb + ln < L
    assert set(((qb - 1) & 15)[left]) == set(range(16)) and set(((qb + ln) & 15)[right]) == set(range(16))
    assert (qb == 8191).any() and (L - qb - ln == 8191).any()
    last = len(reads) - 1
    assert ((idx == 0) & left).any() and ((idx == last) & right).any()          # the flanks that touch the slack words
    assert (np.diff(idx) < 0).any() and np.bincount(idx).max() >= 5              # shuffled; several seeds per read
    assert any(r[0] == 4 for r in reads) and any(r[-1] == 4 for r in reads)


@pytest.mark.parametrize("variant,kernel,pair", [(0, 0, False), (1, 1, False), (2, 0, False), (0, 2, False), (0, 0, True), (1, 2, True)])
def test_extension_equals_the_pointer_form_and_the_oracle(host, pac, ext, ext_want, variant, kernel, pair):
    reads, rdt, rft, sd, idx = ext
    want, _ = ext_want
    p = host.default_params(variant=variant)
    with Bound(host, pac, reads, device=0, kernel=kernel, chunk_tasks=512,
               result_format=host.RESULT_PAIR if pair else host.RESULT_FULL) as b:
        got = b.ctx.submit_reads(p, b.ref, b.rd, rdt)
        b.ctx.wait_ticket(b.ctx.last_ticket)
        ptr = b.ctx.submit_ref(p, b.ref, rft)
        b.ctx.wait()
        assert got.tobytes() == ptr.tobytes()
        if pair:
            w = want[variant]
            for f in host.PAIR.names:
                assert (got[f] == w[f]).all(), f
        else:
            from test_gpu_parity import assert_same
            assert_same(got, want[variant])


# ---- rescue ---------------------------------------------------------------------------------------------------------------------

def rescue_workload(host, pac):
    rng = np.random.default_rng(21)
    edges = set()
    for byte, slen in _kernel_ledger.ALIGN_CLASSES:
        top = slen * (16 if byte else 8)
        prev = max([s * (16 if b2 else 8) for b2, s in _kernel_ledger.ALIGN_CLASSES if b2 == byte and s < slen] or [0])
        edges |= {top, prev + 1}
    lens = sorted(edges) + [150, 0]
    reads, specs, rdm = [], [], []
    for ri, lm in enumerate(lens):
        strand0 = ri % 2
        rb, re = tm.window(rng, strand0, lm + 300 if lm else 400)
        base = tm.mate_in(rng, pac, rb, re, lm, 0, nrate=0.01 if ri % 3 == 0 else 0.0) if lm else np.zeros(0, np.uint8)
        reads.append(np.ascontiguousarray(base, dtype=np.uint8))
        for is_rev in (0, 1):                                       # the same read in several tasks: both orientations, both strands,
            for strand in (0, 1):                                   # the 8-bit and the 16-bit run
                for byte in (1, 0):
                    if strand == strand0:
                        wrb, wre = rb, re
                    else:
                        wrb, wre = 2 * L_PAC - re, 2 * L_PAC - rb
                    x = XSUBO | XSTART | 19 | (XBYTE if byte else 0)
                    rdm.append((ri, is_rev, wrb, wre, x, 19))
    # status 1: an empty window and a window that bridges l_pac, on a read that exists
    rdm += [(3, 0, 5000, 5000, XSUBO | XSTART | 19, 19), (3, 1, L_PAC - 100, L_PAC + 200, XSUBO | XSTART | 19, 19), (3, 0, 7000, 6990, XSTART | 19, 19)]
    rdt = np.zeros(len(rdm), dtype=host.RD_MTASK)
    for k, (ri, is_rev, wrb, wre, x, ms) in enumerate(rdm):
        rdt[k] = (ri, is_rev, wrb, wre, x, ms)
        specs.append(tm.task(reads[ri], is_rev, wrb, wre, xtra=x, min_score=ms))
    return reads, rdt, specs


def test_rescue_equals_the_pointer_form_and_the_restatement(host, oracle, pac):
    reads, rdt, specs = rescue_workload(host, pac)
    p = host.default_params()
    with Bound(host, pac, reads, device=0) as b:
        t, got = b.ctx.submit_matesw_reads(p, b.ref, b.rd, rdt)
        b.ctx.wait_ticket(t)
        mt, keep = tm.make_mtasks(host, specs)
        t, ptr = b.ctx.submit_matesw_ref(p, b.ref, mt)
        b.ctx.wait_ticket(t)
    assert got.tobytes() == ptr.tobytes()
    assert all((got["status"] == s).any() for s in (0, 1, 2))
    assert (got["status"][rdt["read"] == len(reads) - 1] == 1).all() and (got["status"][-3:] == 1).all()     # the empty read; the windows
    want = tm.expected(host, oracle, p, pac, specs)
    got_aln = np.stack([got["aln"][k] for k in mr.ALN], axis=1)
    assert (got_aln == want["aln"]).all(), np.nonzero((got_aln != want["aln"]).any(axis=1))[0][:5]
    for f in tm.FIELDS:
        assert (got[f] == want[f]).all(), f


# ---- CIGAR ----------------------------------------------------------------------------------------------------------------------

def cigar_workload(host, pac):
    """slices at every phase qb of their reads, of 1 / 16 / 17 / 150 bases, both strands; a slice of 1 100 bases of a long read;
    the no-gap shortcut; retries as in test_gpu_cigar_ref.py"""
    rng = np.random.default_rng(33)
    reads, rows, specs = [], [], []

    def add(slice_, qb, tail, rb, re, **kw):
        rd = np.concatenate([rng.integers(0, 5, qb).astype(np.uint8), slice_, rng.integers(0, 5, tail).astype(np.uint8)])
        reads.append(np.ascontiguousarray(rd, dtype=np.uint8))
        s = tc.spec(slice_, rb, re, **kw)
        rows.append((len(reads) - 1, qb, qb + len(slice_), s["w"], rb, re, s["w_cap"], s["min_score"], s["max_tries"], 0))
        specs.append(s)
    for qb in range(16):
        for lq in (1, 16, 17, 150):
            for strand in (0, 1):
                rlen = max(1, lq + int(rng.integers(-2, 3))) if lq > 1 else 1
                rb, re = tc.interval(rng, rlen, strand)
                add(tc.read_of(rng, pac, rb, re, lq, 0.03, 0.01, 0.02 if qb % 4 == 1 else 0.0), qb, (qb * 5) % 7, rb, re)
    for strand in (0, 1):
        rb, re = tc.interval(rng, 1105, strand)
        add(tc.read_of(rng, pac, rb, re, 1100, 0.02, 0.004), 100, 100, rb, re)                      # the LDS ring kernel's
        rb, re = tc.interval(rng, 150, strand)
        add(tc.read_of(rng, pac, rb, re, 150, 0.05, 0.0), 7, 0, rb, re, w=0)                          # no-gap shortcut
        add(tc.read_of(rng, pac, rb, re, 150, 0.2, 0.0), 9, 3, rb, re, w=0, w_cap=50, min_score=150, max_tries=3)
        rb = tc.interval(rng, 150, strand)[0]
        for steps, kw in (([6, 6, -12], dict(w=4, w_cap=64, min_score=1000, max_tries=3)), ([6, -6], dict(w=4, w_cap=64, min_score=1000, max_tries=3)),
                          ([6, -6], dict(w=1, w_cap=0, min_score=1000, max_tries=2))):
            q = tc.retry_read(rng, pac, rb, steps)
            if strand:
                q = q[::-1].copy()
            add(q, 13, 2, rb, rb + 150, **kw)
    # the same read named by two tasks with different slices; an empty slice (status 1)
    rows.append((rows[6][0], rows[6][1], rows[6][2], 100, rows[6][4], rows[6][5], 0, INT_MIN, 1, 0))
    specs.append(specs[6])
    rows.append((0, 0, 0, 100, 1000, 1100, 0, INT_MIN, 1, 0))
    specs.append(tc.spec(np.zeros(0, np.uint8), 1000, 1100))
    rdt = np.zeros(len(rows), dtype=host.RD_CTASK)
    for k, r in enumerate(rows):
        rdt[k] = r
    return reads, rdt, specs


def test_cigar_equals_the_pointer_form_and_the_restatement(host, oracle, pac):
    reads, rdt, specs = cigar_workload(host, pac)
    p = host.default_params()
    with Bound(host, pac, reads, device=0) as b:
        t, res, cig, md = b.ctx.submit_cigar_reads(p, b.ref, b.rd, rdt, max_cigar=64, max_md=2048)
        b.ctx.wait_ticket(t)
        ct, keep = tc.make_ctasks(host, specs)
        t2, res2, cig2, md2 = b.ctx.submit_cigar_ref(p, b.ref, ct, max_cigar=64, max_md=2048)
        b.ctx.wait_ticket(t2)
    assert same_cigar_outputs((res, cig, md), (res2, cig2, md2))
    assert {1, 2, 3} <= set(int(x) for x in res["tries"]) and (res["status"] == 1).any()
    mds = b.ctx.md_strings(res, md)
    want = tc.expected(oracle, p, pac, specs)
    for i, w in enumerate(want):
        r = res[i]
        assert int(r["status"]) == w["status"] and (int(r["tries"]), int(r["w"])) == (w["tries"], w["w"]), i
        if w["status"]:
            continue
        n = len(w["cigar"])
        assert (int(r["score"]), int(r["n_cigar"]), int(r["nm"])) == (w["score"], n, w["nm"]), i
        assert [(int(x) & 0xf, int(x) >> 4) for x in cig[i, :n]] == w["cigar"] and mds[i] == w["md"], i


# ---- pipeline -------------------------------------------------------------------------------------------------------------------

def pipeline_body(host, pac, both):
    """three blocks on devices = [0, 0]: block k's extension, block k-1's rescue and block k-2's CIGAR tickets in flight together
    while block k+1 is uploaded; every submit cut into >= 3 chunks; results equal the serial pointer-form calls"""
    small = bool(os.environ.get("BSW_F4_CIGAR_WORK"))
    # without the switches a chunk holds an eighth of the work target at the least (f4_chunk_work): 2^28 cells of rescue (150 x ~550
    # a task), 2^25 of CIGAR (71 band columns x 150 a task) -> at least three chunks need 9 800 windows and 9 500 alignments
    n_e, n_m, n_c = (1500, 600, 600) if small else (1500, 11000, 12000)
    rng = np.random.default_rng(55)
    p = host.default_params()
    blocks = []
    for k in range(3):
        reads, e_rd, e_pt, m_rd, m_sp, c_rd, c_sp = [], np.zeros(n_e, host.RD_TASK), np.zeros(n_e, host.REF_TASK), np.zeros(n_m, host.RD_MTASK), [], np.zeros(n_c, host.RD_CTASK), []
        rmax, sd = np.zeros(2, np.int64), np.zeros(1, host.SEED)
        for i in range(max(n_e, n_m, n_c)):
            L = 150 + (i % 3)
            x = int(rng.integers(400, L_PAC - 1000)) + (i % 2) * L_PAC
            r = both[x:x + L].copy()
            sub = np.nonzero(rng.random(L) < 0.03)[0]
            r[sub] = (r[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
            reads.append(r)
            if i < n_e:
                qb, ln = int(rng.integers(0, L - 30)), int(rng.integers(19, 30))
                sd[0] = (x + qb, qb, ln)
                host.lib().bsw_chain_window(p.ctypes.data, sd.ctypes.data, 1, L, L_PAC, rmax.ctypes.data)
                for t in (e_rd, e_pt):
                    t[i]["init_score"], t[i]["seed"], t[i]["rmax0"], t[i]["rmax1"], t[i]["tag"] = -1, sd[0], rmax[0], rmax[1], i
                e_rd[i]["read"], e_pt[i]["query"], e_pt[i]["l_query"] = i, r.ctypes.data, L
            lo = (x // L_PAC) * L_PAC
            if i < n_m:
                wb, we = max(lo, x - 200), min(lo + L_PAC, x + L + 200)
                m_rd[i] = (i, i % 2, wb, we, XSUBO | XSTART | 19 | (XBYTE if i % 3 else 0), 19)
                m_sp.append(tm.task(r, i % 2, wb, we, xtra=int(m_rd[i]["xtra"]), min_score=19))
            if i < n_c:
                qb = i % 16
                c_rd[i] = (i, qb, L - 2, 100, x + qb, x + L - 2, 0, INT_MIN, 1, 0)
                c_sp.append(tc.spec(r[qb:L - 2], x + qb, x + L - 2))
        blocks.append((reads, e_rd, e_pt, m_rd, m_sp, c_rd, c_sp))
    with host.BswContext(devices=[0, 0], chunk_tasks=512) as c:
        ref = c.ref_upload(pac, L_PAC)
        try:
            # serial pointer-form calls
            want = []
            for reads, e_rd, e_pt, m_rd, m_sp, c_rd, c_sp in blocks:
                we = c.submit_ref(p, ref, e_pt)
                c.wait()
                mt, k1 = tm.make_mtasks(host, m_sp)
                t, wm = c.submit_matesw_ref(p, ref, mt)
                c.wait_ticket(t)
                ct, k2 = tc.make_ctasks(host, c_sp)
                t, wc, wcig, wmd = c.submit_cigar_ref(p, ref, ct)
                c.wait_ticket(t)
                want.append((we.copy(), wm.copy(), wc.copy(), wcig.copy(), wmd.copy()))
            # the pipeline: stage s of block k runs in round k + s
            rd = [c.reads_upload(blocks[0][0]), None, None]
            got = [[None] * 3 for _ in range(3)]
            for rnd in range(5):
                base = c.host_stats()["chunks"]
                tickets = []
                for s in range(3):
                    k = rnd - s
                    if not 0 <= k < 3:
                        continue
                    reads, e_rd, e_pt, m_rd, m_sp, c_rd, c_sp = blocks[k]
                    if s == 0:
                        got[k][0] = c.submit_reads(p, ref, rd[k], e_rd)
                        tickets.append(c.last_ticket)
                    elif s == 1:
                        t, got[k][1] = c.submit_matesw_reads(p, ref, rd[k], m_rd)
                        tickets.append(t)
                    else:
                        t, r_, cg, md = c.submit_cigar_reads(p, ref, rd[k], c_rd)
                        got[k][2] = (r_, cg, md)
                        tickets.append(t)
                assert c.inflight() == len(tickets)
                if rnd + 1 < 3:
                    rd[rnd + 1] = c.reads_upload(blocks[rnd + 1][0])         # the next block, while this round's tickets are in flight
                if rnd < 3:
                    with pytest.raises(host.BswError) as e:
                        c.reads_free(rd[rnd])
                    assert e.value.code == -6
                for t in tickets:
                    c.wait_ticket(t)
                assert c.host_stats()["chunks"] - base >= 3 * len(tickets)
                if rnd >= 2:
                    c.reads_free(rd[rnd - 2])                                # its last ticket has been collected
            for k in range(3):
                we, wm, wc, wcig, wmd = want[k]
                assert got[k][0].tobytes() == we.tobytes(), k
                assert got[k][1].tobytes() == wm.tobytes(), k
                assert same_cigar_outputs(got[k][2], (wc, wcig, wmd)), k
        finally:
            c.ref_free(ref)


def test_pipeline_of_three_blocks(host, pac, both):
    pipeline_body(host, pac, both)


def test_pipeline_with_the_chunk_work_switches_in_a_child_process():
    """BSW_F4_CIGAR_WORK / BSW_F4_MATESW_WORK are read once per process: the same pipeline with small submits cut by the switches"""
    env = dict(os.environ, BSW_F4_CIGAR_WORK="3000000", BSW_F4_MATESW_WORK="12000000")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(here, "test_gpu_reads.py") + "::test_pipeline_of_three_blocks"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout


# ---- errors: return codes only --------------------------------------------------------------------------------------------------

def test_errors_are_refused_before_anything_is_queued(host, pac, both):
    p = host.default_params()
    reads = [both[1000:1150].copy(), both[5000:5100].copy(), both[9000:9000 + 8300].copy()]
    with Bound(host, pac, reads, device=0) as b, host.BswContext(device=0) as other:
        c, ref, rd = b.ctx, b.ref, b.rd
        assert c.reads_info(rd)["n_reads"] == 3 and c.reads_info(rd)["bases"] == 150 + 100 + 8300
        foreign = other.reads_upload(reads)

        def code(fn, *a, **kw):
            try:
                fn(*a, **kw)
            except host.BswError as e:
                assert c.inflight() == 0
                return e.code
            c.wait()
            return 0
        e = np.zeros(2, host.RD_TASK)
        e["init_score"], e["rmax0"], e["rmax1"] = -1, 900, 1300
        e["seed"]["rbeg"], e["seed"]["qbeg"], e["seed"]["len"] = 1050, 50, 20
        assert code(c.submit_reads, p, ref, rd, e) == 0
        for field, value, want in (("read", 3, -2), ("read", 0xffffffff, -2)):
            bad = e.copy()
            bad[field][1] = value
            assert code(c.submit_reads, p, ref, rd, bad) == want
        bad = e.copy(); bad["seed"]["qbeg"][1] = 140                        # the seed leaves its read
        assert code(c.submit_reads, p, ref, rd, bad) == -2
        bad = e.copy(); bad["rmax0"][1], bad["rmax1"][1] = L_PAC - 5, L_PAC + 5   # the window bridges the strands
        assert code(c.submit_reads, p, ref, rd, bad) == -2
        bad = e.copy(); bad["read"][1] = 2; bad["seed"]["qbeg"][1] = 8192; bad["seed"]["rbeg"][1] = 9000 + 8192   # a left flank beyond BSW_MAX_QLEN
        bad["rmax0"][1], bad["rmax1"][1] = 9000, 9000 + 8300
        assert code(c.submit_reads, p, ref, rd, bad) == -3
        assert code(c.submit_reads, p, ref, foreign, e) == -2
        m = np.zeros(2, host.RD_MTASK)
        m["rb"], m["re"], m["xtra"], m["min_score"] = 900, 1400, XSUBO | XSTART | 19, 19
        assert code(c.submit_matesw_reads, p, ref, rd, m) == 0
        bad = m.copy(); bad["read"][1] = 3
        assert code(c.submit_matesw_reads, p, ref, rd, bad) == -2
        bad = m.copy(); bad["is_rev"][1] = 2
        assert code(c.submit_matesw_reads, p, ref, rd, bad) == -2
        bad = m.copy(); bad["read"][1] = 2                                   # 8 300 bases > BSW_ALIGN_MAX_QLEN
        assert code(c.submit_matesw_reads, p, ref, rd, bad) == -3
        bad = m.copy(); bad["re"][1] = 900 + 65536
        assert code(c.submit_matesw_reads, p, ref, rd, bad) == -3
        assert code(c.submit_matesw_reads, p, ref, foreign, m) == -2
        g = np.zeros(2, host.RD_CTASK)
        g["qb"], g["qe"], g["w"], g["rb"], g["re"], g["min_score"], g["max_tries"] = 10, 90, 50, 1010, 1090, INT_MIN, 1
        assert code(c.submit_cigar_reads, p, ref, rd, g) == 0
        for field, value, want in (("read", 3, -2), ("qb", -1, -2), ("qe", 9, -2), ("qe", 151, -2), ("max_tries", 4, -2), ("w", 70000, -3)):
            bad = g.copy()
            bad[field][1] = value
            assert code(c.submit_cigar_reads, p, ref, rd, bad) == want, field
        bad = g.copy(); bad["read"][1], bad["qb"][1], bad["qe"][1] = 2, 0, 8192     # a slice beyond BSW_GLOBAL_MAX_QLEN
        assert code(c.submit_cigar_reads, p, ref, rd, bad) == -3
        assert code(c.submit_cigar_reads, p, ref, foreign, g) == -2
        # free while in flight
        t, res = c.submit_matesw_reads(p, ref, rd, m)
        with pytest.raises(host.BswError) as ex:
            c.reads_free(rd)
        assert ex.value.code == -6
        c.wait_ticket(t)
        with pytest.raises(host.BswError) as ex:
            other.reads_free(rd)
        assert ex.value.code == -2
        other.reads_free(foreign)
        # upload's own limits
        with pytest.raises(host.BswError) as ex:
            c.reads_upload([np.zeros(65536, np.uint8)])
        assert ex.value.code == -3
        empty = c.reads_upload([])
        c.reads_free(empty)
