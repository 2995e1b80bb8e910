"""The asynchronous read-block upload on the GPU: bsw_reads_upload_start sends the reads across as they lie, bsw_reads_pack_kernel
packs them on the device, and tickets that name the block are ordered behind that on the GPU.

The device image (bsw_reads_image, slack words included) is compared word for word with the image bsw_reads_upload makes of the
same reads; the three *_reads_* tickets submitted right behind the start, without waiting, are compared byte for byte with the
pointer forms on the same bytes.  Every test runs on context [0] and on [0, 0] (two copies on the one card)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _gencigar_ref as gc
import test_gpu_cigar_ref as tc
import test_gpu_matesw_ref as tm
from test_gpu_reads import INT_MIN, L_PAC, XBYTE, XSTART, XSUBO, same_cigar_outputs

pytestmark = pytest.mark.gpu

DEVS = [[0], [0, 0]]
IMAGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 149, 150, 151, 250, 4101, 65535]


@pytest.fixture(scope="module")
def pac():
    rng = np.random.default_rng(4711)
    return gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))


@pytest.fixture(scope="module")
def both(pac):
    g = gc.unpack_pac(pac, L_PAC)
    return np.concatenate([g, 3 - g[::-1]]).astype(np.uint8)


# ---- 4. the image ---------------------------------------------------------------------------------------------------------------

def image_layout():
    """(lens, offsets): reads laid into one arena, a zero-length read first, in the middle and last; the reads with bases start at
    every byte phase 0 - 15 of the arena (the direct path's raw offsets) AND at every phase of the running sum of the lengths
    (the gather path's)"""
    rng = np.random.default_rng(77)
    lens = [0]
    for rep in range(4):
        part = [n for n in IMAGE_LENS if n != 65535 or rep == 0]
        rng.shuffle(part)
        lens += part
        if rep == 1:
            lens += [0, 0]
    tail = len(lens)
    lens += [17] * 16 + [150, 7, 3, 11, 0]                            # sixteen reads of 17 back to back: every phase, whatever came before
    offs, off = [], 0
    for i, n in enumerate(lens):
        offs.append(off)
        off += n + ((i * 7) % 5 if i < tail else 0)
    return np.array(lens, dtype=np.int32), np.array(offs, dtype=np.int64), off


def image_bytes(total):
    rng = np.random.default_rng(78)
    b = rng.integers(0, 5, total).astype(np.uint8)
    odd = rng.random(total) < 0.03
    b[odd] = rng.integers(5, 256, int(odd.sum())).astype(np.uint8)      # stored as 4
    return b


def test_image_layout_covers_what_it_claims():
    lens, offs, total = image_layout()
    has = lens > 0
    assert set(lens.tolist()) >= set(IMAGE_LENS)
    assert lens[0] == 0 and lens[-1] == 0 and (lens[5:-5] == 0).any()
    assert set((offs[has] & 15).tolist()) == set(range(16))                          # direct: offsets into the arena's span
    cum = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert set((cum[has] & 15).tolist()) == set(range(16))                           # gather: the reads back to back
    b = image_bytes(total)
    assert (b > 4).sum() > 100 and set(range(5)) <= set(b.tolist())


def start_raw(host, ctx, ptrs, lens):
    h = C.c_void_p()
    rc = host.lib().bsw_reads_upload_start(ctx.handle, ptrs.ctypes.data, lens.ctypes.data, len(lens), C.byref(h))
    return rc, h


def images_of(host, ctx, ndev, ptrs, lens, reads):
    """(image per device of the asynchronous upload, image of bsw_reads_upload) for reads at ptrs[] / lens[]"""
    rc, rd = start_raw(host, ctx, ptrs, lens)
    assert rc == 0, host.lib().bsw_last_error(ctx.handle).decode()
    ctx.reads_wait(rd)
    assert ctx.reads_test(rd) is True
    ctx.reads_wait(rd)                                                    # may be called again
    got = [ctx.reads_image(rd, k) for k in range(ndev)]
    info = ctx.reads_info(rd)
    ctx.reads_free(rd)
    ref = ctx.reads_upload(reads)
    assert ctx.reads_test(ref) is True and ctx.reads_info(ref) == info
    want = ctx.reads_image(ref, 0)
    ctx.reads_free(ref)
    return got, want


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_image_equals_the_synchronous_uploads(host, devs):
    lens, offs, total = image_layout()
    src = image_bytes(total)
    arena = host.HostArena(total + 64)
    try:
        arena.u8[:total] = src
        reads = [src[o:o + n] for o, n in zip(offs, lens)]
        with host.BswContext(devices=devs) as ctx:
            # the direct path: one DMA of the arena's span
            ptrs = np.array([arena.ptr + int(o) if n else 0 for o, n in zip(offs, lens)], dtype=np.uint64)
            got, want = images_of(host, ctx, len(devs), ptrs, lens, reads)
            assert len(want) == sum((int(n) + 15) // 16 for n in lens) + 4 and not want[:2].any() and not want[-2:].any()
            for k, g in enumerate(got):
                assert (g == want).all(), ("direct", k, np.nonzero(g != want)[0][:5])
            # the gather path: every read an array of its own in pageable memory
            own = [r.copy() for r in reads]
            ptrs = np.array([r.ctypes.data if len(r) else 0 for r in own], dtype=np.uint64)
            got, _ = images_of(host, ctx, len(devs), ptrs, lens, reads)
            for k, g in enumerate(got):
                assert (g == want).all(), ("gather", k, np.nonzero(g != want)[0][:5])
            # the empty block and a block of one read
            for one in ([], [src[3:3 + 150]], [src[:0]]):
                ptrs = np.array([r.ctypes.data if len(r) else 0 for r in one], dtype=np.uint64)
                ln = np.array([len(r) for r in one], dtype=np.int32)
                rc, rd = start_raw(host, ctx, ptrs, ln)
                assert rc == 0
                if not sum(len(r) for r in one):
                    assert ctx.reads_test(rd) is True                 # ready at once
                ctx.reads_wait(rd)
                a = ctx.reads_image(rd, len(devs) - 1)
                ctx.reads_free(rd)
                ref = ctx.reads_upload(one)
                b = ctx.reads_image(ref, 0)
                ctx.reads_free(ref)
                assert len(a) == len(b) and (a == b).all()
            assert ctx.inflight() == 0
    finally:
        arena.free()


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------

N_READS, N_EXT, N_M, N_C = 4096, 8192, 2048, 2048


class Work:
    """4 096 reads of 150 bases in one array; 8 192 seeds, 2 048 rescue windows and 2 048 CIGAR tasks on them, by read index and
    as the pointer forms' records on the same bytes"""

    def __init__(self, host, pac, both, n_reads=N_READS, n_e=N_EXT, n_m=N_M, n_c=N_C, seed=101):
        rng = np.random.default_rng(seed)
        p = host.default_params()
        L = 150
        self.flat = np.zeros(n_reads * L, dtype=np.uint8)
        x = rng.integers(400, L_PAC - 1000, n_reads) + (np.arange(n_reads) % 2) * L_PAC
        for i in range(n_reads):
            r = both[x[i]:x[i] + L].copy()
            sub = np.nonzero(rng.random(L) < 0.03)[0]
            r[sub] = (r[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
            if i % 37 == 0:
                r[int(rng.integers(0, L))] = 4
            self.flat[i * L:(i + 1) * L] = r
        self.reads = [self.flat[i * L:(i + 1) * L] for i in range(n_reads)]
        self.ptrs = np.array([r.ctypes.data for r in self.reads], dtype=np.uint64)
        self.lens = np.full(n_reads, L, dtype=np.int32)
        self.e_rd, self.e_pt = np.zeros(n_e, host.RD_TASK), np.zeros(n_e, host.REF_TASK)
        rmax, sd = np.zeros(2, np.int64), np.zeros(1, host.SEED)
        for k in range(n_e):
            i = k % n_reads
            qb, ln = int(rng.integers(0, L - 30)), int(rng.integers(19, 30))
            sd[0] = (x[i] + qb, qb, ln)
            host.lib().bsw_chain_window(p.ctypes.data, sd.ctypes.data, 1, L, L_PAC, rmax.ctypes.data)
            for t in (self.e_rd, self.e_pt):
                t[k]["init_score"], t[k]["seed"], t[k]["rmax0"], t[k]["rmax1"], t[k]["tag"] = -1, sd[0], rmax[0], rmax[1], k
            self.e_rd[k]["read"], self.e_pt[k]["query"], self.e_pt[k]["l_query"] = i, self.ptrs[i], L
        self.m_rd, m_sp = np.zeros(n_m, host.RD_MTASK), []
        for k in range(n_m):
            i = (k * 2 + 1) % n_reads
            lo = (int(x[i]) // L_PAC) * L_PAC
            wb, we = max(lo, int(x[i]) - 200), min(lo + L_PAC, int(x[i]) + L + 200)
            self.m_rd[k] = (i, k % 2, wb, we, XSUBO | XSTART | 19 | (XBYTE if k % 3 else 0), 19)
            m_sp.append(tm.task(self.reads[i], k % 2, wb, we, xtra=int(self.m_rd[k]["xtra"]), min_score=19))
        self.m_pt, self.keep_m = tm.make_mtasks(host, m_sp)
        self.c_rd, c_sp = np.zeros(n_c, host.RD_CTASK), []
        for k in range(n_c):
            i = (k * 2) % n_reads
            qb = k % 16
            self.c_rd[k] = (i, qb, L - 2, 100, x[i] + qb, x[i] + L - 2, 0, INT_MIN, 1, 0)
            c_sp.append(tc.spec(self.reads[i][qb:L - 2], x[i] + qb, x[i] + L - 2))
        self.c_pt, self.keep_c = tc.make_ctasks(host, c_sp)
        self.want = None

    def pointer_forms(self, host, ctx, ref):
        """the reference, computed once and left unchanged"""
        if self.want is None:
            p = host.default_params()
            we = ctx.submit_ref(p, ref, self.e_pt)
            ctx.wait()
            t, wm = ctx.submit_matesw_ref(p, ref, self.m_pt)
            ctx.wait_ticket(t)
            t, wc, wcig, wmd = ctx.submit_cigar_ref(p, ref, self.c_pt)
            ctx.wait_ticket(t)
            self.want = (we.copy(), wm.copy(), (wc.copy(), wcig.copy(), wmd.copy()))
        return self.want

    def submit_all(self, host, ctx, ref, rd):
        p = host.default_params()
        e = ctx.submit_reads(p, ref, rd, self.e_rd)
        te = ctx.last_ticket
        tm_, m = ctx.submit_matesw_reads(p, ref, rd, self.m_rd)
        tc_, r, cg, md = ctx.submit_cigar_reads(p, ref, rd, self.c_rd)
        return [te, tm_, tc_], (e, m, (r, cg, md))

    def check(self, got, want):
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
        assert same_cigar_outputs(got[2], want[2])


@pytest.fixture(scope="module")
def work(host, pac, both):
    return Work(host, pac, both)


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_tickets_submitted_behind_the_start_see_the_whole_block(host, pac, work, devs):
    with bound(host, pac, devs) as (ctx, ref):
        want = work.pointer_forms(host, ctx, ref)
        assert (want[1]["status"] == 0).any() and (want[2][0]["status"] == 0).all()
        h2d0 = ctx.host_stats()["h2d_bytes"]
        rc, rd = start_raw(host, ctx, work.ptrs, work.lens)
        assert rc == 0, host.lib().bsw_last_error(ctx.handle).decode()
        tickets, got = work.submit_all(host, ctx, ref, rd)            # no wait in between
        assert ctx.inflight() == 3                                    # the upload is no submit
        for t in tickets:
            ctx.wait_ticket(t)
        ctx.reads_wait(rd)
        work.check(got, want)
        # the raw bytes and a 16-byte record per read crossed once per device
        assert ctx.host_stats()["h2d_bytes"] - h2d0 >= len(devs) * (N_READS * 150 + N_READS * 16)
        ctx.reads_free(rd)


def test_image_and_ordering_with_several_pieces_per_device_in_a_child_process():
    """BSW_READS_UP_BYTES is for tests and measurements: 64 KiB pieces cut the ordering test's block of 614 400 bytes into ten
    pieces per device and the image test's into at least four"""
    env = dict(os.environ, BSW_READS_UP_BYTES="65536")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(here, "test_gpu_reads_async.py"),
                        "-k", "test_image_equals or test_tickets_submitted"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout


# ---- 6. three blocks in a pipeline ---------------------------------------------------------------------------------------------

class bound:
    """a context with the reference on it; nothing is left in flight when the reference goes, whatever the test did"""
    def __init__(self, host, pac, devs, **kw):
        self.ctx = host.BswContext(devices=devs, **kw)
        self.ref = self.ctx.ref_upload(pac, L_PAC)

    def __enter__(self):
        return self.ctx, self.ref

    def __exit__(self, *a):
        try:
            self.ctx.wait()
        except Exception:
            pass
        self.ctx.ref_free(self.ref)
        self.ctx.close()                                              # (waits for uploads in flight)


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_pipeline_of_three_blocks(host, pac, both, devs):
    blocks = [Work(host, pac, both, n_reads=1024, n_e=2048, n_m=512, n_c=512, seed=200 + k) for k in range(3)]
    with bound(host, pac, devs, chunk_tasks=512) as (ctx, ref):
        want = [b.pointer_forms(host, ctx, ref) for b in blocks]
        rd = [None] * 3
        rc, rd[0] = start_raw(host, ctx, blocks[0].ptrs, blocks[0].lens)
        assert rc == 0
        for k in range(3):
            tickets, got = blocks[k].submit_all(host, ctx, ref, rd[k])
            if k + 1 < 3:                                             # block k + 1 goes up beside block k's tickets
                rc, rd[k + 1] = start_raw(host, ctx, blocks[k + 1].ptrs, blocks[k + 1].lens)
                assert rc == 0 and ctx.inflight() == 3
            with pytest.raises(host.BswError) as e:                   # its tickets (and maybe its upload) are in flight
                ctx.reads_free(rd[k])
            assert e.value.code == -6
            for t in tickets:
                ctx.wait_ticket(t)
            blocks[k].check(got, want[k])
            ctx.reads_wait(rd[k])
            ctx.reads_free(rd[k])                                     # collected: the block goes


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_third_concurrent_upload_is_busy_and_changes_nothing(host, pac, work, devs):
    """Two uploads queue behind the three tickets of a resident block (every job of the devices' queues ahead of them waits for
    the GPU), a third start follows at once.  How long the two stay in flight is the machine's business: the round is repeated
    until the third start met both of them, eight times at the most."""
    tiny = np.zeros(150, dtype=np.uint8)
    tptr, tlen = np.array([tiny.ctypes.data], dtype=np.uint64), np.array([150], dtype=np.int32)
    with bound(host, pac, devs) as (ctx, ref):
        want = work.pointer_forms(host, ctx, ref)
        front = ctx.reads_upload(work.reads)
        seen = False
        for attempt in range(8):
            tickets, got = work.submit_all(host, ctx, ref, front)
            rc1, a = start_raw(host, ctx, work.ptrs, work.lens)
            rc2, b = start_raw(host, ctx, work.ptrs, work.lens)
            rc3, c = start_raw(host, ctx, tptr, tlen)
            text = host.lib().bsw_last_error(ctx.handle)
            infl = ctx.inflight()
            for t in tickets:
                ctx.wait_ticket(t)
            assert rc1 == 0 and rc2 == 0 and rc3 in (0, -6) and infl == 3
            for h in (a, b) + ((c,) if rc3 == 0 else ()):
                ctx.reads_wait(h)
                ctx.reads_free(h)
            work.check(got, want)
            if rc3 == -6:
                assert not c.value and b"uploads in flight" in text
                seen = True
                break
        assert seen, "eight rounds and the third start never met two uploads in flight"
        rc, again = start_raw(host, ctx, tptr, tlen)                  # the two places are free again
        assert rc == 0
        ctx.reads_wait(again)
        ctx.reads_free(again)
        ctx.reads_free(front)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_refusals_equal_the_synchronous_uploads_and_queue_nothing(host, devs):
    L = host.lib()
    r = np.zeros(200, dtype=np.uint8)
    with host.BswContext(devices=devs) as ctx:
        # a first upload starts the slot threads, so that bsw_host_stats has something to keep unchanged
        rc, rd = start_raw(host, ctx, np.array([r.ctypes.data], dtype=np.uint64), np.array([150], dtype=np.int32))
        assert rc == 0
        ctx.reads_wait(rd)
        ctx.reads_free(rd)
        def counted():                                                # (the CPU times of the slot threads are not counts)
            st = ctx.host_stats()
            return {k: st[k] for k in ("h2d_bytes", "d2h_bytes", "chunks", "submits", "seeds")}
        stats = counted()
        assert stats["h2d_bytes"] > 0
        big = np.full(66000, 65535, dtype=np.int32)                   # 66 000 x 4 096 words > 2^28 - 2^13
        cases = [
            (np.array([r.ctypes.data, 0], dtype=np.uint64), np.array([10, 5], dtype=np.int32), 2, -2),           # a NULL read of 5 bases
            (np.array([r.ctypes.data, r.ctypes.data], dtype=np.uint64), np.array([10, -1], dtype=np.int32), 2, -2),
            (np.array([r.ctypes.data], dtype=np.uint64), np.array([65536], dtype=np.int32), 1, -3),
            (np.full(66000, r.ctypes.data, dtype=np.uint64), big, 66000, -3),
            (np.array([r.ctypes.data], dtype=np.uint64), np.array([10], dtype=np.int32), 1 << 32, -3),
        ]
        for ptrs, lens, n, want in cases:
            for fn in (L.bsw_reads_upload, L.bsw_reads_upload_start):
                h = C.c_void_p(0xdead)
                assert fn(ctx.handle, ptrs.ctypes.data, lens.ctypes.data, n, C.byref(h)) == want, (fn.__name__, n, want)
                assert not h.value
        for fn in (L.bsw_reads_upload, L.bsw_reads_upload_start):
            h = C.c_void_p()
            assert fn(ctx.handle, None, None, 1, C.byref(h)) == -2 and not h.value
            assert fn(ctx.handle, cases[0][0].ctypes.data, None, 1, C.byref(h)) == -2
            assert fn(ctx.handle, cases[0][0].ctypes.data, cases[0][1].ctypes.data, 1, None) == -2
            assert fn(None, cases[0][0].ctypes.data, cases[0][1].ctypes.data, 1, C.byref(h)) == -2
        assert counted() == stats and ctx.inflight() == 0
        # the image of a block that is not this context's, or into too small a buffer
        rc, rd = start_raw(host, ctx, np.array([r.ctypes.data], dtype=np.uint64), np.array([150], dtype=np.int32))
        ctx.reads_wait(rd)
        out = np.zeros(4, dtype=np.uint64)
        assert L.bsw_reads_image(ctx.handle, rd, 0, out.ctypes.data, 4) == -2
        assert L.bsw_reads_image(ctx.handle, rd, len(devs), out.ctypes.data, 4) == -2
        ctx.reads_free(rd)
