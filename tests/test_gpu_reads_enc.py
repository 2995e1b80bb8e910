"""The upload encodings of a resident read block on the GPU: bsw_reads_upload_enc / bsw_reads_upload_start_enc take the reads as
codes, as FASTQ letters (BSW_READS_ASCII) or as 4-bit words (BSW_READS_PACKED), and the store is the same image whatever the
encoding.

The device image (bsw_reads_image, slack words included) of every encoding, on the direct path (one registered arena) and on the
gather path (one pageable array per read), on context [0] and on [0, 0], is compared word for word with the image bsw_reads_upload
makes of the codes the input spells.  The three *_reads_* tickets submitted right behind a start with letters and with words are
compared byte for byte with the same submits on a block of bsw_reads_upload.

An upload has ONE encoding, so reads of different encodings in one kernel launch cannot happen through the API: the kernel's
per-record `enc` with mixed records is covered by the CPU model (tests/test_reads_pack_enc_model.py calls the word function per
read) and by the host double's stand-in launcher (tests/test_reads_enc_double_cpu.py), not here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_reads_async import Work, bound, both, pac  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEVS = [[0], [0, 0]]
CODES, ASCII, PACKED = 0, 1, 2
ENCS = [CODES, ASCII, PACKED]
ENC_IDS = ["codes", "letters", "words"]
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 150, 250, 255, 256, 257, 513, 1000]
LUT = np.full(256, 4, dtype=np.uint8)
for _c, _s in enumerate("ACGT"):
    LUT[ord(_s)] = LUT[ord(_s.lower())] = _c


# ---- the block ----------------------------------------------------------------------------------------------------------------

def layout():
    """lens: zero-length reads first, in the middle and last; the lengths four times, shuffled; sixteen reads of 17 bases (one word
    and a base: an odd number of words) back to back, so that the reads start at every byte phase and at both word parities
    whatever came before.  gaps[i]: unused units behind read i in the arena."""
    rng = np.random.default_rng(177)
    lens = [0]
    for rep in range(4):
        part = list(LENS[1:])
        rng.shuffle(part)
        lens += part
        if rep == 0:
            lens += [0, 0]
    tail = len(lens)
    lens += [17] * 16 + [150, 7, 3, 11, 0]
    gaps = [(i * 7) % 5 if i < tail else 0 for i in range(len(lens))]
    return np.array(lens, dtype=np.int32), gaps


class Block:
    """one encoding of the layout: an arena image (`flat`, of `unit`-byte elements), where every read lies in it, and the codes it spells"""

    def __init__(self, enc):
        self.enc = enc
        self.lens, gaps = layout()
        rng = np.random.default_rng(178 + enc)
        if enc == PACKED:
            self.unit, dtype = 8, np.uint64
            size = [(int(n) + 15) // 16 for n in self.lens]
        else:
            self.unit, dtype = 1, np.uint8
            size = [int(n) for n in self.lens]
        offs, off = [], 3                                                   # (garbage in front of the first read)
        for s, g in zip(size, gaps):
            offs.append(off)
            off += s + g
        self.offs, self.size, total = offs, size, off + 2
        if enc == CODES:
            flat = rng.integers(0, 5, total).astype(np.uint8)
            odd = rng.random(total) < 0.03
            flat[odd] = rng.integers(5, 256, int(odd.sum())).astype(np.uint8)
            spelt = np.minimum(flat, 4)
        elif enc == ASCII:
            flat = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)[rng.integers(0, 10, total)].copy()
            odd = rng.random(total) < 0.05
            flat[odd] = rng.integers(0, 256, int(odd.sum())).astype(np.uint8)
            at = offs[int(np.nonzero(self.lens == 1000)[0][0])]
            flat[at + 100:at + 356] = rng.permutation(256).astype(np.uint8)   # every byte value, inside a read
            spelt = LUT[flat]
        else:
            nib = rng.integers(0, 5, total * 16).astype(np.uint8)
            odd = rng.random(total * 16) < 0.05
            nib[odd] = rng.integers(0, 16, int(odd.sum())).astype(np.uint8)
            at = 16 * offs[int(np.nonzero(self.lens == 1000)[0][0])]
            nib[at + 64:at + 80] = rng.permutation(16).astype(np.uint8)       # every nibble value, inside a read
            for o, n in zip(offs, self.lens):                                 # non-zero garbage behind every read's last base
                end = 16 * (o + (int(n) + 15) // 16)
                nib[16 * o + int(n):end] = rng.integers(5, 16, end - 16 * o - int(n)).astype(np.uint8)
            flat = (nib.reshape(-1, 16).astype(np.uint64) << (4 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint64)
            spelt = np.minimum(nib, 4)
        self.flat = flat.astype(dtype)
        per = 16 if enc == PACKED else 1
        self.codes = [spelt[per * o:per * o + int(n)].copy() for o, n in zip(offs, self.lens)]
        self.seen = np.unique(np.concatenate([(nib if enc == PACKED else flat)[per * o:per * o + int(n)] for o, n in zip(offs, self.lens)]))

    def pointers(self, base):
        """the reads inside a copy of `flat` at address base"""
        return np.array([base + self.unit * o if n else 0 for o, n in zip(self.offs, self.lens)], dtype=np.uint64)

    def own(self):
        """every read an array of its own in pageable memory (garbage nibbles included)"""
        arrs = [self.flat[o:o + s].copy() for o, s in zip(self.offs, self.size)]
        return arrs, np.array([a.ctypes.data if n else 0 for a, n in zip(arrs, self.lens)], dtype=np.uint64)


@pytest.fixture(scope="module")
def blocks():
    return {enc: Block(enc) for enc in ENCS}


def test_layout_covers_what_it_claims(blocks):
    lens, _ = layout()
    has = lens > 0
    assert set(lens.tolist()) == set(LENS) | {7, 3, 11} and lens.sum() < 100000
    assert lens[0] == 0 and lens[-1] == 0 and (lens[5:-5] == 0).any()
    for enc in (CODES, ASCII):
        b = blocks[enc]
        assert set((np.array(b.offs)[has] & 15).tolist()) == set(range(16))              # direct: offsets into the arena's span
        cum = np.concatenate([[0], np.cumsum(lens)[:-1]])
        assert set((cum[has] & 15).tolist()) == set(range(16))                           # gather: the reads back to back
    b = blocks[PACKED]
    assert set((np.array(b.offs)[has] & 1).tolist()) == {0, 1}                           # both halves of a 16-byte line
    cum = np.concatenate([[0], np.cumsum(b.size)[:-1]])
    assert set((cum[has] & 1).tolist()) == {0, 1}
    assert len(blocks[ASCII].seen) == 256 and len(blocks[PACKED].seen) == 16 and blocks[CODES].seen.max() > 4
    for o, n in zip(b.offs, lens):                                                       # garbage behind every packed read that has a tail
        if n & 15:
            assert int(b.flat[o + (n + 15) // 16 - 1]) >> (4 * (int(n) & 15)) != 0
    assert all((c <= 4).all() for e in ENCS for c in blocks[e].codes)


def start_enc(host, ctx, ptrs, lens, enc):
    h = C.c_void_p(0xdead)
    rc = host.lib().bsw_reads_upload_start_enc(ctx.handle, ptrs.ctypes.data, lens.ctypes.data, len(lens), enc, C.byref(h))
    return rc, h


def sync_enc(host, ctx, ptrs, lens, enc):
    h = C.c_void_p(0xdead)
    rc = host.lib().bsw_reads_upload_enc(ctx.handle, ptrs.ctypes.data, lens.ctypes.data, len(lens), enc, C.byref(h))
    return rc, h


def check_images(host, ctx, ndev, ptrs, blk, want, what):
    """the asynchronous and the synchronous upload of the reads at ptrs[], every device's copy, against `want`"""
    h2d0 = ctx.host_stats()["h2d_bytes"]
    rc, rd = start_enc(host, ctx, ptrs, blk.lens, blk.enc)
    assert rc == 0, host.lib().bsw_last_error(ctx.handle).decode()
    ctx.reads_wait(rd)
    assert ctx.reads_test(rd) is True
    grew = ctx.host_stats()["h2d_bytes"] - h2d0
    for k in range(ndev):
        g = ctx.reads_image(rd, k)
        assert len(g) == len(want) and (g == want).all(), (what, "start", k, np.nonzero(g != want)[0][:5])
    ctx.reads_free(rd)
    rc, rd = sync_enc(host, ctx, ptrs, blk.lens, blk.enc)
    assert rc == 0, host.lib().bsw_last_error(ctx.handle).decode()
    for k in range(ndev):
        g = ctx.reads_image(rd, k)
        assert len(g) == len(want) and (g == want).all(), (what, "synchronous", k, np.nonzero(g != want)[0][:5])
    ctx.reads_free(rd)
    return grew


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
@pytest.mark.parametrize("enc", ENCS, ids=ENC_IDS)
def test_image_equals_the_upload_of_the_codes(host, blocks, enc, devs):
    blk = blocks[enc]
    arena = host.HostArena(blk.flat.nbytes + 64)
    try:
        arena.u8[:blk.flat.nbytes] = blk.flat.view(np.uint8)
        with host.BswContext(devices=devs) as ctx:
            ref = ctx.reads_upload(blk.codes)
            want = ctx.reads_image(ref, 0)
            ctx.reads_free(ref)
            assert len(want) == sum((int(n) + 15) // 16 for n in blk.lens) + 4 and not want[:2].any() and not want[-2:].any()
            # the direct path: one DMA of the arena's span
            check_images(host, ctx, len(devs), blk.pointers(arena.ptr), blk, want, "direct")
            # the gather path: raw bytes + a 16-byte record per read, once per device
            keep, ptrs = blk.own()
            grew = check_images(host, ctx, len(devs), ptrs, blk, want, "gather")
            raw = sum(blk.size) * blk.unit
            assert grew == len(devs) * (raw + 16 * len(blk.lens)), (grew, raw, len(blk.lens))
            # through the Python wrapper too
            reads = [(a, int(n)) for a, n in zip(keep, blk.lens)] if enc == PACKED else keep
            rd = ctx.reads_upload_start(reads, encoding=enc)
            ctx.reads_wait(rd)
            assert (ctx.reads_image(rd, len(devs) - 1) == want).all()
            ctx.reads_free(rd)
            rd = ctx.reads_upload(reads, encoding=enc)
            assert (ctx.reads_image(rd, 0) == want).all()
            ctx.reads_free(rd)
            assert ctx.inflight() == 0
    finally:
        arena.free()


def test_image_with_several_pieces_per_device_in_a_child_process():
    """BSW_READS_UP_BYTES is for tests and measurements: 4 KiB pieces cut the block into several per device under every
    encoding (11 747 raw bytes as codes or letters: three pieces; about 6 200 as words: two)"""
    env = dict(os.environ, BSW_READS_UP_BYTES="4096")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(here, "test_gpu_reads_enc.py"),
                        "-k", "test_image_equals"], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout


# ---- tickets behind the start ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(host, pac, both):
    return Work(host, pac, both, n_reads=300, n_e=600, n_m=150, n_c=150, seed=303)


def encode(host, reads, enc, rng):
    """the reads (codes 0..4) as letters of either case, or as bsw_pack_bases words with garbage behind the last base"""
    if enc == ASCII:
        up, lo = np.frombuffer(b"ACGTN", dtype=np.uint8), np.frombuffer(b"acgtn", dtype=np.uint8)
        return [np.where(rng.random(len(r)) < 0.5, up[r], lo[r]).astype(np.uint8) for r in reads]
    out = []
    for r in reads:
        w = host.pack_bases(r)[0]
        if len(r) & 15:
            w[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(4 * (len(r) & 15))
        out.append((w, len(r)))
    return out


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
@pytest.mark.parametrize("enc", [ASCII, PACKED], ids=ENC_IDS[1:])
def test_tickets_behind_a_start_with_letters_and_words(host, pac, small, enc, devs):
    with bound(host, pac, devs) as (ctx, ref):
        block = ctx.reads_upload(small.reads)                           # the codes, packed on the host
        tickets, want = small.submit_all(host, ctx, ref, block)
        for t in tickets:
            ctx.wait_ticket(t)
        want = (want[0].copy(), want[1].copy(), tuple(a.copy() for a in want[2]))
        assert (want[1]["status"] == 0).any() and (want[2][0]["status"] == 0).all()
        ctx.reads_free(block)
        rd = ctx.reads_upload_start(encode(host, small.reads, enc, np.random.default_rng(5)), encoding=enc)
        tickets, got = small.submit_all(host, ctx, ref, rd)             # no wait in between
        assert ctx.inflight() == 3
        for t in tickets:
            ctx.wait_ticket(t)
        ctx.reads_wait(rd)
        small.check(got, want)
        ctx.reads_free(rd)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_refusals_change_nothing(host, devs):
    L = host.lib()
    words = np.zeros(32, dtype=np.uint64)
    letters = np.frombuffer(b"ACGT" * 50, dtype=np.uint8).copy()
    one = np.array([150], dtype=np.int32)
    with host.BswContext(devices=devs) as ctx:
        rc, rd = start_enc(host, ctx, np.array([letters.ctypes.data], dtype=np.uint64), one, ASCII)      # (starts the slot threads)
        assert rc == 0
        ctx.reads_wait(rd)
        ctx.reads_free(rd)

        def counted():
            st = ctx.host_stats()
            return {k: st[k] for k in ("h2d_bytes", "d2h_bytes", "chunks", "submits", "seeds")}
        stats = counted()
        assert stats["h2d_bytes"] == len(devs) * (150 + 16)
        for fn in (start_enc, sync_enc):
            for enc in (3, -1, 255):                                                                   # an unknown encoding
                rc, h = fn(host, ctx, np.array([letters.ctypes.data], dtype=np.uint64), one, enc)
                assert rc == -2 and not h.value and b"encoding" in L.bsw_last_error(ctx.handle)
            for shift in (1, 2, 4, 7):                                                                 # a packed read off its 8-byte boundary
                ptrs = np.array([words.ctypes.data, 0, words.ctypes.data + shift], dtype=np.uint64)
                rc, h = fn(host, ctx, ptrs, np.array([150, 0, 40], dtype=np.int32), PACKED)
                assert rc == -2 and not h.value and b"read 2" in L.bsw_last_error(ctx.handle)
            ptrs = np.array([words.ctypes.data, 1], dtype=np.uint64)                                   # ... which a read without a base need not keep
            rc, h = fn(host, ctx, ptrs, np.array([150, 0], dtype=np.int32), PACKED)
            assert rc == 0
            ctx.reads_wait(h)
            ctx.reads_free(h)
            stats["h2d_bytes"] += len(devs) * (80 + 2 * 16) if fn is start_enc else 0
            for enc in ENCS:                                                                           # the per-read checks, as the existing calls answer them
                p1 = np.array([words.ctypes.data, 0], dtype=np.uint64)
                assert fn(host, ctx, p1, np.array([10, 5], dtype=np.int32), enc)[0] == -2              # a NULL read of 5 bases
                p2 = np.array([words.ctypes.data] * 2, dtype=np.uint64)
                assert fn(host, ctx, p2, np.array([10, -1], dtype=np.int32), enc)[0] == -2
                assert fn(host, ctx, p2[:1], np.array([65536], dtype=np.int32), enc)[0] == -3
        assert counted() == stats and ctx.inflight() == 0


@pytest.fixture(scope="module")
def work(host, pac, both):
    return Work(host, pac, both)


@pytest.mark.parametrize("devs", DEVS, ids=["one", "two_copies"])
def test_third_upload_in_flight_is_busy_under_every_encoding(host, pac, work, devs):
    """as tests/test_gpu_reads_async.py does it for the codes form, and with its workload: two uploads (letters, words) queue
    behind the three tickets of a resident block, a third start follows at once; repeated until it met both, eight times at the
    most, the third start's encoding changing from round to round"""
    n, L = len(work.reads), 150
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[work.flat]                         # read i at byte 150 i
    words = np.concatenate([host.pack_bases(r)[0] for r in work.reads])                  # read i at word 10 i
    lptr = (np.uint64(letters.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(L)).astype(np.uint64)
    wptr = (np.uint64(words.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(80)).astype(np.uint64)
    tiny = np.zeros(16, dtype=np.uint64)
    tptr, tlen = np.array([tiny.ctypes.data], dtype=np.uint64), np.array([100], dtype=np.int32)
    with bound(host, pac, devs) as (ctx, ref):
        front = ctx.reads_upload(work.reads)
        seen = False
        for attempt in range(8):
            tickets, _ = work.submit_all(host, ctx, ref, front)
            rc1, a = start_enc(host, ctx, lptr, work.lens, ASCII)                        # (the tables are ready: three calls in a row)
            rc2, b = start_enc(host, ctx, wptr, work.lens, PACKED)
            rc3, c = start_enc(host, ctx, tptr, tlen, ENCS[(attempt + 1) % 3])
            text = host.lib().bsw_last_error(ctx.handle)
            infl = ctx.inflight()
            for t in tickets:
                ctx.wait_ticket(t)
            assert rc1 == 0 and rc2 == 0 and rc3 in (0, -6) and infl == 3
            for h in (a, b) + ((c,) if rc3 == 0 else ()):
                ctx.reads_wait(h)
                ctx.reads_free(h)
            if rc3 == -6:
                assert not c.value and b"uploads in flight" in text
                seen = True
                break
        assert seen, "eight rounds and the third start never met two uploads in flight"
        assert ctx.inflight() == 0
        rc, again = start_enc(host, ctx, tptr, tlen, PACKED)            # the two places are free again
        rc2, more = start_enc(host, ctx, tptr, tlen, ASCII)
        assert rc == 0 and rc2 == 0
        for h in (again, more):
            ctx.reads_wait(h)
            ctx.reads_free(h)
        ctx.reads_free(front)
