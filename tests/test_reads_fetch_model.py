"""The word fetch of the resident read store (csrc/bsw_reads_fetch.h: bsw_reads_word, the function bsw_pack_kernel inlines for
BSW_PACK_STORE launches), compiled by g++ and checked against a byte loop: every start phase, the lengths around a word, both
directions, the first and the last read of a store (the windows that reach into the slack words), N codes and codes 5 - 255."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rf") / "reads_fetch_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "reads_fetch_model.cpp")])
    L = C.CDLL(so)
    L.reads_model_slack.restype = C.c_int
    L.reads_model_pack.restype = C.c_long
    L.reads_model_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.reads_model_fetch.restype = None
    L.reads_model_fetch.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    return L


class Store:
    """reads -> the device image (slack | reads | slack), and the expected words of any run of bases by a byte loop"""
    POISON = 0xA5A5A5A5A5A5A5A5

    def __init__(self, model, reads):
        self.model, self.reads = model, [np.asarray(r, dtype=np.uint8) for r in reads]
        lens = np.array([len(r) for r in self.reads], dtype=np.int32)
        words = int(sum((int(n) + 15) // 16 for n in lens))
        self.slack = model.reads_model_slack()
        # a poisoned guard word either side of the image: a fetch that reached beyond the slack would hand back its bits
        self.raw = np.full(words + 2 * self.slack + 2, self.POISON, dtype=np.uint64)
        self.buf = self.raw[1:-1]
        self.buf[:] = 0
        flat = np.concatenate(self.reads + [np.zeros(1, dtype=np.uint8)])
        self.woff = np.zeros(max(len(lens), 1), dtype=np.uint32)
        got = model.reads_model_pack(flat.ctypes.data, lens.ctypes.data, len(lens), self.buf.ctypes.data, self.woff.ctypes.data)
        assert got == words
        assert not self.buf[:self.slack].any() and not self.buf[len(self.buf) - self.slack:].any()

    def pos(self, read):
        return 16 * int(self.woff[read])

    def fetch(self, s, backwards, L):
        out = np.full((L + 15) // 16 + 1, self.POISON, dtype=np.uint64)
        self.model.reads_model_fetch(self.buf.ctypes.data, s, int(backwards), L, out.ctypes.data)
        assert out[-1] == self.POISON
        return out[:-1]

    def want(self, read, first, backwards, L):
        """words of bases first, first +- 1, ... of `read` by a byte loop"""
        r = self.reads[read]
        out = np.zeros((L + 15) // 16, dtype=np.uint64)
        for i in range(L):
            c = int(r[first - i] if backwards else r[first + i])
            out[i >> 4] |= np.uint64(min(c, 4) << (4 * (i & 15)))
        return out


def rnd_reads(rng, lens, hi=4):
    return [rng.integers(0, hi, size=n, dtype=np.uint8) for n in lens]


def test_every_phase_length_and_direction(model):
    """start phase 0 - 15 x length 0 - 49 x forwards / backwards, inside a read that sits between two others"""
    rng = np.random.default_rng(1)
    st = Store(model, rnd_reads(rng, [37, 140, 23]))
    p1 = st.pos(1)
    for phase in range(16):
        for L in range(50):
            for off in (phase, 16 + phase, 32 + phase):
                got = st.fetch(p1 + off, False, L)
                assert (got == st.want(1, off, False, L)).all(), (phase, L, off, "forwards")
                last = off + L - 1 if L else off
                got = st.fetch(p1 + last, True, L)
                assert (got == st.want(1, last, True, L)).all(), (phase, L, off, "backwards")


def test_first_and_last_read_touch_the_slack(model):
    """backwards from base 0 .. 15 of the FIRST read (the window starts up to 15 bases in front of the store) and forwards to
    the last base of the LAST read (the second word of the window lies behind the store)"""
    rng = np.random.default_rng(2)
    for last_len in (1, 15, 16, 17, 31, 32, 33, 150):
        st = Store(model, rnd_reads(rng, [40, 64, last_len]))
        for b in range(16):
            got = st.fetch(st.pos(0) + b, True, b + 1)
            assert (got == st.want(0, b, True, b + 1)).all(), ("first", b)
        for first in range(min(last_len, 17)):
            L = last_len - first
            got = st.fetch(st.pos(2) + first, False, L)
            assert (got == st.want(2, first, False, L)).all(), ("last", last_len, first)
        got = st.fetch(st.pos(2) + last_len - 1, True, last_len)
        assert (got == st.want(2, last_len - 1, True, last_len)).all()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17])
def test_short_reads_whole_in_both_directions(model, n):
    rng = np.random.default_rng(3 + n)
    st = Store(model, rnd_reads(rng, [n, 5, n, 33, n]))
    for read in (0, 2, 4):
        assert (st.fetch(st.pos(read), False, n) == st.want(read, 0, False, n)).all()
        if n:
            assert (st.fetch(st.pos(read) + n - 1, True, n) == st.want(read, n - 1, True, n)).all()
    assert len(st.fetch(st.pos(0), False, 0)) == 0 and len(st.fetch(st.pos(0), True, 0)) == 0


def test_an_n_as_first_last_and_sixteenth_base(model):
    rng = np.random.default_rng(4)
    for at in ("first", "last", "sixteenth"):
        r = rng.integers(0, 4, size=40, dtype=np.uint8)
        k = {"first": 0, "last": 39, "sixteenth": 15}[at]
        r[k] = 4
        st = Store(model, [rng.integers(0, 4, size=20, dtype=np.uint8), r, rng.integers(0, 4, size=20, dtype=np.uint8)])
        for first in range(0, 24):
            for L in (1, 15, 16, 17, 40 - first):
                if first + L > 40:
                    continue
                got = st.fetch(st.pos(1) + first, False, L)
                assert (got == st.want(1, first, False, L)).all()
                assert bool((got & np.uint64(0x4444444444444444)).any()) == (first <= k < first + L), (at, first, L)
                back = st.fetch(st.pos(1) + first + L - 1, True, L)
                assert (back == st.want(1, first + L - 1, True, L)).all()
                assert bool((back & np.uint64(0x4444444444444444)).any()) == (first <= k < first + L)


def test_codes_5_to_255_are_stored_as_n(model):
    r = np.arange(256, dtype=np.uint8)
    st = Store(model, [r[:7], r, r[250:]])
    for first, L in ((0, 256), (3, 200), (5, 17), (240, 16)):
        got = st.fetch(st.pos(1) + first, False, L)
        assert (got == st.want(1, first, False, L)).all()
        assert ((got >> np.uint64(3)) & np.uint64(0x1111111111111111) == 0).all()      # no nibble above 7 ...
        back = st.fetch(st.pos(1) + first + L - 1, True, L)
        assert (back == st.want(1, first + L - 1, True, L)).all()
    w = st.fetch(st.pos(1), False, 16)[0]
    assert [(int(w) >> (4 * k)) & 15 for k in range(16)] == [0, 1, 2, 3] + [4] * 12   # ... and none between 5 and 7


def test_pack_matches_the_librarys_device_format(model, host):
    """the model's store is the format bsw_pack_bases produces (what bsw_reads_upload packs with)"""
    rng = np.random.default_rng(5)
    r = rng.integers(0, 6, size=77, dtype=np.uint8)
    st = Store(model, [r])
    words, _ = host.pack_bases(r)
    assert (st.buf[st.slack:st.slack + 5] == np.asarray(words, dtype=np.uint64)[:5]).all()
