"""GPU parity for bwa's banded global alignment (ksw_global2) on queries of 1 024 to 8 191 bases: bsw_global_long_kernel
(the eh[] row in an LDS ring sized by the band) through the batch API and the drop-in ABI, against the CPU oracle, score
and CIGAR operation by operation (test_gpu_global.check: the CIGAR only where the band can hold a path).  A child process
under BSW_GLOBAL_LONG=1 sends read-sized tasks through the same kernel."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _gen
from test_gpu_global import check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def long_pair(rng, qlen, sub=0.04, indel=0.02, drift=0.03):
    """a query of qlen bases read off a target of about qlen (+- drift) bases"""
    tl = max(1, qlen + int(rng.integers(-int(qlen * drift), int(qlen * drift) + 1)))
    t = rng.integers(0, 4, tl).astype(np.uint8)
    return _gen.mutate(rng, t, qlen, sub, indel), t


# ring classes change where n_col + 1 crosses 256, 512, ..., 4 096 records: n_col = 2w + 1, so w = 127 | 128, 255 | 256, ...
RING_EDGE_WS = [127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048]


@pytest.mark.parametrize("qlen", [1023, 1024, 1025, 2047, 2048, 2049, 4096, 8190, 8191])
def test_class_edges(host, oracle, ctx, qlen):
    rng = np.random.default_rng(7000 + qlen)
    ws = [0, 10, 100] + [w for w in RING_EDGE_WS if 2 * w + 1 < qlen + 64] + [qlen, qlen + 5]
    pairs = [long_pair(rng, qlen) for _ in ws]
    check(host, oracle, ctx, host.default_params(), pairs, ws, max_cigar=qlen // 2 + 64)


def test_bands_and_unreachable_last_cell(host, oracle, ctx):
    rng = np.random.default_rng(71)
    pairs, ws = [], []
    for w in (0, 1, 10, 100, 500, 3000, 5000):
        pairs.append(long_pair(rng, 2500, drift=0.0))
        ws.append(w)
    q, t = long_pair(rng, 3000, drift=0.0)
    pairs += [(q, t[:1000]), (q[:1500], t), (q, t[:2800]), (q[:1200], np.concatenate([t, t]))]
    ws += [100, 100, 150, 400]                       # tlen + w < qlen; the band leaves the query (end < beg)
    check(host, oracle, ctx, host.default_params(), pairs, ws, max_cigar=2000)


@pytest.mark.parametrize("pen", [dict(o_del=5, e_del=2, o_ins=7, e_ins=1), dict(o_del=0, e_del=1, o_ins=0, e_ins=1),
                                 dict(o_del=4000, e_del=96, o_ins=4095, e_ins=1)],
                         ids=["asymmetric", "zero-open", "oe-4096"])
def test_gap_penalties(host, oracle, ctx, pen):
    rng = np.random.default_rng(72 + pen["o_del"])
    pairs = [long_pair(rng, 8191), long_pair(rng, 8191), long_pair(rng, 3000), long_pair(rng, 1500)]
    check(host, oracle, ctx, host.default_params(**pen), pairs, [8191, 100, 300, 40], max_cigar=4200)


def test_general_matrix_extremes_and_ns(host, oracle, ctx):
    rng = np.random.default_rng(73)
    p = host.default_params()
    mat = rng.choice(np.array([-128, -127, -1, 0, 1, 126, 127], dtype=np.int8), 25)
    for k in range(5):
        mat[k * 5 + k] = 127 if k % 2 else 126
    mat[4 * 5 + 4] = -128
    p["mat"][0] = mat
    pairs = []
    for ql in (1030, 2100, 5000, 8191):
        q, t = long_pair(rng, ql)
        q[rng.integers(0, ql, ql // 50)] = 4              # N in the query
        t[rng.integers(0, len(t), len(t) // 50)] = 4      # and in the target
        pairs.append((q, t))
    check(host, oracle, ctx, p, pairs, [ql for ql in (1030, 2100, 5000, 8191)], max_cigar=4200)
    check(host, oracle, ctx, p, pairs, [50, 200, 500, 1000], max_cigar=4200)


def test_target_of_65535(host, oracle, ctx):
    rng = np.random.default_rng(74)
    t = rng.integers(0, 4, 65535).astype(np.uint8)
    q1 = _gen.mutate(rng, t[:1100], 1100, 0.03, 0.01)
    q2 = _gen.mutate(rng, t[:2000], 1024, 0.03, 0.01)
    check(host, oracle, ctx, host.default_params(), [(q1, t), (q2, t)], [65535, 100], max_cigar=2000)


def test_cigar_overflow_is_reported(host, oracle, ctx):
    rng = np.random.default_rng(75)
    pairs = [long_pair(rng, 2000, drift=0.0), long_pair(rng, 6000, drift=0.0)]
    check(host, oracle, ctx, host.default_params(), pairs, [300, 400], max_cigar=3)


def test_mixed_short_and_long_batch(host, oracle, ctx):
    """read-sized and long tasks in one call: two kernels, results in task order"""
    rng = np.random.default_rng(76)
    pairs, ws = [], []
    for k in range(120):
        if k % 5 == 0:
            pairs.append(long_pair(rng, int(rng.integers(1024, 6000))))
            ws.append(int(rng.choice([50, 100, 500])))
        else:
            pairs.append(long_pair(rng, int(rng.integers(1, 1024))))
            ws.append(int(rng.integers(0, 120)))
    check(host, oracle, ctx, host.default_params(), pairs, ws, max_cigar=1500)


def test_dropin_from_threads(host, oracle):
    """ksw_global2 / ksw_global from 12 threads, 150 bp and 5 kb calls coalesced into shared trips; CIGARs malloc'ed"""
    rng = np.random.default_rng(77)
    L = host.lib()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    m = host.bwa_matrix()
    jobs = []
    for k in range(96):
        q, t = long_pair(rng, 5000 if k % 3 == 0 else 150)
        q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        w = 100 if k % 3 == 0 else 20
        w = max(w, abs(len(q) - len(t)))
        pen = (5, 2, 7, 1) if k % 2 else (6, 1, 6, 1)
        jobs.append((q, t, w, pen, oracle.global2(q, t, m, *pen, w)))
    errors = []

    def worker(idx):
        for k in range(idx, len(jobs), 12):
            q, t, w, pen, want = jobs[k]
            ncg, cg = C.c_int(0), C.POINTER(C.c_uint32)()
            if pen == (6, 1, 6, 1):
                sc = L.ksw_global(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, w, C.addressof(ncg), C.addressof(cg))
            else:
                sc = L.ksw_global2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, *pen, w, C.addressof(ncg), C.addressof(cg))
            got = [(int(cg[i]) & 0xf, int(cg[i]) >> 4) for i in range(ncg.value)]
            if sc != want["score"] or got != want["cigar"]:
                errors.append((k, len(q), sc, want["score"], ncg.value, len(want["cigar"])))
            libc.free(cg)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(12)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:5]


SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import __graft_entry__ as g
host, orc = g.load_package().host, g.load_oracle()
import _gen
from test_gpu_global import check
rng = np.random.default_rng(78)
with host.BswContext(device=0) as ctx:
    # the edge shapes of test_gpu_global.test_edge_shapes_and_narrow_bands
    z = np.zeros(0, np.uint8)
    s = rng.integers(0, 4, 40).astype(np.uint8)
    pairs = [(s, s), (s, z), (z, s), (z, z), (s[:1], s[:1]), (s[:1], s), (s, s[:1]), (s, s[5:]), (s[7:], s)]
    ws = [100, 100, 100, 5, 0, 100, 100, 3, 2]
    for k in range(300):
        ql, tl = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        pairs.append((rng.integers(0, 5, ql).astype(np.uint8), rng.integers(0, 5, tl).astype(np.uint8)))
        ws.append(int(rng.choice([0, 1, 2, 5, 20, 500])))
    check(host, orc, ctx, host.default_params(), pairs, ws, max_cigar=200)
    # seeded fuzz over qlen 0 .. 1 100: every ring class, both sides of the register kernel's limit
    for pen in (dict(), dict(o_del=5, e_del=2, o_ins=7, e_ins=1)):
        pairs, ws = [], []
        for k in range(400):
            ql = int(rng.integers(0, 1101))
            tl = max(0, ql + int(rng.integers(-20, 21)))
            t = rng.integers(0, 4, tl).astype(np.uint8)
            q = _gen.mutate(rng, t, ql, 0.05, 0.03) if tl and ql else rng.integers(0, 5, ql).astype(np.uint8)
            if ql and rng.random() < 0.2:
                q[rng.integers(0, ql)] = 4
            pairs.append((q, t))
            ws.append(int(rng.choice([0, 1, 3, 20, 60, 127, 128, 300, 2000])))
        check(host, orc, ctx, host.default_params(**pen), pairs, ws, max_cigar=700)
print("ok")
"""


def test_forced_long_kernel_fuzz():
    env = dict(os.environ, BSW_GLOBAL_LONG="1")
    out = subprocess.run([sys.executable, "-c", SNIPPET % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
