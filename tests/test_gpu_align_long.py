"""ksw_align2 for queries of 1 025 to 8 191 bases (bsw_set_align_long, bsw_align_long_kernel) against the oracle's literal
emulation: every output field, both modes, every vector-count boundary around 1 024 bases and around the class edges, the lazy-F
loop across a lane boundary, the start-point pass on long prefixes, every small shape under mode 2, the scalar ABI and mate rescue
against the resident reference.  Every test that turns the switch on restores 0."""
import ctypes as C
import threading

import numpy as np
import pytest

import _gen
import _gencigar_ref as gc
import _matesw_ref as mr

pytestmark = pytest.mark.gpu
XB, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000
FIELDS = ("score", "te", "qe", "score2", "te2", "tb", "qb")
LENGTHS = [1025, 1026, 1031, 1032, 1033, 1040, 1041, 1279, 1500, 2047, 2048, 2049, 3000, 4095, 4096, 4097, 6000, 8184, 8185, 8190, 8191]
XTRAS = [XSUBO | XSTART | 19, XSTART, XSUBO | 40, 0]
L_PAC = 300_003
BYTE_BOUNDS = [16, 32, 64, 128, 256, 512]          # slen bounds of the new kernel's classes, 8-bit mode then 16-bit mode
WORD_BOUNDS = [32, 64, 128, 256, 512, 1024]


def long_class(qlen, byte):
    """index into bsw_align_long_stats of the class that takes the query (the header's rule)"""
    slen = -(-qlen // (16 if byte else 8))
    bounds = BYTE_BOUNDS if byte else WORD_BOUNDS
    return (0 if byte else len(BYTE_BOUNDS)) + next(k for k, b in enumerate(bounds) if slen <= b)


def make(host, pairs, xtras):
    at = np.zeros(len(pairs), dtype=host.ATASK)
    keep = []
    for i, ((q, t), x) in enumerate(zip(pairs, xtras)):
        q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
        keep.append((q, t))
        at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = q.ctypes.data, t.ctypes.data, len(q), len(t), x
    return at, keep


def expect(oracle, p, at):
    want, _ = oracle.align2_batch(p["mat"][0], int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0]), at, nthreads=8)
    return want


def same(at, got, want):
    for k, f in enumerate(FIELDS):
        bad = np.nonzero(got[f] != want[:, k])[0]
        assert bad.size == 0, "%s: task %s (qlen %s tlen %s xtra %s) got %s want %s" % (
            f, bad[:4], at["qlen"][bad[:4]], at["tlen"][bad[:4]], [hex(x) for x in at["xtra"][bad[:4]]], got[f][bad[:4]], want[bad[:4], k])


def run_mode(host, ctx, mode, p, at):
    """align_batch under the mode -> (results, growth of bsw_align_long_stats per class); the switch is 0 afterwards"""
    before = np.array(host.align_long_stats(), dtype=np.int64)
    host.set_align_long(mode)
    try:
        got = ctx.align_batch(p, at)
    finally:
        host.set_align_long(0)
    return got, np.array(host.align_long_stats(), dtype=np.int64) - before


def classes_of(at):
    return sorted({long_class(int(t["qlen"]), bool(t["xtra"] & XB)) for t in at})


@pytest.fixture(scope="module")
def ctx(host):
    with host.BswContext(device=0) as c:
        yield c


def family(rng, piece_len, sub, indel, rep):
    """per length: flank + a mutated piece of the query from a random offset + 60 random bases + a repeat of part of the piece +
    flank; both modes x four flag sets"""
    pairs, xt = [], []
    for L in LENGTHS:
        q = rng.integers(0, 4, L).astype(np.uint8)
        a = int(rng.integers(0, L - piece_len + 1))
        piece = _gen.mutate(rng, q[a:], piece_len, sub, indel)
        t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 150))), piece, rng.integers(0, 4, 60), piece[rep[0]:rep[1]],
                            rng.integers(0, 4, int(rng.integers(0, 150)))]).astype(np.uint8)
        for base in (0, XB):
            for x in XTRAS:
                pairs.append((q, t)); xt.append(base | x)
    return pairs, xt


def test_off_by_default_and_the_limits_of_each_mode(host, oracle, ctx):
    import os
    if os.environ.get("BSW_ALIGN_LONG") not in ("1", "2"):
        assert host.align_long() == 0
    host.set_align_long(0)
    rng = np.random.default_rng(4099)
    p = host.default_params()
    q = rng.integers(0, 4, 1025).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 50), _gen.mutate(rng, q, 1025, 0.03, 0.01), rng.integers(0, 4, 50)]).astype(np.uint8)
    at, keep = make(host, [(q, t)], [XSUBO | XSTART | 19])
    with pytest.raises(host.BswError) as ex:
        ctx.align_batch(p, at)
    assert ex.value.code == -3
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, expect(oracle, p, at))
    assert got["score"][0] > 255 and grew.sum() == 1 and grew[long_class(1025, False)] == 1
    assert host.align_long() == 0
    big, keep2 = make(host, [(np.zeros(8192, np.uint8), t)], [0])
    for mode in (1, 2):
        host.set_align_long(mode)
        try:
            assert host.align_long() == mode
            with pytest.raises(host.BswError) as ex:
                ctx.align_batch(p, big)
            assert ex.value.code == -3
        finally:
            host.set_align_long(0)
    host.set_align_long(7)                              # anything else is 0
    assert host.align_long() == 0


def test_family_p_long_matches_with_a_repeat(host, oracle, ctx):
    """scores far beyond the 8-bit range, start points and ends beyond position 1 024, a second-best end; 8-bit runs saturate"""
    p = host.default_params()
    pairs, xt = family(np.random.default_rng(4100), 900, 0.05, 0.02, (200, 500))
    at, keep = make(host, pairs, xt)
    want = expect(oracle, p, at)
    word = (at["xtra"] & XB) == 0
    print("family P: word score>255 %d, tb>=0 %d, qb>1024 %d, qe>1024 %d, score2>=0 %d; byte saturated %d" % (
        (want[word, 0] > 255).sum(), (want[word, 5] >= 0).sum(), (want[word, 6] > 1024).sum(), (want[word, 2] > 1024).sum(),
        (want[word, 3] >= 0).sum(), (want[~word, 0] == 255).sum()))
    assert (want[word, 0] > 255).sum() >= 42 and (want[word, 5] >= 0).sum() >= 21 and (want[word, 6] > 1024).sum() >= 8
    assert (want[word, 2] > 1024).sum() >= 30 and (want[word, 3] >= 0).sum() >= 21 and (want[~word, 0] == 255).sum() >= 42
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, want)
    assert [c for c in range(len(grew)) if grew[c]] == classes_of(at) and grew.max() == 1


def test_family_s_byte_mode_that_does_not_saturate(host, oracle, ctx):
    p = host.default_params()
    pairs, xt = family(np.random.default_rng(4102), 130, 0.04, 0.01, (30, 90))
    at, keep = make(host, pairs, xt)
    want = expect(oracle, p, at)
    byte = (at["xtra"] & XB) != 0
    print("family S: byte score<255 %d, tb>=0 %d, qb>1024 %d, score2>=0 %d" % (
        (want[byte, 0] < 255).sum(), (want[byte, 5] >= 0).sum(), (want[byte, 6] > 1024).sum(), (want[byte, 3] >= 0).sum()))
    assert (want[byte, 0] < 255).sum() >= 42 and (want[byte, 5] >= 0).sum() >= 21 and (want[byte, 6] > 1024).sum() >= 11
    assert (want[byte, 3] >= 0).sum() >= 20
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, want)
    assert [c for c in range(len(grew)) if grew[c]] == classes_of(at)


def test_family_i_lazy_f_across_a_lane_boundary(host, oracle, ctx):
    """the query carries a 20-base insertion that straddles the boundary between two lanes' stripes: F has to travel from the last
    vector of one lane into the first vector of the next"""
    rng = np.random.default_rng(4104)
    p = host.default_params()
    pairs, xt, bnd = [], [], []
    for L in LENGTHS:
        q = rng.integers(0, 4, L).astype(np.uint8)
        for base, NP, half in ((0, 8, 200), (XB, 16, 60)):
            slen = -(-L // NP)
            ks = [k for k in range(1, NP) if k * slen - half >= 0 and k * slen + half <= L]
            for k in (ks[0], ks[-1]):
                b = k * slen
                t = np.concatenate([rng.integers(0, 4, 40), q[b - half:b - 10], q[b + 10:b + half], rng.integers(0, 4, 40)]).astype(np.uint8)
                pairs.append((q, t)); xt.append(base | XSUBO | XSTART | 19); bnd.append(b)
    at, keep = make(host, pairs, xt)
    want = expect(oracle, p, at)
    bnd = np.array(bnd)
    assert len(at) == 84
    assert ((want[:, 2] - want[:, 6]) - (want[:, 1] - want[:, 5]) == 20).all()
    assert (want[:, 6] < bnd - 10).all() and (want[:, 2] >= bnd + 10).all() and (want[:, 6] >= 0).all()
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, want)
    assert [c for c in range(len(grew)) if grew[c]] == classes_of(at)


def test_two_full_size_tasks(host, oracle, ctx):
    """1 025 and 8 191 bases in 16-bit mode against a mutated copy of the whole query between two flanks.  The 8 191 x 8 391 task is
    the slowest single alignment the route takes: one lane group walks 2 x 8 391 rows of 1 024 vectors, a few seconds on one MI355X
    (DESIGN.md 4.5b), most of this test's time."""
    rng = np.random.default_rng(4106)
    p = host.default_params()
    pairs = []
    for ql in (1025, 8191):
        q = rng.integers(0, 4, ql).astype(np.uint8)
        t = np.concatenate([rng.integers(0, 4, 100), _gen.mutate(rng, q, ql, 0.03, 0.01), rng.integers(0, 4, 100)]).astype(np.uint8)
        pairs.append((q, t))
    at, keep = make(host, pairs, [XSUBO | XSTART | 19] * 2)
    want = expect(oracle, p, at)
    print("full-size tasks: oracle scores", want[:, 0].tolist())
    assert (want[:, 0] > 255).all()
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, want)
    assert grew[long_class(1025, False)] == 1 and grew[long_class(8191, False)] == 1 and grew.sum() == 2


def test_every_small_shape_on_the_new_kernel(host, oracle, ctx):
    """mode 2: query lengths 1..300 in both modes (every slen up to 19 / 38 with every tail), the degenerate inputs and the
    saturation edge, four scoring sets — all on bsw_align_long_kernel: every class a task belongs to is launched exactly once per
    call, which is every task's route under mode 2"""
    import test_gpu_align as ta
    rng = np.random.default_rng(3)
    p = host.default_params()
    pairs, xt = [], []
    for ql in range(1, 301):
        t = rng.integers(0, 4, int(rng.integers(ql, 2 * ql + 40))).astype(np.uint8)
        a = int(rng.integers(0, len(t) - ql + 1))
        q = _gen.mutate(rng, t[a:a + ql], ql, 0.03, 0.02)
        for x in (XB | XSUBO | XSTART | 19, XSUBO | XSTART | 19):
            pairs.append((q, t)); xt.append(x)
    at, keep = make(host, pairs, xt)
    want = expect(oracle, p, at)
    print("small shapes: %d tasks, tb>=0 %d, score2>=0 %d" % (len(at), (want[:, 5] >= 0).sum(), (want[:, 3] >= 0).sum()))
    assert len(at) == 600 and (want[:, 5] >= 0).sum() >= 271 and (want[:, 3] >= 0).sum() >= 157
    got, grew = run_mode(host, ctx, 2, p, at)
    same(at, got, want)
    assert [c for c in range(len(grew)) if grew[c]] == classes_of(at) and grew.max() == 1
    # the counters count launches, not tasks: a batch of ONE task makes exactly one launch, and it has to be the new kernel's, at
    # the task's class (a task that took bsw_align_kernel would leave every counter where it was)
    for k in (0, 1, 298, 299, 598, 599):                   # 1, 150 and 300 bases, 8-bit and 16-bit mode
        got1, grew1 = run_mode(host, ctx, 2, p, at[k:k + 1])
        same(at[k:k + 1], got1, want[k:k + 1])
        assert grew1.sum() == 1 and grew1[long_class(int(at["qlen"][k]), bool(at["xtra"][k] & XB))] == 1, (k, grew1)
    still = host.align_long_stats()
    got0 = ctx.align_batch(p, at[298:300])                  # and with the switch off none moves
    assert got0.tobytes() == got[298:300].tobytes() and host.align_long_stats() == still

    rng = np.random.default_rng(4)
    q = rng.integers(0, 4, 256).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 20), q, rng.integers(0, 4, 20)]).astype(np.uint8)
    pairs = [(q, t), (q, t), (q[:250], t), (q[:251], t), (np.zeros(30, np.uint8), np.full(90, 3, np.uint8)),
             (q[:40], np.zeros(0, np.uint8)), (np.full(60, 4, np.uint8), t), (q[:1], t[:1])]
    xt = [XB | XSTART, XSTART, XB | XSTART, XB | XSTART, XB | XSTART, XB, XSTART | XSUBO | 1, XB | XSTART]
    at, keep = make(host, pairs, xt)
    got, grew = run_mode(host, ctx, 2, p, at)
    same(at, got, expect(oracle, p, at))
    assert got["score"][0] == 255 and got["score"][1] == 256 and got["score"][2] == 250
    assert [c for c in range(len(grew)) if grew[c]] == classes_of(at) and grew.max() == 1

    for seed in range(4):
        rng = np.random.default_rng(20 + seed)
        a, b, nn = [(1, 4, -1), (2, 3, -2), (1, 1, 0), (3, 6, -1)][seed]
        ps = host.default_params(o_del=int(rng.integers(0, 12)), e_del=int(rng.integers(1, 5)), o_ins=int(rng.integers(0, 12)), e_ins=int(rng.integers(1, 5)))
        ps["mat"][0] = host.bwa_matrix(a, b, nn)
        pairs = ta.rescue_like(rng, 300, 200 if a < 3 else 80, 500)
        xt = [int(rng.choice([XB, 0])) | XSUBO | XSTART | int(rng.integers(5, 40)) for _ in pairs]
        at, keep = make(host, pairs, xt)
        got, grew = run_mode(host, ctx, 2, ps, at)
        same(at, got, expect(oracle, ps, at))
        assert [c for c in range(len(grew)) if grew[c]] == classes_of(at) and grew.max() == 1


def test_mixed_batch_takes_both_routes(host, oracle, ctx):
    rng = np.random.default_rng(4108)
    p = host.default_params()
    pairs, xt = [], []
    for i in range(48):
        ql = (150, 1024, 1025, 3000)[i % 4]
        q = rng.integers(0, 4, ql).astype(np.uint8)
        t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 100))), _gen.mutate(rng, q[ql // 3:], min(ql, 400) // 2, 0.04, 0.01),
                            rng.integers(0, 4, int(rng.integers(0, 100)))]).astype(np.uint8)
        pairs.append((q, t)); xt.append((XB if (i // 4) & 1 else 0) | XSUBO | XSTART | 19)
    at, keep = make(host, pairs, xt)
    want = expect(oracle, p, at)
    got, grew = run_mode(host, ctx, 1, p, at)
    same(at, got, want)                                     # in task order
    used = sorted({long_class(ql, byte) for ql in (1025, 3000) for byte in (False, True)})
    assert [c for c in range(len(grew)) if grew[c]] == used and grew.sum() == len(used) == 4
    short = np.nonzero(at["qlen"] <= 1024)[0]               # the same short tasks alone, switch off: the register kernel's results
    got0 = ctx.align_batch(p, at[short])
    assert got0.tobytes() == got[short].tobytes()


def test_two_threads_launch_different_large_lds_classes_at_once(host, oracle):
    """Four of the classes that need more than 64 KiB of dynamic LDS, each with a byte count of its own, launched from two threads with
    a context each on one device at the same time: the limit on the dynamic LDS is one per kernel and device, so it must not depend on
    which class set it last."""
    rng = np.random.default_rng(4114)
    p = host.default_params()
    work = []
    for qls, base in (((3000, 6000), XB), ((6000, 3000), 0)):             # thread 0: the two 8-bit classes, thread 1: the two 16-bit ones
        pairs, xt = [], []
        for ql in qls:
            q = rng.integers(0, 4, ql).astype(np.uint8)
            t = np.concatenate([rng.integers(0, 4, 30), _gen.mutate(rng, q[ql // 2:], 150, 0.03, 0.01), rng.integers(0, 4, 30)]).astype(np.uint8)
            pairs.append((q, t)); xt.append(base | XSUBO | XSTART | 19)
        at, keep = make(host, pairs, xt)
        work.append((at, keep, expect(oracle, p, at)))
    rounds, errors = 6, []
    gate = threading.Barrier(2)

    def worker(k):
        at, keep, want = work[k]
        try:
            with host.BswContext(device=0) as c:
                for r in range(rounds):
                    gate.wait(timeout=60)
                    for one in ((0, 1), (1, 2)):                         # one class per call, alternating
                        got = c.align_batch(p, at[one[0]:one[1]])
                        same(at[one[0]:one[1]], got, want[one[0]:one[1]])
        except Exception as ex:                                         # noqa: BLE001 (reported by the main thread)
            errors.append((k, repr(ex)))
            gate.abort()

    before = np.array(host.align_long_stats(), dtype=np.int64)
    host.set_align_long(1)
    try:
        th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
    finally:
        host.set_align_long(0)
    assert not errors, errors
    grew = np.array(host.align_long_stats(), dtype=np.int64) - before
    large = sorted({long_class(3000, True), long_class(6000, True), long_class(3000, False), long_class(6000, False)})
    assert [c for c in range(len(grew)) if grew[c]] == large and (grew[large] == rounds).all()


class KSWR(C.Structure):
    _fields_ = [(f, C.c_int) for f in FIELDS]


def test_scalar_abi_with_a_concurrent_short_caller(host, oracle):
    L = host.lib()
    L.ksw_align2.restype = KSWR
    L.ksw_align2.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.ksw_align.restype = KSWR
    L.ksw_align.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]
    rng = np.random.default_rng(4110)
    m = host.bwa_matrix()
    q = rng.integers(0, 4, 2000).astype(np.uint8)
    t = np.concatenate([rng.integers(0, 4, 250), _gen.mutate(rng, q, 2000, 0.03, 0.01), rng.integers(0, 4, 250)]).astype(np.uint8)[:2500]
    sq = rng.integers(0, 4, 150).astype(np.uint8)
    st = np.concatenate([rng.integers(0, 4, 100), _gen.mutate(rng, sq, 150, 0.03, 0.01), rng.integers(0, 4, 100)]).astype(np.uint8)
    x = XSUBO | XSTART | 19
    short_got, stop = [], threading.Event()

    def short_caller():
        while not stop.is_set() or len(short_got) < 4:
            r = L.ksw_align2(len(sq), sq.ctypes.data, len(st), st.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, XB | x, None)
            short_got.append([getattr(r, f) for f in FIELDS])

    assert L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, x, None).score == -1     # off: the call's failure
    host.set_align_long(1)
    th = threading.Thread(target=short_caller)
    try:
        th.start()
        long_got = []
        for _ in range(3):
            r = L.ksw_align2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 6, 1, 6, 1, x, None)
            long_got.append(("align2", [getattr(r, f) for f in FIELDS]))
            r = L.ksw_align(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, m.ctypes.data, 5, 2, x, None)
            long_got.append(("align", [getattr(r, f) for f in FIELDS]))
    finally:
        stop.set()
        th.join()
        host.set_align_long(0)
    w2 = oracle.align2(q, t, m, 6, 1, 6, 1, x)
    w1 = oracle.align2(q, t, m, 5, 2, 5, 2, x)
    assert w2["score"] > 255
    for which, g in long_got:
        assert g == [(w2 if which == "align2" else w1)[f] for f in FIELDS], which
    ws = oracle.align2(sq, st, m, 6, 1, 6, 1, XB | x)
    assert len(short_got) >= 4 and all(g == [ws[f] for f in FIELDS] for g in short_got)


def test_mate_rescue_of_long_mates(host, oracle, ctx):
    import test_gpu_matesw_ref as tm
    rng = np.random.default_rng(4112)
    pac = gc.pack_pac(np.random.default_rng(77).integers(0, 4, L_PAC).astype(np.uint8))
    ref = ctx.ref_upload(pac, L_PAC)
    p = host.default_params()
    specs = []
    for l_ms in (1025, 1500, 3000):
        for is_rev in (0, 1):
            for strand in (0, 1):
                for byte in (0, XB):
                    rb, re = tm.window(rng, strand, l_ms + 600)
                    specs.append(tm.task(tm.mate_in(rng, pac, rb, re, l_ms, is_rev, sub=0.03), is_rev, rb, re, xtra=byte | XSUBO | XSTART | 19, min_score=19))
    rd = None
    try:
        host.set_align_long(1)
        res, want = tm.check(host, oracle, ctx, p, (pac, ref), specs)
        word = np.array([(s["xtra"] & XB) == 0 for s in specs])
        assert (res["status"][word] == 0).sum() >= 6 and (res["aln"]["score"][word] > 255).sum() >= 6
        # the host recipe: bns_get_seq, reverse-complement the mate when is_rev
        at = np.zeros(len(specs), dtype=host.ATASK)
        keep = []
        for i, s in enumerate(specs):
            rseq = gc.bns_get_seq(pac, L_PAC, s["rb"], s["re"])
            q = np.ascontiguousarray(mr.revcomp(s["mate"]) if s["is_rev"] else s["mate"])
            keep += [q, rseq]
            at[i]["query"], at[i]["target"], at[i]["qlen"], at[i]["tlen"], at[i]["xtra"] = q.ctypes.data, rseq.ctypes.data, len(q), len(rseq), s["xtra"]
        aln = ctx.align_batch(p, at)
        assert aln.tobytes() == np.ascontiguousarray(res["aln"]).tobytes()
        # the two ticket forms
        mt, keep2 = tm.make_mtasks(host, specs)
        t1, r1 = ctx.submit_matesw_ref(p, ref, mt)
        ctx.wait_ticket(t1)
        assert r1.tobytes() == res.tobytes()
        reads = [s["mate"] for s in specs]
        rd = ctx.reads_upload(reads)
        rdt = np.zeros(len(specs), dtype=host.RD_MTASK)
        for k, s in enumerate(specs):
            rdt[k] = (k, s["is_rev"], s["rb"], s["re"], s["xtra"], s["min_score"])
        t2, r2 = ctx.submit_matesw_reads(p, ref, rd, rdt)
        ctx.wait_ticket(t2)
        assert r2.tobytes() == res.tobytes()
        # submitted under mode 1, collected under mode 0
        t3, r3 = ctx.submit_matesw_ref(p, ref, mt)
        host.set_align_long(0)
        ctx.wait_ticket(t3)
        assert r3.tobytes() == res.tobytes()
        with pytest.raises(host.BswError) as ex:           # and the switch is off again for what enters now
            ctx.submit_matesw_ref(p, ref, mt)
        assert ex.value.code == -3
    finally:
        host.set_align_long(0)
        if rd is not None:
            ctx.reads_free(rd)
        ctx.ref_free(ref)
