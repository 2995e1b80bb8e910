"""BSW_VARIANT_RTL on the GPU: every entry point that takes a variant, bit-exact (every bsw_ext field including `cells`,
every pair field) against tests/ksw_extend_rtl_ref.c.  Each case also checks, on the reference, that RTL and H differ
on some of its sides: a path that silently ran H fails it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _gen
import _rtl_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ["tag", "qb", "qe", "rb", "re", "score", "truesc", "w"]
EXTF = ["score", "qle", "tle", "gtle", "gscore", "max_off", "aw", "cells"]
RTL = 2
MIX150 = dict(read_len=150, seed_len_min=19, seed_len_max=60, seed_at_start=0, sub_rate=0.01, indel_rate=0.001,
              junk_frac=0.05, n_rate=0.0005, w=100)
BP250 = dict(read_len=250, seed_len_min=19, seed_len_max=40, seed_at_start=0, sub_rate=0.04, indel_rate=0.01,
             junk_frac=0.05, n_rate=0.0005, w=500)


def assert_same(got, want):
    if got.tobytes() == want.tobytes():
        return
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "field %s differs at %s: got %s want %s" % (f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
    for side in ("left", "right"):
        for f in EXTF:
            bad = np.nonzero(got[side][f] != want[side][f])[0]
            assert bad.size == 0, "%s.%s differs at %s: got %s want %s" % (side, f, bad[:5], got[side][f][bad[:5]], want[side][f][bad[:5]])
    raise AssertionError("byte difference outside named fields")


def want_rtl(p, tasks, min_share=0.002):
    """the reference's RTL results, after checking that H differs from them on at least min_share of the sides"""
    p = R.with_variant(p, RTL)
    want = R.pair_batch(p, tasks)
    h = R.pair_batch(R.with_variant(p, 0), tasks)
    d = R.sides_differ(want, h)
    assert d.sum() >= max(1, int(min_share * len(d))), (int(d.sum()), len(d))
    return p, want


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("zdrop", [0, 100])
def test_kernels_mixed_150bp(host, kernel, zdrop):
    tasks, arena = host.synth_tasks(6000, seed=11 + zdrop, **MIX150)
    p, want = want_rtl(host.default_params(zdrop=zdrop), tasks)
    with host.BswContext(device=0, kernel=kernel) as c:
        assert_same(c.extend_pairs(p, tasks), want)


def test_lane_classes_and_boundaries(host):
    """one-seed-per-lane kernel: the 72 / 136 / 232-column 8-bit classes and their edges, and the 16-bit class"""
    rng = np.random.default_rng(5)
    seeds = []
    for ql in (1, 2, 63, 64, 65, 71, 72, 73, 127, 128, 135, 136, 137, 200, 231, 232, 233, 255):
        for k in range(40):
            tl = int(ql * rng.choice([0.8, 1.3, 2.0])) + 3
            t = rng.integers(0, 4, tl).astype(np.uint8)
            q = t[:ql].copy() if k % 5 else rng.integers(0, 4, ql).astype(np.uint8)
            q = _gen.mutate(rng, t, ql, 0.03, 0.01) if k % 2 else q
            seeds.append({"rq": q, "rt": t, "h0": int(rng.integers(5, 40)) if k % 7 else int(rng.integers(150, 260))})
            if k % 3 == 0:
                seeds[-1]["lq"], seeds[-1]["lt"] = q[::-1].copy(), t[::-1].copy()
    tasks, arena = host.make_tasks(seeds * 8)
    with host.BswContext(device=0, kernel=2) as c:
        for over in (dict(), dict(w=20), dict(o_del=300, e_del=1, o_ins=300, e_ins=1)):
            p, want = want_rtl(host.default_params(**over), tasks, 0.0005)
            assert_same(c.extend_pairs(p, tasks), want)


def test_16bit_class_and_250bp_w500(host, ctx):
    tasks, arena = host.synth_tasks(8000, seed=8, **BP250)
    p, want = want_rtl(host.default_params(w=500), tasks)
    assert_same(ctx.extend_pairs(p, tasks), want)
    seeds = _gen.random_seeds(np.random.default_rng(9), 8000, qmin=100, qmax=250, h0max=200, junk=0.1)
    tasks, arena = host.make_tasks(seeds)                                  # scores beyond 255: the 16-bit class
    p, want = want_rtl(host.default_params(), tasks)
    with host.BswContext(device=0, kernel=2) as c:
        assert_same(c.extend_pairs(p, tasks), want)


@pytest.mark.parametrize("qlen", [1024, 2047, 2048, 5000])
def test_long_kernel(host, ctx, qlen):
    rng = np.random.default_rng(qlen)
    seeds = []
    for k in range(12):
        t = rng.integers(0, 4, int(qlen * 1.2) + 5).astype(np.uint8)
        q = _gen.mutate(rng, t, qlen, 0.04, 0.01 if k % 2 else 0.0)
        if k % 4 == 0:
            q[rng.integers(0, qlen, 40)] = rng.integers(0, 4, 40)
        s = {"rq": q, "rt": t, "h0": int(rng.integers(5, 50))}
        if k % 3 == 0:
            s["lq"], s["lt"] = q[::-1].copy(), t[::-1].copy()
        seeds.append(s)
    tasks, arena = host.make_tasks(seeds)
    for over in (dict(), dict(w=40, zdrop=0)):
        p, want = want_rtl(host.default_params(**over), tasks, 0.0)
        assert_same(ctx.extend_pairs(p, tasks), want)


@pytest.mark.parametrize("kernel", [0, 2])
def test_n_bases_and_band_retry(host, kernel):
    tasks, arena = host.synth_tasks(30000, seed=81, seed_len_min=19, seed_len_max=60, seed_at_start=0, indel_rate=0.02,
                                    junk_frac=0.1, n_rate=0.01)
    with host.BswContext(device=0, kernel=kernel) as c:
        for over in (dict(w=8, zdrop=0), dict(w=3, max_band_try=3)):
            p, want = want_rtl(host.default_params(**over), tasks)
            assert int((want["left"]["aw"] > p["w"][0]).sum() + (want["right"]["aw"] > p["w"][0]).sum()) > 20   # retries happen
            assert_same(c.extend_pairs(p, tasks), want)


def test_fuzz_random_parameters(host, ctx):
    rng = np.random.default_rng(2026)
    for it in range(24):
        p = host.default_params(o_del=int(rng.integers(0, 12)), e_del=int(rng.integers(1, 5)), o_ins=int(rng.integers(0, 12)),
                                e_ins=int(rng.integers(1, 5)), w=int(rng.choice([5, 30, 100, 300])), zdrop=int(rng.choice([0, 40, 100])),
                                max_band_try=int(rng.integers(1, 4)))
        if it % 3 == 0:
            p["mat"][0] = rng.integers(-9, 10, 25).astype(np.int8)          # a general 5x5 matrix
        seeds = _gen.random_seeds(rng, 1500, qmin=1, qmax=int(rng.choice([40, 130, 250])), junk=float(rng.choice([0.0, 0.3])),
                                  nrate=float(rng.choice([0.0, 0.02])), h0max=int(rng.choice([30, 250])))
        tasks, arena = host.make_tasks(seeds)
        p, want = want_rtl(p, tasks, 0.0)
        assert_same(ctx.extend_pairs(p, tasks), want)


def test_submit_paths(host, ctx):
    """submit (tickets), submit_packed, upload + run, upload_raw + run_staged"""
    tasks, arena = host.synth_tasks(20000, seed=21, **MIX150)
    p, want = want_rtl(host.default_params(), tasks)
    out1 = ctx.submit(p, tasks)
    t1 = ctx.last_ticket
    out2 = ctx.submit(p, tasks)
    t2 = ctx.last_ticket
    ctx.wait_ticket(t2)
    ctx.wait_ticket(t1)
    assert_same(out1[:len(tasks)], want)
    assert_same(out2[:len(tasks)], want)
    ptasks, pk = host.pack_tasks(tasks)
    assert_same(ctx.extend_pairs_packed(p, ptasks), want)
    for up, run in ((ctx.upload, ctx.run), (ctx.upload_raw, ctx.run_staged)):
        b = up(p, tasks)
        run(b)
        assert_same(ctx.download(b)[:len(tasks)], want)
        b.free()


def test_extend_batch(host, ctx):
    rng = np.random.default_rng(3)
    n = 3000
    et = np.zeros(n, dtype=host.EXT_TASK)
    keep = []
    for i in range(n):
        ql, tl = int(rng.integers(1, 180)), int(rng.integers(0, 260))
        t = rng.integers(0, 4, tl).astype(np.uint8)
        q = _gen.mutate(rng, t, ql, 0.04, 0.02)
        keep.append((q, t))
        et[i]["query"], et[i]["target"] = q.ctypes.data, t.ctypes.data if tl else 0
        et[i]["qlen"], et[i]["tlen"] = ql, tl
        et[i]["w"], et[i]["end_bonus"], et[i]["h0"] = int(rng.choice([3, 20, 100, 200])), int(rng.choice([0, 5])), int(rng.integers(1, 70))
    p = host.default_params(variant=RTL)
    want = R.ext_batch(p, et)
    h = R.ext_batch(R.with_variant(p, 0), et)
    assert sum(int((want[f] != h[f]).sum()) for f in EXTF) > 0
    got = ctx.extend_batch(p, et)
    for f in EXTF:
        assert (got[f] == want[f]).all(), f


def test_scalar_abi_after_set_default_variant(host):
    L = host.lib()
    rng = np.random.default_rng(1)
    m = host.bwa_matrix()
    n_diff = 0
    L.bsw_set_default_variant(RTL)
    try:
        for it in range(40):
            ql, tl = int(rng.integers(1, 200)), int(rng.integers(0, 300))
            t = rng.integers(0, 4, tl).astype(np.uint8)
            q = _gen.mutate(rng, t, ql, 0.05, 0.02) if it % 4 else rng.integers(0, 4, ql).astype(np.uint8)
            outs = [C.c_int(0) for _ in range(5)]
            w, eb, zd, h0 = int(rng.choice([5, 50, 100])), int(rng.integers(0, 8)), int(rng.choice([0, 100])), int(rng.integers(1, 60))
            if it % 2:
                sc = L.ksw_extend2(ql, q.ctypes.data, tl, t.ctypes.data, 5, m.ctypes.data, 5, 2, 7, 1, w, eb, zd, h0,
                                   *[C.addressof(o) for o in outs])
                gap = (5, 2, 7, 1)
            else:
                sc = L.ksw_extend(ql, q.ctypes.data, tl, t.ctypes.data, 5, m.ctypes.data, 6, 1, w, eb, zd, h0,
                                  *[C.addressof(o) for o in outs])
                gap = (6, 1, 6, 1)
            ref = R.extend2(q, t, m.reshape(5, 5), *gap, w, eb, zd, h0, RTL)
            refh = R.extend2(q, t, m.reshape(5, 5), *gap, w, eb, zd, h0, 0)
            n_diff += ref != refh
            ref.pop("cells")
            got = dict(score=sc, qle=outs[0].value, tle=outs[1].value, gtle=outs[2].value, gscore=outs[3].value, max_off=outs[4].value)
            assert got == ref, it
    finally:
        L.bsw_set_default_variant(0)
    assert n_diff > 0


def test_reference_wire_format(host, ctx):
    tasks, arena = host.synth_tasks(800, seed=31, seed_at_start=0, seed_len_min=19, seed_len_max=60, indel_rate=0.01, junk_frac=0.1)
    p = host.default_params()
    words, n = host.refbatch_encode(p, tasks)
    out, nres = ctx.refbatch_run(words, variant=RTL, zdrop=0)
    assert nres == n
    got = host.refbatch_decode_results(out, n)
    p0, want = want_rtl(host.default_params(zdrop=0), tasks, 0.0)
    for f in FIELDS:
        assert (got[f] == want[f]).all(), f
    with pytest.raises(host.BswError):
        ctx.refbatch_run(words, variant=3, zdrop=0)


def test_submit_ref(host):
    from test_gpu_ref import _reads_and_seeds
    rng = np.random.default_rng(4)
    genome = rng.integers(0, 4, 200000).astype(np.uint8)
    lp = len(genome)
    pac = host.pack_pac(genome)
    n = 3000
    reads, seeds = _reads_and_seeds(host, rng, genome, n)
    p = host.default_params(variant=RTL)
    tasks, keep = host.seeds_to_tasks(p, pac, lp, reads, seeds)
    p, want = want_rtl(p, tasks)
    rt = np.zeros(n, dtype=host.REF_TASK)
    rmax = np.zeros(2, dtype=np.int64)
    qkeep = []
    for i in range(n):
        q = np.ascontiguousarray(reads[i])
        qkeep.append(q)
        host.lib().bsw_chain_window(p.ctypes.data, seeds[i:i + 1].ctypes.data, 1, len(q), lp, rmax.ctypes.data)
        rt[i]["query"], rt[i]["l_query"], rt[i]["init_score"] = q.ctypes.data, len(q), -1
        rt[i]["seed"] = seeds[i]
        rt[i]["rmax0"], rt[i]["rmax1"], rt[i]["tag"] = rmax[0], rmax[1], i
    with host.BswContext(device=0) as c:
        ref = c.ref_upload(pac, lp)
        assert_same(c.extend_ref(p, ref, rt), want)
        got = c.submit_ref(p, ref, rt)
        c.wait()
        assert_same(got[:n], want)
        c.ref_free(ref)


CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import __graft_entry__ as g
host = g.load_package().host
import _rtl_ref as R
spec = dict(read_len=150, seed_len_min=19, seed_len_max=60, seed_at_start=0, sub_rate=0.01, indel_rate=0.001, junk_frac=0.05, n_rate=0.002, w=100)
for kernel, n, seed in ((0, 3000, 1), (1, 20000, 2), (2, 20000, 3), (0, 100000, 4)):
    tasks, arena = host.synth_tasks(n, seed=seed, **spec)
    p = host.default_params(variant=2)
    want = R.pair_batch(p, tasks)
    assert R.sides_differ(want, R.pair_batch(R.with_variant(p, 0), tasks)).sum() > 0
    with host.BswContext(device=0, kernel=kernel) as c:
        got = c.extend_pairs(p, tasks)
    assert got.tobytes() == want.tobytes(), (kernel, n)
print("ok")
"""


@pytest.mark.parametrize("env", [dict(BSW_QUAD="1"), dict(BSW_NSPLIT="1")])
def test_child_process_switches(env):
    """BSW_QUAD=1 (the four-seeds-per-wavefront kernel for every general class) and BSW_NSPLIT=1: read once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=root)], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
