"""BSW_VARIANT_RTL on the packed two-seeds-per-lane kernels (bsw_set_rtl_packed) on the GPU.  For each case three things
are byte-equal: the results with the switch on, the results with the switch off in the same process, and
tests/ksw_extend_rtl_ref.c.  bsw_rtl_packed_stats proves which kernel ran: the counter of every expected instantiation grows
with the switch on, and none grows with it off."""
import numpy as np
import pytest

import _gen
import _kernel_ledger as L
import _rtl_ref as R
from test_gpu_variant_rtl import FIELDS, assert_same

pytestmark = pytest.mark.gpu

RTL = 2
C72S, C72A, C136S, C136A = 0, 1, 2, 3          # bsw_rtl_packed_stats: 72 columns shared / separate penalties, 136 shared / separate
ASYM = dict(o_del=5, e_del=2, o_ins=7, e_ins=1)


@pytest.fixture(scope="module")
def lane_ctx(host):
    c = host.BswContext(device=0, kernel=host.KERNEL_LANE)       # lane lists whatever the batch size
    yield c
    c.close()


def on_off(host, run, expect, none_other=True):
    """run() with the switch off, then on: (off, on) results.  Off: no counter moves.  On: every counter of `expect` grows,
    and (none_other) no other one does."""
    assert not host.rtl_packed()
    s0 = host.rtl_packed_stats()
    off = run()
    s1 = host.rtl_packed_stats()
    host.set_rtl_packed(True)
    try:
        assert host.rtl_packed()
        on = run()
    finally:
        host.set_rtl_packed(False)
    s2 = host.rtl_packed_stats()
    print("rtl_packed_stats: off %s on %s" % ([b - a for a, b in zip(s0, s1)], [b - a for a, b in zip(s1, s2)]))
    assert s1 == s0
    for k in range(4):
        if k in expect:
            assert s2[k] > s1[k], (k, s1, s2)
        elif none_other:
            assert s2[k] == s1[k], (k, s1, s2)
    return off, on


def check_pairs(host, ctx, p, tasks, expect, none_other=True):
    want = R.pair_batch(p, tasks)
    off, on = on_off(host, lambda: ctx.extend_pairs(p, tasks).copy(), expect, none_other)
    assert_same(on, want)
    assert_same(off, want)
    assert on.tobytes() == off.tobytes()
    return want


@pytest.mark.parametrize("cls,pen", [(72, "shared"), (72, "separate"), (136, "shared"), (136, "separate")])
def test_each_instantiation(host, lane_ctx, cls, pen):
    """a class's own lengths — a third of the seeds at its last column (71 / 135), some at qlen 1 — with one-sided seeds, Ns in
    queries and targets, and half of the seeds at the 8-bit bound h0 + (lq + rq) a + b = 255"""
    rng = np.random.default_rng(cls + len(pen))
    band = (1, 71) if cls == 72 else (72, 135)
    sd = L.seeds(rng, 900, [band, band, band, (1, 1)] if cls == 136 else [band, band, band, (1, 2)], bits=8, nrate=0.01)
    tasks, arena = host.make_tasks(sd)
    assert (tasks["lqlen"] == 0).any() and (tasks["rqlen"] == 0).any()
    qm = np.maximum(tasks["lqlen"], tasks["rqlen"])
    assert (qm == band[1]).sum() > 50 and ((tasks["lqlen"] == 1) | (tasks["rqlen"] == 1)).sum() > 20
    assert (tasks["h0"].astype(np.int64) + tasks["lqlen"] + tasks["rqlen"] + 4 == 255).sum() > 100
    p = host.default_params(variant=RTL, **(ASYM if pen == "separate" else {}))
    k = (C72S if cls == 72 else C136S) + (pen == "separate")
    want = check_pairs(host, lane_ctx, p, tasks, {k}, none_other=False)
    assert int(want["score"].max()) == 255 - 4


@pytest.mark.parametrize("n", [1, 127, 128, 129, 513])
def test_list_lengths(host, lane_ctx, n):
    """right sides only, so a list is n long: empty slots (1, 127), a full wavefront (128), a lane with only its first seed
    (129), two workgroups (513)"""
    seeds = _gen.random_seeds(np.random.default_rng(n), n, qmin=1, qmax=71, h0max=60, both_sides=False, nrate=0.005)
    tasks, arena = host.make_tasks(seeds)
    check_pairs(host, lane_ctx, host.default_params(variant=RTL), tasks, {C72S})


def test_band_retry_and_zdrop(host, lane_ctx):
    """w = 10 with three band tries: sides go through the redo list; zdrop 40 ends extensions early"""
    rng = np.random.default_rng(7)
    sd = L.seeds(rng, 1200, [(1, 71), (72, 135)], bits=8, nrate=0.005, indel=0.05)
    tasks, arena = host.make_tasks(sd)
    p = host.default_params(variant=RTL, w=10, max_band_try=3, zdrop=40)
    want = check_pairs(host, lane_ctx, p, tasks, {C136S}, none_other=False)       # (a chunk of mostly long sides folds the 72-column class into the 136-column one)
    assert int((want["left"]["aw"] > 10).sum() + (want["right"]["aw"] > 10).sum()) > 20
    h = R.pair_batch(R.with_variant(p, 0), tasks)
    assert R.sides_differ(want, h).sum() >= 10                   # the workload tells RTL from H


def test_chunk_with_wide_and_16bit_seeds(host, lane_ctx):
    """232-column and 16-bit seeds in the same chunk stay on bsw_lane_kernel; the narrow classes take the packed kernel"""
    rng = np.random.default_rng(8)
    sd = L.seeds(rng, 1500, [(1, 71), (72, 135), (136, 231)], bits=8, share16=0.2)
    tasks, arena = host.make_tasks(sd)
    top = tasks["h0"].astype(np.int64) + tasks["lqlen"] + tasks["rqlen"] + 4
    assert (top > 255).sum() > 100 and (np.maximum(tasks["lqlen"], tasks["rqlen"]) > 135).sum() > 100
    check_pairs(host, lane_ctx, host.default_params(variant=RTL), tasks, {C136S}, none_other=False)


def test_upload_run_download_and_packed_input(host, lane_ctx):
    tasks, arena = host.make_tasks(L.seeds(np.random.default_rng(9), 1000, [(1, 71), (72, 135)], bits=8))
    p = host.default_params(variant=RTL)
    want = R.pair_batch(p, tasks)

    def resident():
        b = lane_ctx.upload(p, tasks)
        lane_ctx.run(b)
        lane_ctx.sync()
        got = lane_ctx.download(b)[:len(tasks)].copy()
        b.free()
        return got
    off, on = on_off(host, resident, {C136S}, none_other=False)
    assert_same(on, want)
    assert on.tobytes() == off.tobytes()
    ptasks, pk = host.pack_tasks(tasks)
    off, on = on_off(host, lambda: lane_ctx.extend_pairs_packed(p, ptasks).copy(), {C136S}, none_other=False)
    assert_same(on, want)
    assert on.tobytes() == off.tobytes()


def test_pair_result_format(host):
    tasks, arena = host.make_tasks(L.seeds(np.random.default_rng(10), 800, [(1, 71)], bits=8))
    p = host.default_params(variant=RTL)
    want = R.pair_batch(p, tasks)
    with host.BswContext(device=0, kernel=host.KERNEL_LANE, result_format=host.RESULT_PAIR) as c:
        off, on = on_off(host, lambda: c.extend_pairs(p, tasks).copy(), {C72S})
    assert on.tobytes() == off.tobytes()
    for f in FIELDS:
        assert (on[f] == want[f]).all(), f


def test_resident_reference(host, lane_ctx):
    from test_gpu_ref import _reads_and_seeds
    rng = np.random.default_rng(11)
    genome = rng.integers(0, 4, 100000).astype(np.uint8)
    lp = len(genome)
    pac = host.pack_pac(genome)
    n = 1500
    reads, seeds = _reads_and_seeds(host, rng, genome, n)
    p = host.default_params(variant=RTL)
    tasks, keep = host.seeds_to_tasks(p, pac, lp, reads, seeds)
    want = R.pair_batch(p, tasks)
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
    ref = lane_ctx.ref_upload(pac, lp)
    try:
        off, on = on_off(host, lambda: lane_ctx.extend_ref(p, ref, rt)[:n].copy(), {C136S}, none_other=False)
    finally:
        lane_ctx.ref_free(ref)
    assert_same(on, want)
    assert on.tobytes() == off.tobytes()


def test_reference_wire_format(host, lane_ctx):
    """bsw_refbatch_run(…, BSW_VARIANT_RTL, …) builds its lane lists through launch_lane like every other batch"""
    tasks, arena = host.synth_tasks(800, seed=31, seed_at_start=0, seed_len_min=19, seed_len_max=60, indel_rate=0.01, junk_frac=0.1)
    words, n = host.refbatch_encode(host.default_params(), tasks)
    want = R.pair_batch(host.default_params(zdrop=0, variant=RTL), tasks[:n])

    def wire():
        out, nres = lane_ctx.refbatch_run(words, variant=RTL, zdrop=0)
        assert nres == n
        return host.refbatch_decode_results(out, n)
    off, on = on_off(host, wire, {C136S}, none_other=False)
    assert on.tobytes() == off.tobytes()
    for f in FIELDS:
        assert (on[f] == want[f]).all(), f


@pytest.mark.parametrize("variant", [0, 1])
def test_h_and_m_are_untouched(host, oracle, lane_ctx, variant):
    tasks, arena = host.make_tasks(L.seeds(np.random.default_rng(12 + variant), 1000, [(1, 71), (72, 135)], bits=8))
    p = host.default_params(variant=variant)
    off, on = on_off(host, lambda: lane_ctx.extend_pairs(p, tasks).copy(), set())
    assert on.tobytes() == off.tobytes()
    assert_same(on, oracle.pair_batch(p, tasks, nthreads=4))
