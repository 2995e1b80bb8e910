"""Variant RTL on the two-seeds-per-lane formulation, verified on the CPU: tests/lane2_rtl_model.cpp drives lane2r of
csrc/bsw_lane2_core.h — the row bsw_lane2_rtl_kernel is compiled from — and must agree with tests/ksw_extend_rtl_ref.c on
every field of every side record, the cell counts included.  Each case also runs the unchanged variant-H model path against
the same reference under H, and the module checks that its workload tells RTL from H at all."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _gen
import _rtl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTF = _rtl_ref.EXTF
QLENS = {9: (1, 7, 8, 9, 16, 17, 63, 64, 65, 71), 17: (72, 73, 127, 128, 129, 135)}
GEN_SEED = 2      # the generator seed: chosen so that the reference alone meets the RTL-vs-H counts below (checked there)


@pytest.fixture(scope="module")
def model_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("l2r") / "lane2_rtl_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "lane2_rtl_model.cpp")])
    L = C.CDLL(so)
    args = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    L.lane2_rtl_model_run.restype = C.c_int
    L.lane2_rtl_model_run.argtypes = args
    L.lane2_model_run_qb.restype = C.c_int
    L.lane2_model_run_qb.argtypes = args
    L.lane2_rtl_model_stats.restype = None
    L.lane2_rtl_model_stats.argtypes = [C.c_void_p, C.c_int]
    return L


def class_seeds(qb, seed):
    """Seeds of one lane class: the class's edge lengths and random ones, Ns, junk queries and junk flanks, one-sided
    seeds, and seeds at the 8-bit bound h0 + (lq + rq) a + b = 255 (a = 1, b = 4)."""
    rng = np.random.default_rng(seed * 100 + qb)
    lo, hi = (1, 71) if qb == 9 else (72, 135)
    seeds = []
    for k in range(320):
        rq = int(QLENS[qb][k % len(QLENS[qb])]) if k % 2 == 0 else int(rng.integers(lo, hi + 1))
        lq = 0 if k % 5 == 0 else int(rng.integers(lo, min(hi, 250 - rq) + 1))      # (lq + rq <= 250: h0 >= 1 fits the 8 bits)
        if k % 11 == 0 and lq:
            lq, rq = rq, 0                                  # a seed without a right side
        s = {}
        for side, ql in (("l", lq), ("r", rq)):
            if ql == 0:
                continue
            tl = int(rng.integers(max(1, ql // 2), int(ql * 2.2) + 2))
            t = rng.integers(0, 4, tl).astype(np.uint8)
            kind = rng.random()
            if kind < 0.12:
                q = rng.integers(0, 4, ql).astype(np.uint8)                      # junk
            else:
                q = _gen.mutate(rng, t, ql, 0.04, 0.03)
                if kind < 0.4:                                                   # junk flank: the tail matches nothing
                    cut = int(rng.integers(ql // 3, ql + 1))
                    q[cut:] = rng.integers(0, 4, ql - cut)
            if k % 3 == 0:
                q[rng.random(ql) < 0.01] = 4
                t[rng.random(tl) < 0.01] = 4
            s[side + "q"], s[side + "t"] = q, t
        tot = lq + rq
        s["h0"] = 255 - 4 - tot if k % 4 == 0 else int(rng.integers(1, min(60, 255 - 4 - tot) + 1))
        if k % 8 == 0:                                      # at the bound AND matching end to end: the top score is reached
            for side in ("l", "r"):
                if side + "q" in s:
                    q = rng.integers(0, 4, len(s[side + "q"])).astype(np.uint8)
                    s[side + "q"], s[side + "t"] = q, np.concatenate([q, rng.integers(0, 4, 20).astype(np.uint8)])
        s["init_score"] = -1 if rng.random() < 0.8 else int(rng.integers(-1, 50))
        s["tag"] = int(rng.integers(0, 2 ** 32))
        seeds.append(s)
    return seeds


@pytest.fixture(scope="module")
def workloads(host):
    return {qb: host.make_tasks(class_seeds(qb, GEN_SEED)) for qb in (9, 17)}


def model_pairs(run, host, p, tasks, qb):
    """Both sides of every seed through the model, with side_ref's band retries around it (the kernel runs one try; the
    redo list runs the rest on the device): left / right EXT records as pair_ref leaves them."""
    n = len(tasks)
    res = {"left": np.zeros(n, dtype=host.EXT), "right": np.zeros(n, dtype=host.EXT)}
    tries = max(int(p["max_band_try"][0]), 1)
    score = tasks["init_score"].astype(np.int64)
    for side, name, qf in ((0, "left", "lqlen"), (1, "right", "rqlen")):
        h0s = (tasks["h0"] if side == 0 else np.where(tasks["lqlen"] > 0, res["left"]["score"], tasks["h0"])).astype(np.int32)
        if side == 1:
            score = h0s.astype(np.int64)
        todo = np.nonzero(tasks[qf] > 0)[0]
        cells = np.zeros(n, np.uint64)
        for k in range(tries):
            if len(todo) == 0:
                break
            pk = p.copy()
            pk["w"] = int(p["w"][0]) << k
            order = todo[np.argsort(-tasks[qf][todo], kind="stable")].astype(np.uint32)
            out = np.zeros(n, dtype=host.EXT)
            assert run(pk.ctypes.data, tasks.ctypes.data, side, order.ctypes.data, len(order), h0s.ctypes.data, out.ctypes.data, qb) == 0
            cells[todo] += out["cells"][todo]
            res[name][todo] = out[todo]
            res[name]["cells"][todo] = cells[todo].astype(np.uint32)
            aw = int(pk["w"][0])
            done = (out["score"][todo] == score[todo]) | (out["max_off"][todo] < (aw >> 1) + (aw >> 2))
            score[todo] = out["score"][todo]
            todo = todo[~done]
    return res


def compare(got, want, tasks, what):
    for name, qf in (("left", "lqlen"), ("right", "rqlen")):
        sel = np.nonzero(tasks[qf] > 0)[0]
        for f in EXTF:
            bad = sel[got[name][f][sel] != want[name][f][sel]]
            assert bad.size == 0, "%s %s.%s: task %s got %s want %s" % (what, name, f, bad[:4], got[name][f][bad[:4]], want[name][f][bad[:4]])


PEN = {"shared": dict(), "separate": dict(o_del=5, e_del=2, o_ins=7, e_ins=1)}


@pytest.mark.parametrize("pen", ["shared", "separate"])
@pytest.mark.parametrize("zdrop", [0, 10, 100])
@pytest.mark.parametrize("w", [1, 5, 10, 100])
@pytest.mark.parametrize("qb", [9, 17])
def test_rtl_row_matches_the_reference(model_lib, host, workloads, qb, w, zdrop, pen):
    tasks, arena = workloads[qb]
    p = host.default_params(w=w, zdrop=zdrop, max_band_try=3, variant=_rtl_ref.VARIANT_RTL, **PEN[pen])
    compare(model_pairs(model_lib.lane2_rtl_model_run, host, p, tasks, qb), _rtl_ref.pair_batch(p, tasks), tasks, "RTL")
    # the unchanged variant-H path of the same header, same case: the RTL additions did not move it
    pH = _rtl_ref.with_variant(p, _rtl_ref.VARIANT_H)
    compare(model_pairs(model_lib.lane2_model_run_qb, host, pH, tasks, qb), _rtl_ref.pair_batch(pH, tasks), tasks, "H")


def test_workload_tells_rtl_from_h_and_reaches_the_edges(model_lib, host, workloads):
    """The reference alone: under RTL and under H at least 10 sides differ in some field and at least 10 in `cells`, so a
    model that computed variant H would fail above.  And the model's own counters: lanes whose two seeds had different beg
    (end) inside one 8-column block, lanes whose seeds stopped many rows apart, and the 8-bit bound was reached."""
    any_f = cells = 0
    top = 0
    stats = np.zeros(3, np.uint64)
    model_lib.lane2_rtl_model_stats(stats.ctypes.data, 1)
    for qb in (9, 17):
        tasks, arena = workloads[qb]
        p = host.default_params(w=100, zdrop=100, max_band_try=3, variant=_rtl_ref.VARIANT_RTL)
        r = _rtl_ref.pair_batch(p, tasks)
        h = _rtl_ref.pair_batch(_rtl_ref.with_variant(p, _rtl_ref.VARIANT_H), tasks)
        any_f += int(_rtl_ref.sides_differ(r, h).sum())
        cells += int(_rtl_ref.sides_differ(r, h, ("cells",)).sum())
        top = max(top, int(r["score"].max()))
        model_pairs(model_lib.lane2_rtl_model_run, host, p, tasks, qb)
    model_lib.lane2_rtl_model_stats(stats.ctypes.data, 1)
    print("sides differing RTL vs H: any field %d, cells %d; top score %d; model counters %s" % (any_f, cells, top, stats))
    assert any_f >= 10 and cells >= 10
    assert top == 255 - 4
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0


def test_ragged_and_tiny_waves(model_lib, host, workloads):
    """list lengths around the wave's 64 / 128 slots: empty slots, a lane with only its first seed"""
    tasks, arena = workloads[9]
    p = host.default_params(w=10, zdrop=40, max_band_try=3, variant=_rtl_ref.VARIANT_RTL)
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        compare(model_pairs(model_lib.lane2_rtl_model_run, host, p, tasks[:n], 9), _rtl_ref.pair_batch(p, tasks[:n]), tasks[:n], "RTL n=%d" % n)
