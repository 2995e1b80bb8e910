"""The right edge of the two-seeds-per-lane block bodies, on the CPU model (tests/lane2_model.cpp over bsw_lane2_core.h).

The edge body forces H to 0 at the columns j >= end and lets everything else run unmasked; it relies on the right-edge
invariant of bsw_lane2_core.h (eh[j].e == 0 for j >= end when a row starts) and keeps the entries beyond `end` as they
are, because the first row leaves h values there when the w clip cuts it short (qlen >= w + 2 and
h0 > oe_ins + (w + 1) e_ins) and bwa reads them once `end` reaches them.  These cases aim at exactly that: the w clip on
both sides of its boundary, `end` shrinking after long rows, zdrop / m == 0 stops, `end` at qlen and inside the ragged
last block, a query N in the `end` block, variant M and separate gap penalties.  Every output field is compared with
the oracle, the cell count included."""
import os
import subprocess

import numpy as np
import pytest

import _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTF = ["score", "qle", "tle", "gtle", "gscore", "max_off", "aw", "cells"]
KINDS = {"unrolled": 135, "unrolled9": 71, "loop17": 135, "loop29": 231, "group3": 191, "group4": 231}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    import ctypes as C
    so = str(tmp_path_factory.mktemp("l2re") / "lane2_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "lane2_model.cpp")])
    L = C.CDLL(so)
    for name, extra in (("lane2_model_run", []), ("lane2_model_run_qb", [C.c_int]), ("lane2l_model_run", [C.c_int]),
                        ("lane2g_model_run", [C.c_int])):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + extra
    return L


def run_model(lib, kind, *a):
    if kind == "unrolled":
        return lib.lane2_model_run(*a)
    if kind == "unrolled9":
        return lib.lane2_model_run_qb(*a, 9)
    if kind in ("group3", "group4"):
        return lib.lane2g_model_run(*a, 3 if kind == "group3" else 4)
    return lib.lane2l_model_run(*a, 29 if kind == "loop29" else 17)


def first_row_clipped(qlen, h0, w, oe_ins, e_ins):
    """The first row leaves non-zero h beyond its `end` = w + 1 (bwa's init loop, ksw_extend2)."""
    return qlen >= w + 2 and h0 > oe_ins + (w + 1) * e_ins


def check_side(lib, kind, host, oracle, p, tasks, side, h0s=None):
    qcap = KINDS[kind]
    qf = "rqlen" if side else "lqlen"
    idx = np.nonzero((tasks[qf] > 0) & (tasks[qf] <= qcap))[0]
    if len(idx) == 0:
        return idx
    order = idx[np.argsort(-tasks[qf][idx], kind="stable")].astype(np.uint32)
    got = np.zeros(len(tasks), dtype=host.EXT)
    rc = run_model(lib, kind, p.ctypes.data, tasks.ctypes.data, side, order.ctypes.data, len(order),
                   h0s.ctypes.data if h0s is not None else None, got.ctypes.data)
    assert rc == 0
    et = np.zeros(len(tasks), dtype=host.EXT_TASK)
    pre = "r" if side else "l"
    et["query"], et["target"] = tasks[pre + "query"], tasks[pre + "target"]
    et["qlen"], et["tlen"] = tasks[pre + "qlen"], tasks[pre + "tlen"]
    et["w"], et["end_bonus"] = int(p["w"][0]), int(p["pen_clip3" if side else "pen_clip5"][0])
    et["h0"] = tasks["h0"] if h0s is None else h0s
    want = oracle.ext_batch(p, et, nthreads=4)
    for f in EXTF:
        bad = np.nonzero(got[f][idx] != want[f][idx])[0]
        assert bad.size == 0, "%s side %d field %s: task %s got %s want %s" % (
            kind, side, f, idx[bad[:4]], got[f][idx[bad[:4]]], want[f][idx[bad[:4]]])
    return idx


def cap_h0(seeds, b=4, a=1):
    for s in seeds:                                       # the 8-bit class bound: h0 + qlen * a + b <= 255
        tot = len(s.get("lq", ())) + len(s.get("rq", ()))
        s["h0"] = max(1, min(s["h0"], 255 - b - tot * a))
    return seeds


def edge_seeds(rng, n, qcap, nq=False):
    """Shapes that move `end` around: a query that matches its target for a while and then not at all (the range opens,
    then shrinks back), perfect matches (end runs into qlen), query lengths on both sides of a multiple of 8, and (nq)
    an N a few columns before the query's end."""
    seeds = []
    for k in range(n):
        s = {"h0": int(rng.integers(1, 70)), "init_score": -1, "tag": k}
        for side in ("l", "r"):
            if side == "l" and rng.random() < 0.3:
                continue
            m = int(rng.integers(1, qcap // 8 + 1)) * 8
            ql = int(np.clip(m + int(rng.integers(-2, 3)), 1, qcap))
            kind = k % 3
            q = rng.integers(0, 4, ql).astype(np.uint8)
            if kind == 0:                                 # matches for a while, then junk: end grows, then is trimmed
                cut = int(rng.integers(1, ql + 1))
                t = np.concatenate([q[:cut], rng.integers(0, 4, int(rng.integers(ql, 2 * ql + 2))).astype(np.uint8)])
            elif kind == 1:                               # the query end to end: end reaches qlen and stays there
                t = np.concatenate([q, rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8)])
            else:                                         # mutated, with indels
                t = rng.integers(0, 4, int(ql * 1.5) + 2).astype(np.uint8)
                q = _gen.mutate(rng, t, ql, 0.05, 0.04)
            if nq and ql > 3 and rng.random() < 0.5:
                q = q.copy()
                q[ql - 1 - int(rng.integers(0, min(ql, 8)))] = 4
            s[side + "q"], s[side + "t"] = q, t
        if "lq" not in s and "rq" not in s:
            continue
        seeds.append(s)
    return seeds


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("w", [1, 5, 37])
def test_first_row_clip_on_both_sides_of_its_boundary(lib, host, oracle, kind, w):
    """h0 just below, at and above oe_ins + (w + 1) e_ins: above it, the first row leaves h values beyond its `end` that
    later rows read as H(i-1, j-1); the edge body must keep them."""
    rng = np.random.default_rng(1000 + w + 7 * len(kind))
    p = host.default_params(w=w)
    oe_ins, e_ins = int(p["o_ins"][0]) + int(p["e_ins"][0]), int(p["e_ins"][0])
    bound = oe_ins + (w + 1) * e_ins
    qcap = KINDS[kind]
    seeds = []
    for k in range(240):
        ql = int(rng.integers(w + 2, max(w + 3, min(qcap, 255 - 4 - 1 - bound - 6) + 1)))
        h0 = bound + int(rng.integers(-3, 7))
        q = rng.integers(0, 4, ql).astype(np.uint8)
        t = np.concatenate([q[:int(rng.integers(0, ql + 1))], rng.integers(0, 4, int(rng.integers(w, 3 * w + 40))).astype(np.uint8)])
        seeds.append({"h0": max(1, h0), "rq": q, "rt": t, "init_score": -1, "tag": k})
    seeds = cap_h0(seeds)
    tasks, arena = host.make_tasks(seeds)
    clipped = np.array([first_row_clipped(int(q), int(h), w, oe_ins, e_ins) for q, h in zip(tasks["rqlen"], tasks["h0"])])
    sel = (tasks["rqlen"] <= qcap)
    assert clipped[sel].sum() > 40 and (~clipped[sel]).sum() > 40      # both sides of the boundary are populated
    check_side(lib, kind, host, oracle, p, tasks, 1)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("over", [
    dict(), dict(zdrop=5), dict(zdrop=20, w=9), dict(w=3, zdrop=0),
    dict(variant=1), dict(variant=1, zdrop=15, w=6),
    dict(o_del=6, e_del=1, o_ins=4, e_ins=2), dict(variant=1, o_del=3, e_del=2, o_ins=8, e_ins=1, w=11),
])
def test_edge_shapes_match_the_oracle(lib, host, oracle, kind, over):
    rng = np.random.default_rng(abs(hash((kind, str(sorted(over.items()))))) % (2 ** 31))
    p = host.default_params(**over)
    for nq in (False, True):
        seeds = cap_h0(edge_seeds(rng, 260, KINDS[kind], nq=nq))
        tasks, arena = host.make_tasks(seeds)
        check_side(lib, kind, host, oracle, p, tasks, 0)
        check_side(lib, kind, host, oracle, p, tasks, 1)


@pytest.mark.parametrize("kind", ["unrolled", "loop29", "group4"])
def test_m_zero_stops_and_junk(lib, host, oracle, kind):
    """Unrelated queries: most rows reach m == 0 early (:1942) or zdrop stops them, with `end` collapsing to beg + 1."""
    rng = np.random.default_rng(31)
    seeds = cap_h0(_gen.random_seeds(rng, 500, qmin=1, qmax=KINDS[kind], tfac=2.5, sub=0.2, indel=0.05, junk=0.7, h0max=12))
    tasks, arena = host.make_tasks(seeds)
    for over in (dict(), dict(zdrop=3), dict(variant=1, zdrop=3)):
        p = host.default_params(**over)
        check_side(lib, kind, host, oracle, p, tasks, 0)
        check_side(lib, kind, host, oracle, p, tasks, 1)
