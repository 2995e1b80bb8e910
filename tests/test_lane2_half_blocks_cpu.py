"""The half-block skips of the two-seeds-per-lane kernel's N-free block bodies (lane2::block8h), on the CPU model.

A row's first block is entered at column 4 when its columns 0..3 lie left of every active seed's beg, its last block is left
after column 3 when its columns 4..7 lie right of every active seed's `end` column.  tests/lane2_half_model.cpp is the CPU
model with the kernel's choice of block bodies (the default model runs the column-by-column bodies at every ragged first
and last block, which leaves the skips almost nothing) and counts what the rows reach; the shapes below are built so that
whole waves move their [beg, end) ranges together — jlo & 7 and jhi & 7 take every value, the first block is the last one,
the first block is an edge block, the band clamp moves beg (w = 1, 5), the first row is clipped by w — for variants H and
M, shared and separate gap penalties, the 9- and the 17-block class (the 9-block class takes no skip: the same shapes
through its whole-block bodies).  Every output field of every seed, the cell count
included, must equal the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _gen
from test_lane2_right_edge_cpu import cap_h0, check_side

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QCAP = {"unrolled": 135, "unrolled9": 71}
OVERS = [dict(), dict(w=1), dict(w=5), dict(variant=1), dict(variant=1, w=5),
         dict(o_del=6, e_del=1, o_ins=4, e_ins=2), dict(variant=1, o_del=3, e_del=2, o_ins=8, e_ins=1, w=5)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("l2h") / "lane2_half_model.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(ROOT, "tests", "lane2_half_model.cpp")])
    L = C.CDLL(so)
    for name, extra in (("lane2_model_run", []), ("lane2_model_run_qb", [C.c_int]), ("lane2l_model_run", [C.c_int]),
                        ("lane2g_model_run", [C.c_int])):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + extra
    L.lane2_half_stats.restype = None
    L.lane2_half_stats.argtypes = [C.c_void_p, C.c_int]
    return L


def half_seeds(rng, qcap, w, oe_ins=7, e_ins=1, group=128, both=True):
    """Groups of `group` seeds with one query length each (the lists are sorted by query length, so a group fills waves of
    its own and its seeds move their ranges together):
      kind 0  the query end to end with a small h0: the range stays a narrow strip along the diagonal, beg and end climb
              a column or so per row and pass every residue mod 8 — the first block is often the last one too;
      kind 1  a match that turns into junk: the range opens, then shrinks to nothing from the left;
      kind 2  mutated with indels: ragged ranges inside a wave;
      kind 3  h0 on both sides of oe_ins + (w + 1) e_ins with qlen >= w + 2: the first row is clipped by w and leaves
              entries beyond its `end`; with a small w the band clamp then moves beg every row;
      kind 4  a mismatch every few bases: the score hovers near zero and the strip is a few columns wide.
    Lengths: one block and less, every residue mod 8 (where `end` stays once it reaches qlen), up to the class's widest row."""
    lens = sorted({3, 7, 8, 9, 10, 12, 17, 21, 23, 30, 31, 36, 44, 52, 63, qcap - 4, qcap} | ({77, 90, 100, 109, 118, 127} if qcap > 71 else set()))
    bound = oe_ins + (w + 1) * e_ins
    seeds, tag = [], 0
    for gi, ql in enumerate(lens):
        kind = gi % 5
        if kind == 3 and ql < w + 2:
            kind = 0
        for k in range(group):
            s = {"init_score": -1, "tag": tag}
            tag += 1
            s["h0"] = {0: 1 + k % 3, 1: 1 + k % 5, 2: 1 + int(rng.integers(0, 30)), 3: max(1, bound + int(rng.integers(-3, 7))), 4: 2 + k % 2}[kind]
            for side in ("r", "l") if both and gi % 2 == 0 else ("r",):
                q = rng.integers(0, 4, ql).astype(np.uint8)
                tail = rng.integers(0, 4, int(rng.integers(ql // 2 + 2, ql + 12))).astype(np.uint8)
                if kind in (0, 3):
                    t = np.concatenate([q, tail])
                elif kind == 1:
                    t = np.concatenate([q[:max(1, (ql * (1 + k % 4)) // 5)], tail])
                elif kind == 2:
                    t = np.concatenate([q, tail])
                    q = _gen.mutate(rng, t, ql, 0.05, 0.04)
                else:
                    t = np.concatenate([q, tail])
                    t[3 + k % 3::5] = (t[3 + k % 3::5] + 1) & 3
                s[side + "q"], s[side + "t"] = q, t
            seeds.append(s)
    return cap_h0(seeds)


def read_stats(lib):
    st = (C.c_ulonglong * 20)()
    lib.lane2_half_stats(st, 1)
    return [int(x) for x in st]


@pytest.mark.parametrize("kind", sorted(QCAP))
@pytest.mark.parametrize("over", OVERS, ids=lambda o: "-".join("%s%s" % kv for kv in sorted(o.items())) or "default")
def test_half_block_skips_match_the_oracle(lib, host, oracle, kind, over):
    rng = np.random.default_rng(len(kind) * 100 + len(str(over)))
    p = host.default_params(**over)
    w = int(p["w"][0])
    seeds = half_seeds(rng, QCAP[kind], w, int(p["o_ins"][0]) + int(p["e_ins"][0]), int(p["e_ins"][0]))
    tasks, arena = host.make_tasks(seeds)
    read_stats(lib)
    n = 0
    for side in (0, 1):
        n += len(check_side(lib, kind, host, oracle, p, tasks, side))
    st = read_stats(lib)
    assert n > 1500
    # the shapes reach what they are built for: every residue of the first and the last column, and every skip
    assert all(x > 0 for x in st[:16]), "rows by jlo & 7: %s, by jhi & 7: %s" % (st[:8], st[8:16])
    if kind == "unrolled":
        assert st[16] > 0 and st[17] > 0, st                  # entered at column 4: a dense first block, an edge first block
        assert st[18] > 0, st                                 # left after column 3
    else:
        assert st[16:19] == [0, 0, 0], st                     # the 9-block class keeps its whole-block bodies
    assert st[19] == 0, st                                    # never both in one block: the first column run lies at or left of the last

