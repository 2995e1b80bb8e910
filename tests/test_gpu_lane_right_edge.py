"""The right edge of the two-seeds-per-lane block bodies on the GPU (the asm bodies of bsw_lane2_body_asm.inc): the shapes of
tests/test_lane2_right_edge_cpu.py through the C ABI, against the oracle — the 136-column class (bsw_lane2_kernel<17,2>),
the 72-column class (<9,3>, chosen when a chunk holds no wider side), 250 bp queries (bsw_lane2l_kernel) and a mid-sized
chunk under BSW_KERNEL_AUTO (the group kernel, both sides in one launch)."""
import numpy as np
import pytest

from test_gpu_parity import assert_same
from test_lane2_right_edge_cpu import cap_h0, edge_seeds

pytestmark = pytest.mark.gpu


def clip_seeds(rng, n, w, qmin, qmax, oe_ins=7, e_ins=1):
    """Both sides with h0 around oe_ins + (w + 1) e_ins and qlen >= w + 2: the first row leaves h values beyond its `end`."""
    bound = oe_ins + (w + 1) * e_ins
    seeds = []
    for k in range(n):
        s = {"h0": max(1, bound + int(rng.integers(-3, 7))), "init_score": -1, "tag": k}
        for side in ("l", "r"):
            ql = int(rng.integers(max(qmin, w + 2), max(qmin, w + 2, qmax) + 1))
            q = rng.integers(0, 4, ql).astype(np.uint8)
            t = np.concatenate([q[:int(rng.integers(0, ql + 1))], rng.integers(0, 4, int(rng.integers(w, 3 * w + 40))).astype(np.uint8)])
            s[side + "q"], s[side + "t"] = q, t
        seeds.append(s)
    return seeds


@pytest.fixture(scope="module")
def lctx(host):
    c = host.BswContext(device=0, kernel=host.KERNEL_LANE)
    yield c
    c.close()


@pytest.mark.parametrize("qr", [(3, 34), (40, 65), (72, 130), (140, 230)])     # 72-column class / 136-column class / looped kernel
@pytest.mark.parametrize("w", [1, 5, 37])
def test_first_row_clip(host, oracle, lctx, w, qr):
    rng = np.random.default_rng(w * 1000 + qr[1])
    seeds = clip_seeds(rng, 1500, w, *qr)
    for s in seeds:                                       # 8-bit lane class: h0 + (lqlen + rqlen) a + b <= 255
        s["h0"] = max(1, min(s["h0"], 255 - 4 - len(s["lq"]) - len(s["rq"])))
    tasks, arena = host.make_tasks(seeds)
    p = host.default_params(w=w)
    assert_same(lctx.extend_pairs(p, tasks), oracle.pair_batch(p, tasks, nthreads=8), tasks)


@pytest.mark.parametrize("over", [dict(), dict(zdrop=5), dict(w=3, zdrop=0), dict(variant=1, zdrop=15, w=6),
                                  dict(o_del=6, e_del=1, o_ins=4, e_ins=2), dict(variant=1, o_del=3, e_del=2, o_ins=8, e_ins=1, w=11)])
@pytest.mark.parametrize("qcap", [71, 135, 231])
def test_edge_shapes(host, oracle, lctx, over, qcap):
    rng = np.random.default_rng(qcap + len(str(over)))
    seeds = cap_h0(edge_seeds(rng, 1200, qcap, nq=False) + edge_seeds(rng, 300, qcap, nq=True))
    tasks, arena = host.make_tasks(seeds)
    p = host.default_params(**over)
    assert_same(lctx.extend_pairs(p, tasks), oracle.pair_batch(p, tasks, nthreads=8), tasks)


@pytest.mark.parametrize("w", [5, 37])
def test_mid_sized_chunk_auto(host, oracle, w):
    """A chunk of ~40 k seeds under BSW_KERNEL_AUTO runs the group kernel with both sides of a seed in one launch."""
    rng = np.random.default_rng(77 + w)
    seeds = clip_seeds(rng, 20000, w, 10, 60) + cap_h0(edge_seeds(rng, 20000, 60))
    for s in seeds:
        s["h0"] = max(1, min(s["h0"], 255 - 4 - len(s.get("lq", ())) - len(s.get("rq", ()))))
    tasks, arena = host.make_tasks(seeds)
    p = host.default_params(w=w)
    with host.BswContext(device=0, kernel=host.KERNEL_AUTO) as c:
        got = c.extend_pairs(p, tasks)
    assert_same(got, oracle.pair_batch(p, tasks, nthreads=8), tasks)
