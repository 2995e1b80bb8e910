"""The half-block skips of the two-seeds-per-lane kernel's N-free block bodies on the GPU (the block8h_asm statements of
bsw_lane2_body_asm.inc): the shapes of tests/test_lane2_half_blocks_cpu.py through the C ABI against the oracle, bit for bit —
the 136-column class (<17,2>) and the 72-column class (bsw_lane2_kernel<9,3>, chosen when a chunk holds no wider side; it keeps
its whole-block bodies and runs the same shapes through them), a
chunk large enough for the fused instantiation (left sides, then right sides from their scores, in one launch) and a list
that ends one wavefront short of a full wave."""
import numpy as np
import pytest

from test_gpu_parity import assert_same
from test_lane2_half_blocks_cpu import OVERS, half_seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lctx(host):
    c = host.BswContext(device=0, kernel=host.KERNEL_LANE)
    yield c
    c.close()


def shapes(host, p, qcap, seed, **kw):
    rng = np.random.default_rng(seed)
    seeds = half_seeds(rng, qcap, int(p["w"][0]), int(p["o_ins"][0]) + int(p["e_ins"][0]), int(p["e_ins"][0]), **kw)
    return host.make_tasks(seeds)


@pytest.mark.parametrize("qcap", [71, 135])
@pytest.mark.parametrize("over", OVERS, ids=lambda o: "-".join("%s%s" % kv for kv in sorted(o.items())) or "default")
def test_half_block_shapes(host, oracle, lctx, over, qcap):
    p = host.default_params(**over)
    tasks, arena = shapes(host, p, qcap, qcap + len(str(over)))
    assert 2000 <= len(tasks) <= 4000
    assert_same(lctx.extend_pairs(p, tasks), oracle.pair_batch(p, tasks, nthreads=8), tasks)


@pytest.mark.parametrize("over", [dict(), dict(variant=1, w=5)], ids=["default", "variant1-w5"])
def test_fused_chunk(host, oracle, over):
    """Past the group kernel's range BSW_KERNEL_AUTO runs both sides of a seed in one launch of the lane kernel's fused
    instantiation: the right side's first row starts from the score the left side just found."""
    p = host.default_params(**over)
    tasks, arena = shapes(host, p, 135, 7)
    tasks = np.concatenate([tasks] * (52_000 // len(tasks) + 1))
    tasks["tag"] = np.arange(len(tasks), dtype=np.uint32)
    tasks = tasks[np.random.default_rng(3).permutation(len(tasks))]
    with host.BswContext(device=0, kernel=host.KERNEL_AUTO) as c:
        got = c.extend_pairs(p, tasks)
    assert_same(got, oracle.pair_batch(p, tasks, nthreads=8), tasks)


def test_list_short_by_a_wavefront(host, oracle, lctx):
    """A right list of 128 k + 64 seeds: the last wave runs with one seed per lane, its high halves never active."""
    p = host.default_params()
    tasks, arena = shapes(host, p, 135, 11, both=False)
    tasks = tasks[:len(tasks) // 128 * 128 - 64]
    assert len(tasks) % 128 == 64 and (tasks["lqlen"] == 0).all()
    assert_same(lctx.extend_pairs(p, tasks), oracle.pair_batch(p, tasks, nthreads=8), tasks)
