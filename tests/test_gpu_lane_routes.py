"""Seeded fuzz of the kernels a chunk that does not fill the machine runs under BSW_KERNEL_AUTO (about 10 k - 260 k seeds), forced
onto small batches under BSW_KERNEL_LANE with the routing switches (tests/_routes.py):
  group        BSW_GROUP=1 BSW_GROUP_FUSE=0   bsw_lane2g_kernel<3 | 4, ., VM, SYM, false>, a launch per side and class
  group_fused  BSW_GROUP=1 BSW_GROUP_FUSE=1   bsw_lane2g_kernel<3 | 4, ., VM, SYM, true>, left then right sides in one launch
  lane_fused   BSW_GROUP=0 BSW_LANE_FUSE=1    bsw_lane2_kernel<17, 2, VM, SYM, true>
each as is (query Ns stay in the kernels: phase_a<true>) and with BSW_NSPLIT=1 (seeds with a query N go to the general kernel's
list, the lane lists keep unused slots).  Every draw: the route proven on the host plan, the launch count of a resident batch,
and every field — cells included — against the oracle through upload/run/download, a streaming submit and pair records.
The group scan across eight lanes (gshr / gfrom7 / gmax / gmin), the left score handed to the right side of a fused launch and
bsw_pair_decide with the redo list are what the CPU model of these kernels does not run.  The switches are read once per
process: every route runs in a child of its own, one after the other."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
import sys, time
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as g
host, orc = g.load_package().host, g.load_oracle()
import _routes as R
from test_gpu_parity import assert_same
route, nsplit = %(route)r, %(nsplit)d
t0 = time.time()
tally = R.Tally()
with host.BswContext(device=0, kernel=host.KERNEL_LANE) as c, \
        host.BswContext(device=0, kernel=host.KERNEL_LANE, result_format=host.RESULT_PAIR) as cp:
    for over, mat, seeds, wide in R.draws(route, %(ndraws)d, %(n)d, %(seed)d):
        p = R.make_params(host, over, mat)
        tasks, arena = host.make_tasks(seeds)
        info = R.prove_route(host, p, tasks, seeds, route, nsplit)
        want = orc.pair_batch(p, tasks, nthreads=8)
        nz = None
        if over["zdrop"] > 0:
            nz = orc.pair_batch(R.make_params(host, dict(over, zdrop=0), mat), tasks, nthreads=8)
        b = c.upload(p, tasks); c.run(b); c.sync()
        got, launches = c.download(b), b.info()["launches"]
        b.free()
        assert launches == info["launches"], (launches, info["launches"], over, mat)
        assert_same(got, want, tasks)
        assert_same(c.extend_pairs(p, tasks), want, tasks)
        gp = cp.extend_pairs(p, tasks)
        for f in R.FIELDS:
            assert (gp[f] == want[f]).all(), f
        tally.add(p, info, want, nz)
tally.check(route, nsplit)
print(route, "nsplit" if nsplit else "", tally, "seconds %%.1f" %% (time.time() - t0))
print("ok")
"""

CASES = [(route, nsplit) for route in ("group", "group_fused", "lane_fused") for nsplit in (0, 1)]


def run_route(route, nsplit, ndraws=16, n=4000, timeout=300):
    from _routes import child_env
    seed = 31000 + 10 * CASES.index((route, nsplit))
    src = SNIPPET % dict(root=ROOT, route=route, nsplit=nsplit, ndraws=ndraws, n=n, seed=seed)
    out = subprocess.run([sys.executable, "-c", src], env=child_env(os.environ, route, nsplit), capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("route,nsplit", CASES, ids=["%s-%s" % (r, "nsplit" if s else "inkernel") for r, s in CASES])
def test_route_fuzz(route, nsplit):
    print(run_route(route, nsplit))
