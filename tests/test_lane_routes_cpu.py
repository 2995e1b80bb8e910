"""The routing half of tests/test_gpu_lane_routes.py on every CPU run: bsw_plan_batch (host only) under each route's switches, with
the same draws and seed generator (tests/_routes.py), shows the route — and the same draws without the route's switch show it is
not taken, so the GPU fuzz cannot pass by running the plain lane kernels if a threshold moves.  The switches are read once per
process: every case runs in a child of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import __graft_entry__ as g
host = g.load_package().host
import _routes as R
route, nsplit, taken = %(route)r, %(nsplit)d, %(taken)d
n16 = nq = 0
for over, mat, seeds, wide in R.draws(route, 16, %(n)d, %(seed)d):
    p = R.make_params(host, over, mat)
    tasks, arena = host.make_tasks(seeds)
    if taken:
        R.prove_route(host, p, tasks, seeds, route, nsplit)
    else:
        a, b = R.prove_not_taken(host, p, tasks, seeds, route)
        n16 += a; nq += b
assert taken or (n16 > 0 and nq > 0), (n16, nq)
print("ok")
"""

CASES = [(route, nsplit) for route in ("group", "group_fused", "lane_fused") for nsplit in (0, 1)]


def _run(route, env_route, nsplit, taken):
    from _routes import child_env
    seed = 31000 + 10 * CASES.index((route, nsplit))          # the draws of the GPU fuzz: its parameters, the first 400 seeds of each
    src = SNIPPET % dict(root=ROOT, route=route, nsplit=nsplit, taken=int(taken), n=400, seed=seed)
    out = subprocess.run([sys.executable, "-c", src], env=child_env(os.environ, env_route, nsplit), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("route,nsplit", CASES, ids=["%s-%s" % (r, "nsplit" if s else "inkernel") for r, s in CASES])
def test_route_is_taken(built, route, nsplit):
    _run(route, route, nsplit, True)


# each route's switches without the one that selects it: BSW_GROUP=1 for the group routes, BSW_LANE_FUSE=1 for the fused lane
# launch; BSW_NSPLIT is left off (its presence is what the nsplit cases above prove)
WITHOUT = {"group": dict(BSW_GROUP_FUSE="0"), "group_fused": dict(BSW_GROUP_FUSE="1"), "lane_fused": dict(BSW_GROUP="0")}


@pytest.mark.parametrize("route", sorted(WITHOUT))
def test_route_is_not_taken_without_its_switch(built, route):
    _run(route, WITHOUT[route], 0, False)
