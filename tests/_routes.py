"""The routes of a chunk that does not fill the machine, forced under BSW_KERNEL_LANE with the routing switches: the group kernel
(bsw_lane2g_kernel, a seed pair per group of eight lanes) per side and fused, and the lane kernel's fused launch
(bsw_lane2_kernel<17, 2, ., ., true>), each with and without the N list (BSW_NSPLIT=1).  The switches are read once per process,
so every route runs in a child process of its own: tests/test_gpu_lane_routes.py (kernels against the oracle) and
tests/test_lane_routes_cpu.py (the host plan alone).  Shared here: the draws, the seed generator and the route proof."""
import numpy as np

ROUTES = {
    "group": dict(BSW_GROUP="1", BSW_GROUP_FUSE="0"),         # lane2g NS=3 / NS=4, FUSED=false: a launch per side and class
    "group_fused": dict(BSW_GROUP="1", BSW_GROUP_FUSE="1"),   # lane2g NS=3 / NS=4, FUSED=true: one launch, left then right
    "lane_fused": dict(BSW_GROUP="0", BSW_LANE_FUSE="1"),     # lane2<17, 2, ., ., true> (sides <= 135)
}
ROUTE_ENVS = ("BSW_GROUP", "BSW_GROUP_FUSE", "BSW_LANE_FUSE", "BSW_NSPLIT", "BSW_NO_NARROW", "BSW_NARROW_SHARE", "BSW_NO_LANE2")
NONE = 0xffffffff
# the default lane class table (bsw_lane_kernel.hip): 72 / 136 / 232 columns at 8 bits, 136 at 16 bits
L8, L16 = (0, 1, 2), 3
COLS8, COLS16 = 232, 136
FIELDS = ("tag", "qb", "qe", "rb", "re", "score", "truesc", "w")


def child_env(environ, route, nsplit):
    """`environ` without any routing switch, then the switches of `route` (a name of ROUTES or a dict)"""
    env = {k: v for k, v in environ.items() if k not in ROUTE_ENVS}
    env.update(route if isinstance(route, dict) else ROUTES[route])
    if nsplit:
        env["BSW_NSPLIT"] = "1"
    return env


def _side(rng, ql, tfac, sub, indel, junk, perfect):
    """query of ql bases and its target"""
    if perfect:
        q = rng.integers(0, 4, ql).astype(np.uint8)
        return q, np.concatenate([q, rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8)])
    tl = int(rng.integers(0, int(ql * tfac) + 2))
    t = rng.integers(0, 4, tl).astype(np.uint8)
    if rng.random() < junk:
        return rng.integers(0, 4, ql).astype(np.uint8), t
    q = np.concatenate([t[:ql], rng.integers(0, 4, max(0, ql - tl)).astype(np.uint8)])
    q = np.where(rng.random(ql) < sub, (q + rng.integers(1, 4, ql)) & 3, q).astype(np.uint8)
    for _ in range(int(rng.poisson(indel * ql))):                   # short insertions and deletions, query length kept
        at, k = int(rng.integers(0, ql)), int(rng.integers(1, 8))
        if rng.random() < 0.5:
            q = np.concatenate([q[:at], rng.integers(0, 4, k).astype(np.uint8), q[at:]])[:ql]
        else:
            q = np.concatenate([q[:at], q[at + k:], rng.integers(0, 4, k).astype(np.uint8)])[:ql]
    return q, t


def route_seeds(rng, n, a, b, qcap, nrate, wide=False, tfac=1.6, sub=0.02, indel=0.01, junk=0.15):
    """Mostly two-sided seeds, some left-only and right-only.  70 % have h0 pushed to the 8-bit bound:
    h0 + (lqlen + rqlen) a + b in 252 .. 258; 15 % of those match perfectly to the end of both queries (the score is the
    bound itself).  2 % have h0 = 300 (16-bit).  `wide`: half the seeds get one side of 136 - 231 bases (the 232-column class);
    it needs a = 1 for such seeds to stay within 8 bits.  Ns in queries and targets at rate `nrate`."""
    tmax = max(1, (254 - b) // a)                     # the longest total that leaves h0 >= 1 at the bound
    seeds = []
    for k in range(n):
        r = rng.random()
        sides = "lr" if r < 0.75 else "l" if r < 0.87 else "r"
        bound, perfect = rng.random() < 0.7, rng.random() < 0.15
        lens = {sd: int(rng.integers(1, qcap + 1)) for sd in sides}
        if wide and rng.random() < 0.5:
            lens[sides[int(rng.integers(0, len(sides)))]] = int(rng.integers(136, 232))
        if bound:
            while sum(lens.values()) > tmax:             # shrink the shorter side first
                sd = min(lens, key=lens.get) if len(lens) == 2 and min(lens.values()) > 1 else max(lens, key=lens.get)
                lens[sd] = max(1, lens[sd] - max(1, (sum(lens.values()) - tmax)))
            h0 = max(1, 255 - b - sum(lens.values()) * a + int(rng.integers(-3, 4)))
        else:
            h0 = int(rng.integers(1, 61))
        if rng.random() < 0.02:
            h0 = 300
        s = {"h0": h0, "init_score": -1 if rng.random() < 0.8 else int(rng.integers(-1, 50)), "tag": int(rng.integers(0, 2 ** 32))}
        for sd in sides:
            q, t = _side(rng, lens[sd], tfac, sub, indel, junk, perfect and bound)
            if nrate > 0 and not (perfect and bound):
                q[rng.random(len(q)) < nrate] = 4
                t[rng.random(len(t)) < nrate] = 4
            s[sd + "q"], s[sd + "t"] = q, t
        seeds.append(s)
    return seeds


def draws(route, ndraws, n, seed):
    """(params overrides, matrix (a, b, n), seeds, wide) per draw: the parameter space of the two-seeds-per-lane fuzz, the
    four (variant, symmetric) kinds in turn; on the group routes the second half of the draws has sides in the 232-column
    class.  The parameters do not depend on n, and the seeds of a smaller n are the first n of a larger one.  Draw 1 has b = 0: its perfect matches at the bound score exactly 255 on the 8-bit path; draw 2 has w = 7 and three
    band tries: band retries of 8-bit seeds."""
    rng = np.random.default_rng(seed)
    for it in range(ndraws):
        kind = it % 4                                   # H/sym, M/sym, H/asym, M/asym
        wide = route != "lane_fused" and it >= ndraws // 2
        a = 1 if wide else int(rng.integers(1, 5))
        b = 0 if it == 1 else int(rng.integers(0, 9))
        nsc = -int(rng.integers(0, b + 1))
        o, e = int(rng.integers(0, 16)), int(rng.integers(1, 7))
        oi, ei = (o, e)
        if kind >= 2:
            oi, ei = int(rng.integers(0, 16)), int(rng.integers(1, 7))
            if (oi, ei) == (o, e):
                oi = (o + 1) % 16
        over = dict(o_del=o, e_del=e, o_ins=oi, e_ins=ei, w=int(rng.choice([1, 2, 7, 20, 100, 300])),
                    zdrop=int(rng.choice([0, 1, 10, 50, 100, 1000])), pen_clip5=int(rng.integers(0, 15)),
                    pen_clip3=int(rng.integers(0, 15)), max_band_try=int(rng.integers(1, 4)), variant=kind & 1)
        if it == 2:
            over.update(w=7, max_band_try=3)
        qcap = 231 if wide else (12, 60, 135)[it % 3]
        nrate = (0.0, 0.002, 0.04)[(it + 1) % 3]
        shape = dict(tfac=float(rng.choice([1.0, 1.6, 2.4])), sub=float(rng.choice([0.0, 0.02, 0.08])),
                     indel=float(rng.choice([0.0, 0.01, 0.05])))
        seeds = route_seeds(np.random.default_rng([seed, it]), n, a, b, qcap, nrate, wide=wide, **shape)
        yield over, (a, b, nsc), seeds, wide


def make_params(host, over, mat):
    p = host.default_params(**over)
    p["mat"][0] = host.bwa_matrix(a=mat[0], b=mat[1], n=mat[2])
    return p


def lane_bits(p, tasks):
    """bsw_seed_lane_bits per task: 8, 16, or 0 (a general kernel)"""
    a, b = int(p["mat"][0][0]), max(0, -int(p["mat"][0][1]))
    lq, rq = tasks["lqlen"].astype(np.int64), tasks["rqlen"].astype(np.int64)
    qm = np.maximum(lq, rq)
    top = tasks["h0"].astype(np.int64) + (lq + rq) * a
    return np.where(qm == 0, 0, np.where((top + b <= 255) & (qm + 1 <= COLS8), 8, np.where((top < 65000) & (qm + 1 <= COLS16), 16, 0)))


def query_n(seeds):
    return np.array([any(bool((np.asarray(s.get(k, ()), np.uint8) >= 4).any()) for k in ("lq", "rq")) for s in seeds])


def prove_route(host, p, tasks, seeds, route, nsplit):
    """The host plan under the child's switches shows `route`; returns what the launches must look like."""
    order, seg, _ = host.plan_batch(p, tasks, kernel=host.KERNEL_LANE)
    bits = lane_bits(p, tasks)
    lq, rq = tasks["lqlen"] > 0, tasks["rqlen"] > 0
    e8, e16 = bits == 8, bits == 16
    qn = query_n(seeds)
    moved = e8 & qn if nsplit else np.zeros(len(tasks), bool)        # to the general kernel's N list
    left = lambda c: order[seg[9 + c]:seg[10 + c]]
    right = lambda c: order[seg[17 + c]:seg[18 + c]]
    l8, r8 = np.concatenate([left(c) for c in L8]), np.concatenate([right(c) for c in L8])
    l16, r16 = left(L16), right(L16)
    wave = order[seg[0]:seg[8]]
    fused = route in ("group_fused", "lane_fused")
    group = route in ("group", "group_fused")
    assert seg[9] - seg[8] == e8.sum() + (0 if group else e16.sum())           # the lane seeds
    if fused:
        assert len(r8) == 0, "fused: no 8-bit right list"
        assert len(l8) == e8.sum(), "fused: every 8-bit seed on a left list"
        assert sorted(l8[l8 != NONE]) == list(np.nonzero(e8 & ~moved)[0])
    else:
        assert len(l8) == (e8 & lq).sum() and len(r8) == (e8 & rq).sum()
        assert sorted(l8[l8 != NONE]) == list(np.nonzero(e8 & lq & ~moved)[0])
        assert sorted(r8[r8 != NONE]) == list(np.nonzero(e8 & rq & ~moved)[0])
    nnone = int((l8 == NONE).sum() + (r8 == NONE).sum())
    assert (nnone > 0) == bool(moved.any()), (nnone, int(moved.sum()))
    h300 = np.nonzero(tasks["h0"] == 300)[0]
    if group:
        assert len(l16) == 0 and len(r16) == 0, "group: no 16-bit lane class"
        assert set(np.nonzero(e16)[0]) <= set(wave), "group: the 16-bit seeds run in the wave classes"
        assert set(h300) <= set(wave)
    else:
        assert sorted(l16) == list(np.nonzero(e16 & lq)[0]) and sorted(r16) == list(np.nonzero(e16 & rq)[0])
        assert set(h300[e16[h300]]) <= set(l16) | set(r16), "lane: the h0 = 300 seeds keep the 16-bit lane class"
    # launches of a resident batch (enqueue_batch): general classes, the N list, the fused launch, one per non-empty lane list,
    # then the redo list — and bsw_pair_finalize when the 16-bit class (the one-seed-per-lane kernel) runs
    nwave = sum(1 for c in range(8) if seg[c + 1] > seg[c])
    lists = sum(1 for c in range(4) for s0 in (9, 17) if seg[s0 + c + 1] > seg[s0 + c] and not (fused and c in L8))
    launches = nwave + (1 if nsplit and seg[9] > seg[8] else 0) + (1 if fused and len(l8) else 0) + lists + (1 if len(l16) + len(r16) == 0 else 2)
    side8 = np.concatenate([tasks["lqlen"][e8], tasks["rqlen"][e8]])
    if route == "group":
        ns3 = any(seg[s0 + c + 1] > seg[s0 + c] for c in (0, 1) for s0 in (9, 17))
        ns4 = any(seg[s0 + 3] > seg[s0 + 2] for s0 in (9, 17))
    elif route == "group_fused":
        ns4 = bool((side8 >= COLS16).any())
        ns3 = bool(e8.any()) and not ns4
    else:
        ns3 = ns4 = False
        assert not (side8 >= COLS16).any(), "lane fused: sides <= 135 only"
    return dict(launches=launches, e8=e8, ns3=ns3, ns4=ns4, moved=int(moved.sum()), n8=int(e8.sum()), nnone=nnone)


def prove_not_taken(host, p, tasks, seeds, route):
    """The same draw without the route's switch runs a list per side and keeps the 16-bit lane class."""
    order, seg, _ = host.plan_batch(p, tasks, kernel=host.KERNEL_LANE)
    bits = lane_bits(p, tasks)
    e8, e16 = bits == 8, bits == 16
    r8 = order[seg[17]:seg[20]]
    assert len(r8) == (e8 & (tasks["rqlen"] > 0)).sum() > 0, "a right list per 8-bit side"
    assert seg[13] - seg[12] == (e16 & (tasks["lqlen"] > 0)).sum() and seg[21] - seg[20] == (e16 & (tasks["rqlen"] > 0)).sum()
    lists = order[seg[9]:seg[21]]
    assert not (lists == NONE).any(), "no N list without BSW_NSPLIT"
    assert set(np.nonzero(e8)[0]) <= set(lists), "every 8-bit seed on a lane list, query Ns included"
    return int(e16.sum()), int((e8 & query_n(seeds)).sum())


class Tally:
    def __init__(self):
        self.kinds, self.ns3, self.ns4, self.retry, self.zstop, self.s255, self.nsplit = set(), 0, 0, 0, 0, 0, 0
        self.draws = self.seeds = self.seeds8 = 0

    def add(self, p, info, want, want_nozdrop):
        e8 = info["e8"]
        self.draws += 1
        self.seeds += len(want)
        self.seeds8 += int(e8.sum())
        if e8.any():
            sym = p["o_del"][0] == p["o_ins"][0] and p["e_del"][0] == p["e_ins"][0]
            self.kinds.add((int(p["variant"][0]), bool(sym)))
        self.ns3 += info["ns3"]
        self.ns4 += info["ns4"]
        w = int(p["w"][0])
        self.retry += int((e8 & ((want["left"]["aw"] > w) | (want["right"]["aw"] > w))).sum())
        if want_nozdrop is not None:
            self.zstop += int((e8 & ((want["left"]["cells"] != want_nozdrop["left"]["cells"]) |
                                     (want["right"]["cells"] != want_nozdrop["right"]["cells"]))).sum())
        self.s255 += int((e8 & (want["score"] == 255)).sum())
        self.nsplit += info["moved"]

    def check(self, route, nsplit):
        assert len(self.kinds) == 4, self.kinds
        if route != "lane_fused":
            assert self.ns3 and self.ns4, (self.ns3, self.ns4)
        assert self.retry and self.zstop and self.s255, (self.retry, self.zstop, self.s255)
        assert bool(self.nsplit) == bool(nsplit), self.nsplit

    def __str__(self):
        return "draws %d seeds %d (8-bit %d) kinds %d ns3 %d ns4 %d retries %d zdrop stops %d score255 %d nlist %d" % (
            self.draws, self.seeds, self.seeds8, len(self.kinds), self.ns3, self.ns4, self.retry, self.zstop, self.s255, self.nsplit)
