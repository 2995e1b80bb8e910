"""Synthetic chains and literal bsw_pair records for the device replay of mem_chain2aln's seed loop (bsw_chain2aln_replay_batch and
its ticket, tests/test_c2a_device_cpu.py and tests/test_gpu_c2a_device.py).  No DP runs: the replay only READS result records, so
the records are made up, and the oracle for everything is the host's bsw_chain2aln_replay on the same arrays.

The recipe: reads of 100 - 250 bases with 1 - 4 chains each; a chain takes its seed count from `sizes`; chain 0's diagonal d0 is
random and each later chain keeps the previous chain's with probability 1/2 (so that regions of earlier chains explain seeds);
a seed has len 12 - 40, qbeg uniform, rbeg = d0 + qbeg + off (off = 0 with probability 0.7, else -6 .. 6) and score = len with
probability 0.7, else uniform 0 .. len; its record grows it by gl in [0, qbeg] and gr in [0, l - qbeg - len] on the query, by that
-2 .. +2 on the reference (clamped to the seed), with w in {1, 5, 10, 50, 100, 200} and random score / truesc.
test_generator_is_non_vacuous (tests/test_c2a_device_cpu.py) keeps the recipe from being hollowed out."""
import numpy as np

SMALL = (1, 2, 3, 5, 8)
MIDDLE = (15, 16, 17, 31, 32, 33)
LARGE = (63, 64, 65, 127, 128, 129)
WS = (1, 5, 10, 50, 100, 200)


def make(host, n_reads, sizes, seed, d0_base=0, empty=(), chain_sizes=None):
    """-> dict(chains=CHAIN[], seeds=CSEED[], lens=int32[n_reads], pairs=PAIR[]).  empty: reads without any chain.  chain_sizes
    (optional): {read: [seed count per chain]} in place of the random draw for those reads."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(100, 251, size=n_reads).astype(np.int32)
    chains, seeds, pairs = [], [], []
    for r in range(n_reads):
        if r in empty:
            continue
        l = int(lens[r])
        fixed = (chain_sizes or {}).get(r)
        counts = list(fixed) if fixed is not None else [int(sizes[rs.randint(len(sizes))]) for _ in range(rs.randint(1, 5))]
        d0 = 0
        for k, n in enumerate(counts):
            if k == 0 or rs.rand() < 0.5:
                d0 = d0_base + int(rs.randint(1000, 1000000))
            chains.append((r, n, len(seeds), 0, 0, int(rs.randint(0, 25)), float(rs.randint(0, 100)) / 128.0))
            ln = rs.randint(12, 41, size=n)
            qb = (rs.rand(n) * (l - ln + 1)).astype(np.int64)
            off = np.where(rs.rand(n) < 0.7, 0, rs.randint(-6, 7, size=n))
            sc = np.where(rs.rand(n) < 0.7, ln, (rs.rand(n) * (ln + 1)).astype(np.int64))
            gl = (rs.rand(n) * (qb + 1)).astype(np.int64)
            gr = (rs.rand(n) * (l - qb - ln + 1)).astype(np.int64)
            dl, dr = rs.randint(-2, 3, size=n), rs.randint(-2, 3, size=n)
            w = np.array(WS)[rs.randint(len(WS), size=n)]
            psc, ptr = rs.randint(0, 300, size=n), rs.randint(0, 300, size=n)
            for i in range(n):
                seeds.append((d0 + int(qb[i]) + int(off[i]), int(qb[i]), int(ln[i]), int(sc[i]), 0))
                # the pair record: qb absolute, qe relative to the seed's query end, rb / re relative to the seed's reference begin / end
                pairs.append((len(pairs), int(qb[i] - gl[i]), int(gr[i]), -max(int(gl[i] + dl[i]), 0), max(int(gr[i] + dr[i]), 0), int(psc[i]), int(ptr[i]), int(w[i])))
    return dict(chains=np.array(chains, dtype=host.CHAIN).reshape(-1), seeds=np.array(seeds, dtype=host.CSEED).reshape(-1), lens=lens,
                pairs=np.array(pairs, dtype=host.PAIR).reshape(-1))


def params(host, a=1, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100):
    """scoring as the replay reads it: the match score, the gap penalties and the band of bsw_cal_max_gap"""
    p = host.default_params(o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, w=w)
    p["mat"][0] = host.bwa_matrix(a=a)
    return p


# the penalties (a, o, e, w) every parity test runs: bwa's, another symmetric set, an asymmetric one (o_del / o_ins, e_del / e_ins)
PENALTIES = (dict(), dict(a=2, o_del=5, e_del=3, o_ins=5, e_ins=3, w=7), dict(a=1, o_del=4, o_ins=2, e_del=9, e_ins=1, w=37))


def full_records(host, pairs, seed=1):
    """the same records as bsw_result[]: the pair record is the head, the tail is junk the replay must never read"""
    rs = np.random.RandomState(seed)
    raw = rs.randint(0, 256, size=(len(pairs), host.RESULT.itemsize)).astype(np.uint8)
    raw[:, :host.PAIR.itemsize] = pairs.view(np.uint8).reshape(len(pairs), host.PAIR.itemsize)
    return raw.reshape(-1).view(host.RESULT)


def host_replay(host, params, s, results=None, opt=None):
    """the oracle: bsw_chain2aln_replay on the host -> (regs, extended, reg_start)"""
    return host.chain2aln_replay(params, s["chains"], s["seeds"], s["lens"], s["pairs"] if results is None else results, opt=opt)


def same(got, want):
    """None, or what differs between two (regs, extended, reg_start) triples, compared byte for byte"""
    for name, a, b in zip(("regs", "extended", "reg_start"), got, want):
        if a is None:
            continue
        if len(a) != len(b):
            return "%s: %d entries, want %d" % (name, len(a), len(b))
        if a.tobytes() != b.tobytes():
            bad = [i for i in range(len(a)) if a[i:i + 1].tobytes() != b[i:i + 1].tobytes()]
            return "%s: %d entries differ, the first at %d: %s, want %s" % (name, len(bad), bad[0], a[bad[0]], b[bad[0]])
    return None


def dump(path, params, opt, s, results, stride):
    """the set as tests/c2a_core_model.cpp reads it: a header of int64, then the arrays as they lie in memory"""
    hdr = np.array([len(s["chains"]), len(s["seeds"]), len(s["lens"]), stride], dtype=np.int64)
    with open(path, "wb") as f:
        f.write(hdr.tobytes())
        f.write(params.tobytes())
        f.write(opt.tobytes())
        f.write(s["chains"].tobytes())
        f.write(s["seeds"].tobytes())
        f.write(s["lens"].tobytes())
        f.write(results.tobytes())
