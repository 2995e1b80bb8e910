"""GPU parity of bsw_cigar_ref_batch (bwa_gen_cigar2 + mem_reg2aln's retries against the resident reference) with the CPU
restatement in tests/_gencigar_ref.py: score, every CIGAR op, NM, MD, w, tries and status, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _gen
import _gencigar_ref as gc

pytestmark = pytest.mark.gpu

L_PAC = 300_003                       # not a multiple of 4
INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def genome(ctx):
    rng = np.random.default_rng(2024)
    bases = rng.integers(0, 4, L_PAC).astype(np.uint8)
    pac = gc.pack_pac(bases)
    ref = ctx.ref_upload(pac, L_PAC)
    yield pac, ref
    ctx.ref_free(ref)


def pen_of(p):
    return int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0])


def spec(read, rb, re, w=100, w_cap=0, min_score=INT_MIN, max_tries=1):
    return dict(read=np.ascontiguousarray(read, dtype=np.uint8), rb=int(rb), re=int(re), w=w, w_cap=w_cap, min_score=min_score,
                max_tries=max_tries)


def read_of(rng, pac, rb, re, l_query, sub=0.03, indel=0.01, nrate=0.0):
    """a read of l_query bases derived from the bases of [rb, re) in bns_get_seq order (what the read aligns to)"""
    rseq = gc.bns_get_seq(pac, L_PAC, rb, re)
    q = _gen.mutate(rng, rseq, l_query, sub, indel)
    if nrate:
        q[rng.random(l_query) < nrate] = 4
    return q


def interval(rng, rlen, strand):
    lo = 0 if strand == 0 else L_PAC
    rb = lo + int(rng.integers(0, L_PAC - rlen + 1))
    return rb, rb + rlen


def make_ctasks(host, specs, arena=None):
    ct = np.zeros(len(specs), dtype=host.CTASK)
    keep = []
    off = 0
    for i, s in enumerate(specs):
        q = s["read"]
        if arena is not None and len(q):
            v = arena.u8[off:off + len(q)]
            v[:] = q
            ptr = arena.ptr + off
            off += len(q) + 1
        else:
            keep.append(q)
            ptr = q.ctypes.data if len(q) else 0
        ct[i]["query"], ct[i]["l_query"], ct[i]["w"] = ptr, len(q), s["w"]
        ct[i]["rb"], ct[i]["re"], ct[i]["w_cap"] = s["rb"], s["re"], s["w_cap"]
        ct[i]["min_score"], ct[i]["max_tries"] = s["min_score"], s["max_tries"]
    return ct, keep


def expected(oracle, p, pac, specs):
    mat, pen = p["mat"][0], pen_of(p)
    return [gc.reg2aln(oracle, mat, pen, L_PAC, pac, s["read"], s["rb"], s["re"], s["w"], s["w_cap"], s["min_score"],
                       s["max_tries"]) for s in specs]


def check(host, oracle, ctx, p, genome, specs, max_cigar=64, max_md=4096, arena=None, want=None):
    pac, ref = genome
    ct, keep = make_ctasks(host, specs, arena)
    res, cig, md = ctx.cigar_ref_batch(p, ref, ct, max_cigar=max_cigar, max_md=max_md)
    want = want or expected(oracle, p, pac, specs)
    for i, w in enumerate(want):
        r = res[i]
        ctxt = (i, len(specs[i]["read"]), specs[i]["rb"], specs[i]["re"], w.get("runs"), r)
        assert int(r["status"]) == w["status"], ctxt
        assert (int(r["tries"]), int(r["w"])) == (w["tries"], w["w"]), ctxt
        if w["status"]:
            assert (int(r["score"]), int(r["n_cigar"]), int(r["nm"]), int(r["md_len"]), md[i]) == (0, 0, -1, 0, ""), ctxt
            continue
        assert int(r["score"]) == w["score"], ctxt
        n = len(w["cigar"])
        if n > max_cigar:
            assert (int(r["n_cigar"]), int(r["nm"]), int(r["md_len"]), md[i]) == (-n, -1, 0, ""), ctxt
            continue
        assert int(r["n_cigar"]) == n, ctxt
        assert [(int(x) & 0xf, int(x) >> 4) for x in cig[i, :n]] == w["cigar"], ctxt
        assert int(r["nm"]) == w["nm"], ctxt
        if len(w["md"]) + 1 <= max_md:
            assert (int(r["md_len"]), md[i]) == (len(w["md"]), w["md"]), ctxt
        else:
            assert (int(r["md_len"]), md[i]) == (-(len(w["md"]) + 1), ""), ctxt
    return res, cig, md, want


def retry_read(rng, pac, rb, steps):
    """a 150-base read of [rb, rb + 150) whose path leaves the diagonal by the given insertions (+) / deletions (-) in turn"""
    rseq = gc.bns_get_seq(pac, L_PAC, rb, rb + 150)
    out, pos = [], 0
    cuts = [30 + 25 * k for k in range(len(steps))]
    for c, s in zip(cuts, steps):
        out.append(rseq[pos:c])
        if s > 0:
            out.append(rng.integers(0, 4, s).astype(np.uint8))
            pos = c
        else:
            pos = c - s
    out.append(rseq[pos:])
    return np.concatenate(out)


def build_mixed(pac, seed=5):
    rng = np.random.default_rng(seed)
    specs = []
    for lq in (1, 150, 250, 1023, 1024, 1025, 2048, 8191):
        for strand in (0, 1):
            for k in range(2):
                rlen = max(1, lq + int(rng.integers(-lq // 20 - 1, lq // 20 + 2)))
                rb, re = interval(rng, rlen, strand)
                q = read_of(rng, pac, rb, re, lq, 0.03, 0.01, 0.01 if k else 0.0)
                w = int(rng.choice([0, 5, 40, 100, 200]))
                specs.append(spec(q, rb, re, w=w))
    # the edges of both strands
    for rb, re in ((0, 180), (L_PAC - 170, L_PAC), (L_PAC, L_PAC + 160), (2 * L_PAC - 190, 2 * L_PAC)):
        specs.append(spec(read_of(rng, pac, rb, re, 175), rb, re, w=100))
    # no-gap shortcut (w_ = 0, equal lengths), alone and with a second try
    for strand in (0, 1):
        rb, re = interval(rng, 150, strand)
        specs.append(spec(read_of(rng, pac, rb, re, 150, 0.05, 0.0), rb, re, w=0))
        specs.append(spec(read_of(rng, pac, rb, re, 150, 0.05, 0.0), rb, re, w=0, w_cap=50, min_score=1000, max_tries=3))
    # retries: 3 tries (the score grows with every band), a stop on an equal score, a stop at w_cap, min_score reached
    for strand in (0, 1):
        rb, _ = interval(rng, 150, strand)
        specs.append(spec(retry_read(rng, pac, rb, [6, 6, -12]), rb, rb + 150, w=4, w_cap=64, min_score=1000, max_tries=3))
        specs.append(spec(retry_read(rng, pac, rb, [6, -6]), rb, rb + 150, w=4, w_cap=64, min_score=1000, max_tries=3))
        specs.append(spec(retry_read(rng, pac, rb, [6, 6, -12]), rb, rb + 150, w=4, w_cap=8, min_score=1000, max_tries=3))
        specs.append(spec(retry_read(rng, pac, rb, [6, -6]), rb, rb + 150, w=4, w_cap=64, min_score=-1000, max_tries=3))
        specs.append(spec(retry_read(rng, pac, rb, [6, -6]), rb, rb + 150, w=1, w_cap=0, min_score=1000, max_tries=2))
    # random retry parameters
    for _ in range(40):
        rb, re = interval(rng, int(rng.integers(140, 170)), int(rng.integers(0, 2)))
        q = read_of(rng, pac, rb, re, 150, 0.03, 0.02)
        specs.append(spec(q, rb, re, w=int(rng.integers(0, 30)), w_cap=int(rng.integers(0, 120)),
                          min_score=int(rng.integers(80, 170)), max_tries=int(rng.integers(0, 4))))
    # bwa's "no alignment" answers mixed in
    q = read_of(rng, pac, 1000, 1100, 100)
    for rb, re in ((5000, 5000), (5100, 5000), (L_PAC - 50, L_PAC + 50), (2 * L_PAC - 50, 2 * L_PAC + 50), (-20, 80)):
        specs.append(spec(q, rb, re))
    specs.append(spec(np.zeros(0, np.uint8), 100, 200))
    perm = rng.permutation(len(specs))
    return [specs[i] for i in perm]


@pytest.mark.parametrize("memory", ["staged", "registered"])
def test_mixed_batch(host, oracle, ctx, genome, memory):
    pac, _ = genome
    specs = build_mixed(pac)
    arena = host.HostArena(sum(len(s["read"]) + 1 for s in specs) + 64) if memory == "registered" else None
    try:
        _, _, _, want = check(host, oracle, ctx, host.default_params(), genome, specs, max_cigar=2048, max_md=20000, arena=arena)
    finally:
        if arena is not None:
            arena.free()
    stops = [w["stop"] for w in want]
    for what in ("status", "equal", "cap", "score", "tries"):
        assert what in stops, (what, stops)
    assert any(w["tries"] == 3 for w in want)
    assert any(w.get("band") is None and w["status"] == 0 for w in want)      # the no-gap shortcut ran
    assert any(w["status"] == 0 and w["md"].count("^") for w in want)         # interior deletions in MD


def test_other_penalties_and_longest_target(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(9)
    specs = []
    for strand in (0, 1):
        rb, re = interval(rng, 65535, strand)
        full = gc.bns_get_seq(pac, L_PAC, rb, re)
        specs.append(spec(_gen.mutate(rng, full[20000:], 8191, 0.02, 0.002), rb, re, w=100))
    for _ in range(20):
        rb, re = interval(rng, int(rng.integers(240, 270)), int(rng.integers(0, 2)))
        specs.append(spec(read_of(rng, pac, rb, re, 250, 0.04, 0.02), rb, re, w=int(rng.integers(1, 80)), w_cap=200,
                          min_score=240, max_tries=3))
    check(host, oracle, ctx, host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1), genome, specs, max_cigar=256, max_md=70000)


def general_specs(pac):
    """200 reads of 150 bases with substitutions, indels and N on both strands, bands of 5 to 60 with up to three tries"""
    rng = np.random.default_rng(11)
    mat = _gen.general_matrix(rng, off_hi=-1)
    specs = []
    for i in range(200):
        rb, re = interval(rng, int(rng.integers(140, 170)), i & 1)
        q = read_of(rng, pac, rb, re, 150, 0.04, 0.02, 0.01 if i % 3 == 0 else 0.0)
        specs.append(spec(q, rb, re, w=int(rng.integers(5, 60)), w_cap=120, min_score=int(rng.integers(100, 900)), max_tries=int(rng.integers(1, 4))))
    return mat, specs


def test_matrix_without_symmetry_on_both_strands(host, oracle, ctx, genome):
    """On the reverse strand the read and the reference are both reversed before the global alignment: which of them is the row
    and which the column of mat[target * 5 + query] is invisible under bwa's matrices.  Here the transposed matrix gives the CPU
    restatement itself another score on 196 of 200 reads (measured; half is asserted)."""
    pac, _ = genome
    mat, specs = general_specs(pac)
    p = host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1)
    p["mat"][0] = mat.reshape(25)
    _, _, _, want = check(host, oracle, ctx, p, genome, specs, max_cigar=128, max_md=2048)
    for strand in (0, 1):
        mine = [w for s, w in zip(specs, want) if (s["rb"] >= L_PAC) == strand]
        assert len(mine) == 100 and sum(1 for w in mine if not w["status"] and len(w["cigar"]) >= 3) >= 40, strand
    ops = {op for w in want if not w["status"] for op, _ in w["cigar"]}
    assert {0, 1, 2} <= ops                                       # M, I and D
    pt = host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1)
    pt["mat"][0] = mat.T.reshape(25)
    other = expected(oracle, pt, pac, specs)
    differ = sum(1 for a, b in zip(want, other) if a["score"] != b["score"])
    print("transposed matrix: %d of %d scores differ" % (differ, len(specs)))
    assert differ >= 0.49 * len(specs)


def test_cigar_and_md_overflow(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(13)
    specs = []
    for i in range(60):                          # many ops / a long MD / a short MD
        rb, re = interval(rng, 150 if i % 3 else int(rng.integers(150, 160)), int(rng.integers(0, 2)))
        specs.append(spec(read_of(rng, pac, rb, re, 150, (0.05, 0.05, 0.0)[i % 3], (0.03, 0.0, 0.0)[i % 3]), rb, re, w=100))
    res, _, _, want = check(host, oracle, ctx, host.default_params(), genome, specs, max_cigar=3, max_md=12)
    assert (res["n_cigar"] < 0).any() and (res["md_len"] < 0).any() and (res["md_len"] > 0).any()


def test_empty_batch(host, ctx, genome):
    _, ref = genome
    res, cig, md = ctx.cigar_ref_batch(host.default_params(), ref, np.zeros(0, dtype=host.CTASK))
    assert len(res) == 0 and cig.shape[0] == 0 and md == []


def test_fifty_thousand_150bp_reads(host, oracle, ctx, genome):
    pac, _ = genome
    rng = np.random.default_rng(21)
    specs = []
    for _ in range(50_000):
        rb, re = interval(rng, int(rng.integers(148, 156)), int(rng.integers(0, 2)))
        specs.append(spec(read_of(rng, pac, rb, re, 150, 0.02, 0.005, 0.002), rb, re, w=100))
    check(host, oracle, ctx, host.default_params(), genome, specs, max_cigar=32, max_md=512)


def test_matches_global_batch_on_host_fetched_targets(host, ctx, genome):
    pac, ref = genome
    p = host.default_params()
    mat, pen = p["mat"][0], pen_of(p)
    rng = np.random.default_rng(31)
    specs = []
    for lq in (150, 250, 1500):
        for _ in range(30):
            rb, re = interval(rng, lq + int(rng.integers(-5, 6)), int(rng.integers(0, 2)))
            specs.append(spec(read_of(rng, pac, rb, re, lq, 0.03, 0.01), rb, re, w=int(rng.integers(1, 120))))
    ct, keep = make_ctasks(host, specs)
    res, cig, _ = ctx.cigar_ref_batch(p, ref, ct, max_cigar=128, want_md=False)
    gt = np.zeros(len(specs), dtype=host.GTASK)
    for i, s in enumerate(specs):                # the host recipe: bns_get_seq, reverse both on the reverse strand, bwa's band
        rseq = gc.bns_get_seq(pac, L_PAC, s["rb"], s["re"])
        q = s["read"]
        if s["rb"] >= L_PAC:
            q, rseq = q[::-1].copy(), rseq[::-1].copy()
        keep += [q, rseq]
        gt[i]["query"], gt[i]["target"], gt[i]["qlen"], gt[i]["tlen"] = q.ctypes.data, rseq.ctypes.data, len(q), len(rseq)
        gt[i]["w"] = gc.band(mat, *pen, len(q), len(rseq), s["w"])
    gres, gcig = ctx.global_batch(p, gt, max_cigar=128)
    assert (res["score"] == gres["score"]).all()
    assert (res["n_cigar"] == gres["n_cigar"]).all()
    for i in range(len(specs)):
        n = int(res["n_cigar"][i])
        assert (cig[i, :n] == gcig[i, :n]).all(), i


def test_errors(host, ctx, genome):
    _, ref = genome
    p = host.default_params()
    q = np.zeros(8192, dtype=np.uint8)

    def rc_of(ref_, **f):
        ct = np.zeros(2, dtype=host.CTASK)
        for t in ct:
            t["query"], t["l_query"], t["w"], t["rb"], t["re"], t["max_tries"] = q.ctypes.data, 100, 10, 0, 100, 1
        for k, v in f.items():
            ct[1][k] = v
        try:
            ctx.cigar_ref_batch(p, ref_, ct)
            return 0
        except host.BswError as e:
            return e.code

    assert rc_of(ref) == 0
    assert rc_of(ref, l_query=8192) == -3
    assert rc_of(ref, re=65536) == -3
    assert rc_of(ref, rb=1000, re=1000 + 65536) == -3
    assert rc_of(ref, w_cap=70000) == -3
    assert rc_of(ref, max_tries=4) == -2
    assert rc_of(ref, l_query=-1) == -2
    assert rc_of(ref, w=-1) == -2
    assert rc_of(ref, query=0) == -2
    assert rc_of(None) == -2


def test_long_kernel_route_in_a_child_process():
    """BSW_GLOBAL_LONG=1 sends every try to the LDS ring kernel: the mixed batch again, bit-exact, in a fresh process"""
    env = dict(os.environ, BSW_GLOBAL_LONG="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(here, "test_gpu_cigar_ref.py") + "::test_mixed_batch"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout
