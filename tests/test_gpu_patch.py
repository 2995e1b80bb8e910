"""GPU parity of bsw_patch_ref_batch and its two ticket forms (mem_patch_reg against the resident reference) with the CPU
restatement in tests/_patch_ref.py: every field of bsw_presult, on both strands, at the kernel class edges of the joined query,
through bwa's no-gap shortcut, across chunk cuts, beside other tickets, and what comes back over PCIe."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _gen
import _gencigar_ref as gc
import _patch_ref as P

pytestmark = pytest.mark.gpu

L_PAC = 200_003                       # not a multiple of 4
INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def pac():
    rng = np.random.default_rng(31337)
    return gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))


@pytest.fixture(scope="module")
def both(pac):
    g = gc.unpack_pac(pac, L_PAC)
    return np.concatenate([g, 3 - g[::-1]]).astype(np.uint8)


@pytest.fixture(scope="module")
def ref(ctx, pac):
    r = ctx.ref_upload(pac, L_PAC)
    yield r
    ctx.ref_free(r)


def pen_of(p):
    return int(p["o_del"][0]), int(p["e_del"][0]), int(p["o_ins"][0]), int(p["e_ins"][0])


INDELS = [0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 8, 10, 12]


def split_read(rng, both, L, strand, kind, x=None, d=None):
    """a read of L bases off strand `strand` in two regions a, b: the read follows the reference up to a cut, then an insertion or a
    deletion of 0 - 12 bases, then the reference again; a ends and b starts within 10 bases of the cut (overlapping or apart).
    kind: what is done to the pair afterwards.  -> dict(read, a, b, kind)"""
    if x is None:
        x = int(rng.integers(500, L_PAC - 1500)) + strand * L_PAC
    cut = int(rng.integers(45, L - 45))
    if d is None:
        d = INDELS[int(rng.integers(0, len(INDELS)))] if kind != "shortcut" else 0
    ins = d if rng.random() < 0.5 else 0
    dele = d - ins
    tail = L - cut - ins
    read = np.concatenate([both[x:x + cut], rng.integers(0, 4, ins).astype(np.uint8), both[x + cut + dele:x + cut + dele + tail]]).astype(np.uint8)
    sub = np.nonzero(rng.random(L) < 0.005)[0]
    read[sub] = (read[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
    aqb = int(rng.integers(0, 6))
    aqe = cut + int(rng.integers(-10, 11))
    bqb = cut + ins + int(rng.integers(-10, 11))
    bqe = L - int(rng.integers(0, 6))
    if kind == "shortcut":
        bqb = aqe + int(rng.integers(-5, 6))
    a = P.reg(x + aqb, x + aqe, aqb, aqe, aqe - aqb - int(rng.integers(0, 8)), int(rng.integers(0, 25)))
    brb = x + cut + dele + (bqb - cut - ins)
    b = P.reg(brb, brb + (bqe - bqb), bqb, bqe, bqe - bqb - int(rng.integers(0, 8)), int(rng.integers(0, 25)))
    if kind == "shortcut":
        a["w"] = b["w"] = 0
    elif kind == "strand":               # (a forward a only: a.rb <= b.rb must hold)
        b["rb"] += L_PAC
        b["re"] += L_PAC
    elif kind == "colinear":
        if rng.random() < 0.5:
            b["qb"], b["qe"] = a["qb"], a["qb"] + (bqe - bqb)
        else:
            b["qe"] = a["qe"]
            b["qb"] = min(b["qb"], a["qe"] - 20)
    elif kind == "far":                  # too far apart on the reference for the band (and for the ratio)
        sh = int(rng.integers(250, 700))
        b["rb"] += sh
        b["re"] += sh
    elif kind == "skew":                 # within the band, beyond the ratio
        sh = int(rng.integers(40, 90))
        b["rb"] += sh
        b["re"] += sh
    elif kind == "skew_ovl":             # overlapping on both, by too different amounts
        sh = int(0.12 * L) + int(rng.integers(0, 8))
        b["qb"] = a["qe"] - 5
        b["rb"] = max(a["re"] - 5 - sh, a["rb"])
        b["re"] = b["rb"] + (b["qe"] - b["qb"])
    elif kind == "junk":                 # the regions claim what the read does not hold: the alignment runs, the ratio fails
        lo = min(a["qe"], b["qb"])
        read[lo:] = rng.integers(0, 4, L - lo).astype(np.uint8)
    elif kind == "n":
        read[rng.random(L) < 0.03] = 4
        read[a["qb"]] = 4
        read[b["qe"] - 1] = 4
    return dict(read=read, a=a, b=b, kind=kind)


def status_workload(both):
    rng = np.random.default_rng(77)
    kinds = ["plain"] * 8 + ["shortcut"] * 2 + ["n"] * 2 + ["junk"] * 2 + ["strand", "colinear", "far", "skew", "skew_ovl"]
    specs = []
    for i in range(1980):
        kind = kinds[i % len(kinds)]
        strand = 0 if kind == "strand" else (i // len(kinds)) % 2
        specs.append(split_read(rng, both, 250 if i % 3 else 150, strand, kind))
    # bwa_gen_cigar2 without an alignment: the joined interval bridges l_pac, or leaves [0, 2 l_pac) at either end
    for x in (L_PAC - 130, L_PAC - 135, L_PAC - 140):
        specs.append(split_read(rng, both, 150, 0, "plain", x=x, d=1))
    s = split_read(rng, both, 150, 1, "plain", x=2 * L_PAC - 400, d=1)
    for g in (s["a"], s["b"]):
        g["rb"] += 300
        g["re"] += 300
    specs.append(s)
    s = split_read(rng, both, 150, 0, "plain", x=500, d=0)
    for g in (s["a"], s["b"]):
        g["rb"] -= 520
        g["re"] -= 520
    specs.append(s)
    return specs


def make_ptasks(host, specs):
    pt = np.zeros(len(specs), dtype=host.PTASK)
    for i, s in enumerate(specs):
        pt[i]["query"], pt[i]["l_query"] = s["read"].ctypes.data, len(s["read"])
        for nm in ("a", "b"):
            for k, v in s[nm].items():
                pt[i][nm][k] = v
    return pt


def make_rd_ptasks(host, specs):
    pt = np.zeros(len(specs), dtype=host.RD_PTASK)
    for i, s in enumerate(specs):
        pt[i]["read"] = i
        for nm in ("a", "b"):
            for k, v in s[nm].items():
                pt[i][nm][k] = v
    return pt


def expected(oracle, p, pac, specs):
    mat, pen, opt_w = p["mat"][0], pen_of(p), int(p["w"][0])
    return [P.patch_reg(oracle, mat, pen, opt_w, L_PAC, pac, s["read"], s["a"], s["b"]) for s in specs]


def same(res, want, specs=None):
    for i, w in enumerate(want):
        got = tuple(int(res[i][k]) for k in ("score", "w", "gscore", "status"))
        assert got == (w["score"], w["w"], w["gscore"], w["status"]), (i, got, w, specs[i]["a"] if specs else None, specs[i]["b"] if specs else None)


@pytest.fixture(scope="module")
def statuses(host, oracle, pac, both):
    """the ~2 000 pairs and their expected records, computed once and left unchanged"""
    specs = status_workload(both)
    p = host.default_params()
    return specs, p, expected(oracle, p, pac, specs)


def test_statuses_and_strands(host, ctx, ref, statuses):
    specs, p, want = statuses
    res = ctx.patch_ref_batch(p, ref, make_ptasks(host, specs))
    same(res, want, specs)
    count = lambda f: sum(1 for w in want if f(w))              # noqa: E731
    for why in (P.STRAND, P.COLINEAR, P.GAP_W, P.GAP_R, P.OVL_R, "noaln"):
        assert count(lambda w: w["why"] == why) >= (5 if why == "noaln" else 20), why
    for st in (0, 1, 2):
        for rev in (False, True):
            assert count(lambda w: w["status"] == st and w["rev"] == rev) >= 50, (st, rev)
    assert count(lambda w: w["shortcut"] and not w["rev"]) >= 50 and count(lambda w: w["shortcut"] and w["rev"]) >= 50
    assert count(lambda w: w["status"] == 0 and not w["shortcut"]) >= 500
    ns = [w for s, w in zip(specs, want) if s["kind"] == "n"]
    assert sum(1 for w in ns if w["status"] != 1) >= 100


def joined(rng, both, lq, strand, aw, bw, indel=3, lead=5):
    """a read whose regions a, b join into a query of exactly lq bases starting at base `lead` of the read"""
    x = int(rng.integers(500, L_PAC - 9000)) + strand * L_PAC
    L = lq + lead + 4
    cut = lead + lq // 2
    read = np.concatenate([both[x:x + cut], both[x + cut + indel:x + indel + L]]).astype(np.uint8)
    sub = np.nonzero(rng.random(L) < 0.01)[0]
    read[sub] = (read[sub] + 1 + rng.integers(0, 3, len(sub))) % 4
    a = P.reg(x + lead, x + cut, lead, cut, cut - lead - 3, aw)
    b = P.reg(x + cut + indel, x + indel + lead + lq, cut, lead + lq, lead + lq - cut - 3, bw)
    return dict(read=read, a=a, b=b, kind="edge")


def test_kernel_class_edges(host, oracle, ctx, ref, pac, both):
    """the joined query at the register classes' bounds (qlen + 1 = 64 / 256 / 1 024), at the hand-over to the LDS ring with a
    narrow and a wide band, at 8 191 bases, and a band capped by opt->w << 2"""
    rng = np.random.default_rng(5)
    p = host.default_params()
    assert int(p["w"][0]) == 100
    specs, bands = [], []
    for lq in (63, 64, 65, 255, 256):
        for strand in (0, 1):
            specs.append(joined(rng, both, lq, strand, 4, 3))
            bands.append(10)
    for lq in (1022, 1023, 1024):
        for strand in (0, 1):
            specs.append(joined(rng, both, lq, strand, 4, 3))          # w = 3 (the deletion) + 7
            bands.append(10)
            specs.append(joined(rng, both, lq, strand, 200, 197))      # 3 + 397 = 400, the cap itself
            bands.append(400)
    specs.append(joined(rng, both, 8191, 1, 300, 97))
    bands.append(400)
    specs.append(joined(rng, both, 300, 0, 900, 900))                  # 1 803 capped by opt->w << 2
    bands.append(400)
    want = expected(oracle, p, pac, specs)
    assert [w["w"] for w in want] == bands
    assert all(w["status"] != 1 for w in want) and sum(1 for w in want if w["status"] == 0) >= len(want) // 2
    assert [s["b"]["qe"] - s["a"]["qb"] for s in specs[-2:]] == [8191, 300]
    same(ctx.patch_ref_batch(p, ref, make_ptasks(host, specs)), want, specs)


def test_no_gap_shortcut_beside_its_neighbour_under_a_general_matrix(host, oracle, ctx, ref, pac, both):
    """a.w = b.w = 0 and equal spans: w_ = 0, the score is the sum of matrix entries, no DP; with b.w = 1 the same pair goes through
    the band formula.  An asymmetric 5x5 matrix and four distinct gap penalties tell the two sequences and the two gaps apart."""
    rng = np.random.default_rng(6)
    p = host.default_params(o_del=5, e_del=2, o_ins=7, e_ins=1)
    p["mat"][0] = _gen.general_matrix(rng, off_hi=-1).reshape(25)
    specs = []
    for i in range(60):
        s = split_read(rng, both, 150 if i % 2 else 250, (i // 2) % 2, "shortcut")
        if i % 5 == 0:
            s["read"][rng.random(len(s["read"])) < 0.02] = 4
        t = dict(read=s["read"], a=dict(s["a"]), b=dict(s["b"], w=1), kind="neighbour")
        specs += [s, t]
    want = expected(oracle, p, pac, specs)
    assert all(w["shortcut"] and w["w"] == 0 for w in want[0::2]) and all(not w["shortcut"] and w["w"] == 1 for w in want[1::2])
    assert all(w["status"] != 1 for w in want)
    same(ctx.patch_ref_batch(p, ref, make_ptasks(host, specs)), want, specs)


def test_three_forms_agree(host, ctx, ref, statuses):
    """batch call, pointer ticket, reads ticket on a block of bsw_reads_upload, and on one of bsw_reads_upload_start with the
    ticket submitted before bsw_reads_wait: the same bytes"""
    specs, p, want = statuses
    specs, want = specs[:600], want[:600]
    pt, rpt = make_ptasks(host, specs), make_rd_ptasks(host, specs)
    base = ctx.patch_ref_batch(p, ref, pt)
    same(base, want, specs)
    t, r1 = ctx.submit_patch_ref(p, ref, pt)
    ctx.wait_ticket(t)
    assert r1.tobytes() == base.tobytes()
    reads = [s["read"] for s in specs]
    rd = ctx.reads_upload(reads)
    try:
        t, r2 = ctx.submit_patch_reads(p, ref, rd, rpt)
        with pytest.raises(host.BswError) as e:
            ctx.reads_free(rd)                                          # held by the ticket
        assert e.value.code == -6
        ctx.wait_ticket(t)
        assert r2.tobytes() == base.tobytes()
    finally:
        ctx.reads_free(rd)
    rd = ctx.reads_upload_start(reads)
    try:
        t, r3 = ctx.submit_patch_reads(p, ref, rd, rpt)
        ctx.reads_wait(rd)
        ctx.wait_ticket(t)
        assert r3.tobytes() == base.tobytes()
    finally:
        ctx.reads_free(rd)


def cigar_tasks_of(host, specs, want):
    """bwa_gen_cigar2 on the intervals the pairs that run are joined over: one try with the band mem_patch_reg hands over"""
    run = [k for k, w in enumerate(want) if w["status"] != 1]
    ct = np.zeros(len(run), dtype=host.CTASK)
    for j, k in enumerate(run):
        s, a, b = specs[k], specs[k]["a"], specs[k]["b"]
        ct[j]["query"], ct[j]["l_query"], ct[j]["w"] = s["read"].ctypes.data + a["qb"], b["qe"] - a["qb"], want[k]["w"]
        ct[j]["rb"], ct[j]["re"], ct[j]["min_score"], ct[j]["max_tries"] = a["rb"], b["re"], INT_MIN, 1
    return run, ct


def test_patch_ticket_beside_extension_and_cigar_tickets(host, oracle):
    """a patch ticket is accepted with an extension and a CIGAR ticket in flight and completes with the serial results; the fifth
    submit answers BSW_E_BUSY and changes nothing"""
    p = host.default_params()
    n, L = 4000, 150
    arena = host.HostArena(n * L + 64)
    try:
        pac, rt, _ = host.synth_ref_tasks(n, L_PAC, p, arena=arena.u8, seed=12, read_len=L, seed_len_min=19, seed_len_max=60,
                                          seed_at_start=0, sub_rate=0.02, indel_rate=0.004, n_rate=0.002, junk_frac=0.05)
        g = gc.unpack_pac(pac, L_PAC)
        specs = status_workload(np.concatenate([g, 3 - g[::-1]]).astype(np.uint8))[:400]
        want = expected(oracle, p, pac, specs)
        run, ct = cigar_tasks_of(host, specs, want)
        pt = make_ptasks(host, specs)
        with host.BswContext(device=0, chunk_tasks=1024) as c:
            ref = c.ref_upload(pac, L_PAC)
            try:
                want_e = c.submit_ref(p, ref, rt)
                c.wait()
                want_e = want_e.copy()
                t, wc, _, _ = c.submit_cigar_ref(p, ref, ct)
                c.wait_ticket(t)
                # bwa_gen_cigar2's score is the score, with or without its CIGAR
                assert [int(x) for x in wc["score"]] == [want[k]["gscore"] for k in run]
                e1 = c.submit_ref(p, ref, rt); t_e1 = c.last_ticket                 # noqa: E702
                t_c, rc, _, _ = c.submit_cigar_ref(p, ref, ct)
                t_p, rp = c.submit_patch_ref(p, ref, pt)
                t_p2, rp2 = c.submit_patch_ref(p, ref, pt[:50])
                assert len({t_e1, t_c, t_p, t_p2}) == 4 and c.inflight() == 4
                with pytest.raises(host.BswError) as ei:
                    c.submit_patch_ref(p, ref, pt)
                assert ei.value.code == -6 and c.inflight() == 4
                with pytest.raises(host.BswError) as ei:
                    c.patch_ref_batch(p, ref, pt)                                   # the synchronous call, too
                assert ei.value.code == -6 and c.inflight() == 4
                for t in (t_p, t_c, t_e1, t_p2):
                    c.wait_ticket(t)
                assert c.inflight() == 0
                same(rp, want, specs)
                same(rp2, want[:50], specs)
                assert e1.tobytes() == want_e.tobytes() and rc.tobytes() == wc.tobytes()
                same(c.patch_ref_batch(p, ref, pt), want, specs)                    # and the call works again
            finally:
                c.ref_free(ref)
    finally:
        arena.free()


def test_only_scores_come_back(host, ctx, ref, statuses):
    """D2H: 8 bytes per task of a chunk (bsw_gresult) and 32 per task of the no-gap shortcut (its bsw_cresult), nothing else; the
    CIGAR ticket on the same intervals brings back more"""
    specs, p, want = statuses
    run, ct = cigar_tasks_of(host, specs, want)
    pt = make_ptasks(host, specs)
    d0 = ctx.host_stats()["d2h_bytes"]
    t, rp = ctx.submit_patch_ref(p, ref, pt)
    ctx.wait_ticket(t)
    d1 = ctx.host_stats()["d2h_bytes"]
    t, rc, _, _ = ctx.submit_cigar_ref(p, ref, ct)
    ctx.wait_ticket(t)
    d2 = ctx.host_stats()["d2h_bytes"]
    same(rp, want, specs)
    short = sum(1 for w in want if w["shortcut"])
    print("D2H: patch %d bytes for %d tasks (%d run, %d by the shortcut), CIGAR %d bytes for %d" % (d1 - d0, len(specs), len(run), short, d2 - d1, len(run)))
    assert 0 < d1 - d0 <= 8 * len(specs) + 32 * short
    assert d1 - d0 < d2 - d1


def spans_of(cells, work):
    """cut_spans with work alone: a span is closed once it holds `work` cells"""
    n = acc = 0
    for i, c in enumerate(cells):
        if acc >= work:
            n, acc = n + 1, 0
        acc += c
    return n + (1 if len(cells) else 0)


def cuts_body(host, oracle):
    """run by the child process of the test below, under BSW_F4_PATCH_WORK"""
    work = int(float(os.environ["BSW_F4_PATCH_WORK"]))
    rng = np.random.default_rng(31337)
    pac = gc.pack_pac(rng.integers(0, 4, L_PAC).astype(np.uint8))
    g = gc.unpack_pac(pac, L_PAC)
    specs = status_workload(np.concatenate([g, 3 - g[::-1]]).astype(np.uint8))[:900]
    p = host.default_params()
    want = expected(oracle, p, pac, specs)
    mat, pen = p["mat"][0], pen_of(p)
    cells = []
    for s, w in zip(specs, want):
        if w["status"] == 1:
            cells.append(0)
            continue
        lq, rlen = s["b"]["qe"] - s["a"]["qb"], s["b"]["re"] - s["a"]["rb"]
        cells.append(min(lq, 2 * gc.band(mat, *pen, lq, rlen, w["w"]) + 1) * rlen)
    streams = 2
    with host.BswContext(devices=[0, 0], streams=streams) as c:
        ref = c.ref_upload(pac, L_PAC)
        try:
            pt = make_ptasks(host, specs)
            res = c.patch_ref_batch(p, ref, pt)                         # sub-batches of `work` cells on the context's lane
            same(res, want, specs)
            base = c.host_stats()["chunks"]
            t, r1 = c.submit_patch_ref(p, ref, pt)
            c.wait_ticket(t)
            grew = int(c.host_stats()["chunks"] - base)
            assert r1.tobytes() == res.tobytes()
            total, lanes = sum(cells), 2 * streams
            # the work of a chunk: the target, less when the lanes would otherwise go without, never below an eighth of it
            spans = spans_of(cells, min(work, max(work // 8, (total + lanes - 1) // lanes)))
            print("patch cuts: %d cells, work %d, %d chunks, %d spans" % (total, work, grew, spans))
            assert grew >= 5 and grew == spans, (grew, spans)
        finally:
            c.ref_free(ref)
    print("cuts ok")


def test_cuts_and_devices_in_a_child_process():
    """BSW_F4_PATCH_WORK is read once per process: a ticket of 900 pairs cut into >= 5 chunks over devices = [0, 0], the batch call
    into as many sub-batches; the results are those of the restatement, and bsw_host_stats counts one chunk per span"""
    env = dict(os.environ, BSW_F4_PATCH_WORK="1000000")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "cuts ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft
    cuts_body(graft.load_package().host, graft.load_oracle())
