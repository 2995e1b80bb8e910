"""bsw_cigar_md_kernel (NM and MD from the final CIGAR) at its step, lane, digit and buffer edges: the planted cases of
tests/_md_cases.py through all three entry forms, every field of every task against _gencigar_ref.reg2aln
(test_gpu_cigar_ref.check), the GPU's own CIGAR and MD against the definition of MD (_md_cases.rebuild), and slots of max_md
bytes / max_cigar words that fit exactly or miss by one.  test_cigar_md_edges_cpu.py shows on the reference's answers that
every case holds the feature it is there for.

Measured on an MI355X, the answers of the reference included: test_planted_edges 0.14 s and 0.11 s,
test_exact_fit_of_md_and_cigar 0.16 s (eight batches), the tickets and resident reads 0.14 s, the child process 2.4 s.
LIMIT and CHILD_LIMIT below bound them (about 25 times the slowest), and the module's context waits at most WAIT_MS for
the GPU."""
import os
import subprocess
import sys
import time
from contextlib import contextmanager

import numpy as np
import pytest

import _md_cases as mc
from test_gpu_cigar_ref import L_PAC, check, pen_of

pytestmark = pytest.mark.gpu

LIMIT = 5.0                            # seconds for one in-process test
WAIT_MS = 20000                        # the library's own limit for one wait on the GPU
CHILD_LIMIT = 60                       # seconds for the child process: interpreter, imports, context, the four batches


@contextmanager
def within(seconds):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print("%.2f s" % dt)
    assert dt < seconds, dt


@pytest.fixture(scope="module")
def bound(host):
    """a context of its own (a short wait limit) with the genome of _md_cases on it"""
    c = host.BswContext(device=0, timeout_ms=WAIT_MS)
    ref = c.ref_upload(mc.genome_pac(), L_PAC)
    yield c, (mc.genome_pac(), ref)
    c.ref_free(ref)
    c.close()


def params(host, ts=False):
    p = host.default_params()
    assert bytes(p["mat"][0]) == mc.MAT.tobytes() and pen_of(p) == mc.PEN      # what the shared answers were computed with
    return host.default_params(mat=mc.MAT_TS) if ts else p


def batch(oracle, strands, ts=False, only="abcdef", seed=77):
    """the planted cases of these strands whose names start with a letter of `only`, shuffled: (names, specs, answers)"""
    rows = []
    for strand in strands:
        for (name, s), w in zip(mc.cases(strand, ts), mc.answers(oracle, strand, ts)):
            if name[0] in only:
                rows.append(("%s/%d" % (name, strand), s, w))
    perm = np.random.default_rng(seed).permutation(len(rows))
    return [rows[i][0] for i in perm], [rows[i][1] for i in perm], [rows[i][2] for i in perm]


class Form:
    """cigar_ref_batch's face on one of the three entry forms, so that check() compares every field of every task on each of
    them; `raw` keeps the arrays of the last call.  A slot's NUL is looked at too (check() compares md_len bytes)."""
    def __init__(self, host, ctx, form, rd=None):
        self.host, self.ctx, self.form, self.rd, self.raw = host, ctx, form, rd, None

    def cigar_ref_batch(self, p, ref, ct, max_cigar=64, max_md=256):
        if self.form == "batch":
            return self.ctx.cigar_ref_batch(p, ref, ct, max_cigar=max_cigar, max_md=max_md)
        if self.form == "ticket":
            t, res, cig, md = self.ctx.submit_cigar_ref(p, ref, ct, max_cigar=max_cigar, max_md=max_md)
        else:                                                                  # read k of the block is task k's read
            rdt = np.zeros(len(ct), dtype=self.host.RD_CTASK)
            rdt["read"], rdt["qb"], rdt["qe"] = np.arange(len(ct)), 0, ct["l_query"]
            for f in ("w", "rb", "re", "w_cap", "min_score", "max_tries"):
                rdt[f] = ct[f]
            t, res, cig, md = self.ctx.submit_cigar_reads(p, ref, self.rd, rdt, max_cigar=max_cigar, max_md=max_md)
        self.ctx.wait_ticket(t)
        self.raw = res, cig, md
        ends = np.clip(res["md_len"], 0, max_md - 1)
        assert (md[np.arange(len(ct)), ends] == 0).all(), np.nonzero(md[np.arange(len(ct)), ends])[0]
        return res, cig, self.ctx.md_strings(res, md)


def own_cigars(res, cig):
    return [[(int(x) & 0xf, int(x) >> 4) for x in cig[i, :int(res["n_cigar"][i])]] for i in range(len(res))]


@pytest.mark.parametrize("strand", [0, 1])
def test_planted_edges(host, oracle, bound, strand):
    """every planted case of one strand in one shuffled batch, pointer form; then the GPU's CIGAR and MD must rebuild the target"""
    ctx, genome = bound
    with within(LIMIT):
        for ts in (False, True):
            names, specs, want = batch(oracle, [strand], ts)
            res, cig, md, _ = check(host, oracle, ctx, params(host, ts), genome, specs, max_cigar=64, max_md=20000, want=want)
            for i, c in enumerate(own_cigars(res, cig)):
                assert int(res["n_cigar"][i]) > 0 and int(res["md_len"][i]) > 0, names[i]
                mc.check_rebuild(specs[i], c, md[i], int(res["nm"][i]))


def test_exact_fit_of_md_and_cigar(host, oracle, bound):
    """a slot of max_md bytes that the MD of task k fills to the last byte, and one a byte short; max_cigar words that hold
    task k's ops exactly, and one word short.  Other tasks of the batch lie on both sides of each limit, and every slot is
    compared, so a store past a slot's end shows in the neighbour."""
    ctx, genome = bound
    names, specs, want = batch(oracle, [0, 1], only="def")
    k = names.index("d64/0")
    assert 0 < k < len(names) - 1                                              # a neighbour on either side
    lens, ops = [len(w["md"]) for w in want], [len(w["cigar"]) for w in want]
    assert min(lens) + 1 < lens[k] < max(lens) and min(ops) < ops[k] - 1 and ops[k] < max(ops)
    assert all(n > 0 for n in (sum(x + 1 <= lens[k] for x in lens), sum(x > lens[k] for x in lens),
                               sum(x <= ops[k] - 1 for x in ops), sum(x > ops[k] for x in ops)))
    p = params(host)
    with within(LIMIT):
        for form in ("batch", "ticket"):
            f = Form(host, ctx, form)
            res, _, md, _ = check(host, oracle, f, p, genome, specs, max_cigar=64, max_md=lens[k] + 1, want=want)
            assert (int(res["md_len"][k]), md[k]) == (lens[k], want[k]["md"])
            fit = int((res["md_len"] > 0).sum())
            res, _, md, _ = check(host, oracle, f, p, genome, specs, max_cigar=64, max_md=lens[k], want=want)
            assert (int(res["md_len"][k]), md[k]) == (-(lens[k] + 1), "")
            assert 0 < int((res["md_len"] > 0).sum()) < fit < len(specs)
            res, cig, _, _ = check(host, oracle, f, p, genome, specs, max_cigar=ops[k], max_md=20000, want=want)
            assert own_cigars(res, cig)[k] == want[k]["cigar"] and (res["n_cigar"] < 0).any()
            res, _, md, _ = check(host, oracle, f, p, genome, specs, max_cigar=ops[k] - 1, max_md=20000, want=want)
            assert (int(res["n_cigar"][k]), int(res["nm"][k]), md[k]) == (-ops[k], -1, "") and (res["n_cigar"] > 0).any()


def test_planted_edges_through_tickets_and_resident_reads(host, oracle, bound):
    """the planted batch of both strands through bsw_cigar_ref_submit_t and, by read index, bsw_cigar_reads_submit_t: each
    against the reference field by field, and equal to the batch call's records, CIGAR words and MD bytes"""
    ctx, genome = bound
    names, specs, want = batch(oracle, [0, 1])
    p = params(host)
    with within(LIMIT):
        res, cig, md, _ = check(host, oracle, ctx, p, genome, specs, max_cigar=64, max_md=20000, want=want)
        rd = ctx.reads_upload([s["read"] for s in specs])
        try:
            for f in (Form(host, ctx, "ticket"), Form(host, ctx, "reads", rd)):
                check(host, oracle, f, p, genome, specs, max_cigar=64, max_md=20000, want=want)
                res2, cig2, md2 = f.raw
                assert res2.tobytes() == res.tobytes(), f.form
                for i in range(len(specs)):
                    n, m = int(res["n_cigar"][i]), int(res["md_len"][i])
                    assert (cig2[i, :n] == cig[i, :n]).all() and bytes(md2[i, :m + 1]) == md[i].encode() + b"\0", (f.form, names[i])
        finally:
            ctx.reads_free(rd)


def test_planted_edges_on_the_ring_kernel():
    """BSW_GLOBAL_LONG=1 sends every try to the LDS ring kernel, whose CIGARs the NM / MD kernel then walks: the planted
    batches again, in a fresh process"""
    env = dict(os.environ, BSW_GLOBAL_LONG="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(here, "test_gpu_cigar_md_edges.py") + "::test_planted_edges"],
                       env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout
