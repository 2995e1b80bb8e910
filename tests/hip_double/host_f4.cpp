/* host_f4.cpp — the hosts of bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch and bsw_matesw_ref_batch (bsw_f4.hip,
 * bsw_cigar.hip, bsw_matesw.hip) and the scalar queue's ksw_align2 / ksw_global2 groups on the host-memory HIP stand-in, under
 * ASan / UBSan or TSan (TEST INFRASTRUCTURE; tests/test_host_double_cpu.py).
 *
 *   host_f4 f4 FILE              the four batch calls over n x memory kind on a workload that reaches every class and branch
 *   host_f4 f4split WHICH FILE   WHICH = count | z | b: batches that cross one bound of the hosts' sub-batch loops
 *   host_f4 f4scalar             ksw_global2 / ksw_global / ksw_align2 / ksw_align / ksw_extend2 from 12 threads and an offender
 *   host_f4 faults CALL          CALL = global | align | cigar | matesw: every single HIP failure inside that batch call
 *   host_f4 cuts                 cut_spans (csrc/bsw_f4_host.h), the hosts' sub-batch cutter, with small caps on made-up costs
 *   host_f4 rejects              the 8-bit-mode tasks the align hosts refuse (matrix minimum above 0, gap open + extend above 255)
 *
 * Expected values do not travel the path under test.  The stand-ins compute from the words the host staged; for the global and
 * the local alignment this program calls the oracle on the caller's byte-per-base sequences.  For CIGAR / NM / MD / retries and
 * for mate rescue it writes inputs and results to FILE and the Python test compares them with tests/_gencigar_ref.reg2aln and
 * tests/_matesw_ref.matesw.
 */
#include "host_f4_work.h"

/* ---- f4: parity over n x memory kind ---- */
static const size_t F4_NS[] = {0, 1, 63, 64, 65, 2600};

static int f4_mode(const char *path)
{
    FILE *f = fopen(path, "w");
    CHECK(f, "cannot write %s", path);
    const bsw_params p = default_params();
    genome1_t g;
    g.make(150001, 77);
    write_genome(f, g, p);
    size_t cases = 0;
    for (int reg = 0; reg < 2; ++reg)
        for (size_t n : F4_NS) {
            char what[96];
            snprintf(what, sizeof(what), "%s_n%zu", reg ? "registered" : "pageable", n);
            fresh(1);
            {
                rng_t r(1000 + n + (uint64_t)reg);
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
                bsw_ref *ref = nullptr;
                CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
                {
                    arena_t ar(n * 700 + 8192, reg != 0);
                    gwork w;
                    make_global(w, ar, g, r, n);
                    check_global(ctx, p, w, 48, true, what);
                    if (n == 65 || n == 2600) { check_global(ctx, p, w, 2, true, what); check_global(ctx, p, w, 48, false, what); }
                }
                {
                    arena_t ar(n * 900 + 8192, reg != 0);
                    awork w;
                    make_align(w, ar, g, r, n);
                    check_align(ctx, p, w, what);
                }
                {
                    arena_t ar(n * 300 + 8192, reg != 0);
                    cwork w;
                    make_cigar(w, ar, g, r, n);
                    run_cigar(ctx, p, ref, w, 64, 512, true, true, f, what);
                    if (n == 65) {
                        run_cigar(ctx, p, ref, w, 3, 512, true, true, f, what);       /* CIGAR overflow */
                        run_cigar(ctx, p, ref, w, 64, 6, true, true, f, what);        /* MD overflow */
                        run_cigar(ctx, p, ref, w, 64, 512, false, true, f, what);     /* cigars == NULL */
                        run_cigar(ctx, p, ref, w, 64, 512, true, false, f, what);     /* md == NULL */
                    }
                }
                {
                    arena_t ar(n * 400 + 8192, reg != 0);
                    mwork w;
                    make_matesw(w, ar, g, r, n);
                    run_matesw(ctx, p, ref, w, f, what);
                }
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
            }
            CHECK(hipdbl::live_objects() == 0, "%s: %zu HIP objects left alive after bsw_destroy", what, hipdbl::live_objects());
            ++cases;
        }
    fclose(f);
    printf("f4: %zu cases, %llu launch rounds checked, %llu tasks computed by the stand-ins\n", cases, (unsigned long long)standin::f4_rounds(), (unsigned long long)standin::f4_tasks());
    return 0;
}

/* ---- f4split: one bound of the sub-batch loops per invocation ---- */
template <class T>
static void cycle(std::vector<T> &v, size_t n)
{
    const size_t d = v.size();
    v.reserve(n);
    for (size_t k = d; k < n; ++k) v.push_back(v[k % d]);
}

static uint64_t packs() { return hipdbl::calls("launch_pack"); }

static void same_cycle_g(const std::vector<bsw_gresult> &res, const std::vector<uint32_t> &cig, int max_cigar, size_t n, size_t D, const char *what)
{
    for (size_t k = D; k < n; ++k) {
        CHECK(memcmp(&res[k], &res[k % D], sizeof(bsw_gresult)) == 0, "%s: result %zu differs from result %zu of the same task (score %d / %d, n_cigar %d / %d)", what, k, k % D,
              res[k].score, res[k % D].score, res[k].n_cigar, res[k % D].n_cigar);
        const int nc = std::min(std::max(res[k].n_cigar, 0), max_cigar);
        CHECK(nc == 0 || memcmp(&cig[k * (size_t)max_cigar], &cig[(k % D) * (size_t)max_cigar], (size_t)nc * 4) == 0, "%s: the CIGAR of result %zu differs from that of result %zu", what, k, k % D);
    }
}

static void global_split(bsw_ctx *ctx, const bsw_params &p, gwork &w, size_t n, int max_cigar, const char *what, uint64_t *sub)
{
    const size_t D = w.t.size();
    cycle(w.t, n);
    std::vector<bsw_gresult> res(n);
    std::vector<uint32_t> cig(n * (size_t)max_cigar);
    const uint64_t p0 = packs();
    const int rc = bsw_global_batch(ctx, &p, w.t.data(), n, max_cigar, res.data(), cig.data());
    CHECK(rc == BSW_OK, "%s: bsw_global_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    *sub = packs() - p0;
    for (size_t i = 0; i < D; ++i) {
        int nc = 0;
        uint32_t *cg = nullptr;
        const int score = ksw_global2_ref(w.t[i].qlen, w.q[i].data(), w.t[i].tlen, w.tg[i].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, w.t[i].w, &nc, &cg, nullptr);
        CHECK(nc <= max_cigar, "%s: distinct task %zu needs %d CIGAR words", what, i, nc);
        CHECK(res[i].score == score && res[i].n_cigar == nc, "%s: distinct task %zu: score %d n_cigar %d, the oracle's %d %d", what, i, res[i].score, res[i].n_cigar, score, nc);
        CHECK(memcmp(&cig[i * (size_t)max_cigar], cg, (size_t)nc * 4) == 0, "%s: distinct task %zu: the CIGAR differs from the oracle's", what, i);
        free(cg);
    }
    same_cycle_g(res, cig, max_cigar, n, D, what);
}

static void align_split(bsw_ctx *ctx, const bsw_params &p, awork &w, size_t n, const char *what, uint64_t *sub)
{
    const size_t D = w.t.size();
    cycle(w.t, n);
    std::vector<bsw_kswr> res(n);
    const uint64_t p0 = packs();
    const int rc = bsw_align_batch(ctx, &p, w.t.data(), n, res.data());
    CHECK(rc == BSW_OK, "%s: bsw_align_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    *sub = packs() - p0;
    for (size_t i = 0; i < D; ++i) {
        int32_t want[7];
        ksw_align2_ref(w.t[i].qlen, w.q[i].data(), w.t[i].tlen, w.tg[i].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, w.t[i].xtra, want, nullptr);
        CHECK(memcmp(&res[i], want, sizeof(want)) == 0, "%s: distinct task %zu: score %d te %d score2 %d tb %d, the oracle's %d %d %d %d", what, i, res[i].score, res[i].te, res[i].score2,
              res[i].tb, want[0], want[1], want[3], want[5]);
    }
    for (size_t k = D; k < n; ++k)
        CHECK(memcmp(&res[k], &res[k % D], sizeof(bsw_kswr)) == 0, "%s: result %zu differs from result %zu of the same task (score %d / %d, te %d / %d, score2 %d / %d)", what, k, k % D,
              res[k].score, res[k % D].score, res[k].te, res[k % D].te, res[k].score2, res[k % D].score2);
}

static void cigar_split(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, cwork &w, size_t n, int max_cigar, int max_md, FILE *f, const char *what, uint64_t *sub)
{
    const size_t D = w.t.size();
    cycle(w.t, n);
    std::vector<bsw_cresult> res;
    std::vector<uint32_t> cig;
    std::vector<char> md;
    const uint64_t p0 = packs();
    run_cigar(ctx, p, ref, w, max_cigar, max_md, true, true, f, what, D, &res, &cig, &md);
    *sub = packs() - p0;
    for (size_t k = D; k < n; ++k) {
        CHECK(memcmp(&res[k], &res[k % D], sizeof(bsw_cresult)) == 0, "%s: result %zu differs from result %zu of the same task (score %d / %d, nm %d / %d, tries %d / %d)", what, k, k % D,
              res[k].score, res[k % D].score, res[k].nm, res[k % D].nm, res[k].tries, res[k % D].tries);
        const int nc = std::min(std::max(res[k].n_cigar, 0), max_cigar);
        CHECK(nc == 0 || memcmp(&cig[k * (size_t)max_cigar], &cig[(k % D) * (size_t)max_cigar], (size_t)nc * 4) == 0, "%s: the CIGAR of result %zu differs from that of result %zu", what, k, k % D);
        CHECK(strcmp(&md[k * (size_t)max_md], &md[(k % D) * (size_t)max_md]) == 0, "%s: the MD of result %zu differs from that of result %zu", what, k, k % D);
    }
}

static void matesw_split(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, mwork &w, size_t n, FILE *f, const char *what, uint64_t *sub)
{
    const size_t D = w.t.size();
    cycle(w.t, n);
    std::vector<bsw_mresult> res;
    const uint64_t p0 = packs();
    run_matesw(ctx, p, ref, w, f, what, D, &res);
    *sub = packs() - p0;
    for (size_t k = D; k < n; ++k)
        CHECK(memcmp(&res[k], &res[k % D], sizeof(bsw_mresult)) == 0, "%s: result %zu differs from result %zu of the same task (score %d / %d, status %d / %d, rb %lld / %lld)", what, k, k % D,
              res[k].aln.score, res[k % D].aln.score, res[k].status, res[k % D].status, (long long)res[k].rb, (long long)res[k % D].rb);
}

/* D distinct tiny tasks, D odd, neighbours of different lengths */
static void tiny_global(gwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t D)
{
    for (size_t i = 0; i < D; ++i) {
        const int ql = 1 + (int)((i * 3) % 8), tl = 1 + (int)((i * 5 + 2) % 10);
        const int64_t at = r.below((int)(g.l_pac - 40));
        std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl), q(g.bases.begin() + at + (i % 2), g.bases.begin() + at + (i % 2) + ql);
        if (i % 3 == 0) q[q.size() / 2] = (uint8_t)((q[q.size() / 2] + 1) & 3);
        w.q.push_back(q); w.tg.push_back(tg);
    }
    for (size_t i = 0; i < D; ++i) {
        bsw_gtask t;
        memset(&t, 0, sizeof(t));
        t.qlen = (int)w.q[i].size(); t.tlen = (int)w.tg[i].size(); t.query = ar.put(w.q[i]); t.target = ar.put(w.tg[i]);
        t.w = abs(t.qlen - t.tlen) + 3;
        w.t.push_back(t);
    }
}

static void tiny_align(awork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t D, int tlen_fixed, int no_subo_every)
{
    for (size_t i = 0; i < D; ++i) {
        const int ql = 1 + (int)((i * 3) % 8), tl = tlen_fixed ? tlen_fixed - (int)(i % 2) * 7 : 9 + (int)((i * 7) % 30);
        const int64_t at = r.below((int)(g.l_pac - tl - 1));
        std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl);
        const int off = r.below(tl - ql + 1);
        std::vector<uint8_t> q(tg.begin() + off, tg.begin() + off + ql);
        for (int c = 0; c < 6; ++c) std::copy(q.begin(), q.end(), tg.begin() + r.below(tl - ql + 1));      /* planted repeats of the query */
        w.q.push_back(q); w.tg.push_back(tg);
    }
    for (size_t i = 0; i < D; ++i) {
        bsw_atask t;
        memset(&t, 0, sizeof(t));
        t.qlen = (int)w.q[i].size(); t.tlen = (int)w.tg[i].size(); t.query = ar.put(w.q[i]); t.target = ar.put(w.tg[i]);
        t.xtra = KSW_XSUBO | KSW_XSTART | ((i & 1) ? KSW_XBYTE : 0) | (t.qlen > 4 ? 4 : 1);
        if (no_subo_every && i % (size_t)no_subo_every == 1) t.xtra &= ~KSW_XSUBO;
        w.t.push_back(t);
    }
}

static void tiny_cigar(cwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t D)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < D; ++i) {
        bsw_ctask t;
        memset(&t, 0, sizeof(t));
        t.min_score = INT_MIN; t.max_tries = 1; t.w = 10;
        const bool rev = i % 2 == 1;
        const int rl = 3 + (int)((i * 3) % 8);
        int64_t rb = (rev ? L : 0) + r.below((int)(L - 20)), re = rb + rl;
        std::vector<uint8_t> q = g.seq(rb, re);
        if (i % 4 == 0 && q.size() > 4) q.erase(q.begin() + 2);                       /* a deletion from the read */
        if (i % 4 == 1) q[q.size() / 2] = (uint8_t)((q[q.size() / 2] + 2) & 3);       /* a mismatch */
        if (i % 4 == 2 && q.size() > 3) q.insert(q.begin() + 1, (uint8_t)r.below(4));
        if (i % 4 == 3) { q[0] = (uint8_t)((q[0] + 1) & 3); t.w = 0; }                 /* the no-gap shortcut */
        if (i == 5) { rb = L - 3; re = L + 4; }                                       /* status 1 */
        if (q.size() > 8) q.resize(8);
        w.q.push_back(q);
        t.l_query = (int)q.size(); t.rb = rb; t.re = re;
        w.t.push_back(t);
    }
    for (size_t i = 0; i < D; ++i) w.t[i].query = ar.put(w.q[i]);
}

static void tiny_matesw(mwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t D, int tlen_fixed, int no_subo_every)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < D; ++i) {
        bsw_mtask t;
        memset(&t, 0, sizeof(t));
        const int lm = 2 + (int)((i * 3) % 7), tl = tlen_fixed ? tlen_fixed - (int)(i % 2) * 5 : 12 + (int)((i * 7) % 30);
        const bool strand = i % 3 == 1;
        int64_t rb = (strand ? L : 0) + r.below((int)(L - tl - 1)), re = rb + tl;
        t.is_rev = (int)(i % 2);
        std::vector<uint8_t> win = g.seq(rb, re);
        const int off = r.below(tl - lm + 1);
        std::vector<uint8_t> aligned(win.begin() + off, win.begin() + off + lm);
        std::vector<uint8_t> ms = t.is_rev ? revcomp(aligned) : aligned;
        if (!tlen_fixed && i == 4) re = rb;                                           /* status 1 */
        t.xtra = KSW_XSUBO | KSW_XSTART | ((i & 1) ? KSW_XBYTE : 0) | (lm > 4 ? 4 : 2);
        if (no_subo_every && i % (size_t)no_subo_every == 1) t.xtra &= ~KSW_XSUBO;
        t.min_score = lm > 4 ? 4 : 2;
        t.l_ms = lm; t.rb = rb; t.re = re;
        w.m.push_back(ms);
        w.t.push_back(t);
    }
    for (size_t i = 0; i < D; ++i) w.t[i].mate = ar.put(w.m[i]);
}

static int f4split_mode(const std::string &which, const char *path)
{
    FILE *f = fopen(path, "w");
    CHECK(f, "cannot write %s", path);
    const bsw_params p = default_params();
    genome1_t g;
    g.make(which == "b" ? 700001 : 150001, 91);
    write_genome(f, g, p);
    uint64_t sub[4] = {0, 0, 0, 0};
    fresh(1);
    {
        rng_t r(4711);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 280000);      /* (the oracle computes a sub-batch for a minute: no watchdog) */
        bsw_ref *ref = nullptr;
        CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
        arena_t ar(1 << 20, true);
        if (which == "count") {                               /* 2^20 + 37 tasks per call */
            const size_t n = (1u << 20) + 37;
            { gwork w; tiny_global(w, ar, g, r, 11); global_split(ctx, p, w, n, 8, "count_global", &sub[0]); }
            { awork w; tiny_align(w, ar, g, r, 11, 0, 0); align_split(ctx, p, w, n, "count_align", &sub[1]); }
            { cwork w; tiny_cigar(w, ar, g, r, 13); cigar_split(ctx, p, ref, w, n, 6, 24, f, "count_cigar", &sub[2]); }
            { mwork w; tiny_matesw(w, ar, g, r, 9, 0, 0); matesw_split(ctx, p, ref, w, n, f, "count_matesw", &sub[3]); }
        } else if (which == "z") {                            /* more than 4 GiB of backtrack bytes in about 140 tasks */
            const size_t n = 141, D = 5;
            gwork gw;
            cwork cw;
            for (size_t i = 0; i < D; ++i) {
                const int tl = 8000 - (int)i * 3;
                const int64_t at = r.below((int)(g.l_pac - tl - 1));
                std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl), q = mutate(r, tg, 0.01, 0.002);
                if (q.size() > 8000) q.resize(8000);
                gw.q.push_back(q); gw.tg.push_back(tg);
                const bool rev = i % 2 == 1;
                const int64_t rb = (rev ? g.l_pac : 0) + r.below((int)(g.l_pac - tl - 1));
                std::vector<uint8_t> rd = mutate(r, g.seq(rb, rb + tl), 0.01, 0.002);
                if (rd.size() > 8000) rd.resize(8000);
                cw.q.push_back(rd);
                bsw_ctask t;
                memset(&t, 0, sizeof(t));
                t.l_query = (int)rd.size(); t.w = 3000; t.rb = rb; t.re = rb + tl; t.min_score = INT_MIN; t.max_tries = 1;
                cw.t.push_back(t);
            }
            arena_t big(D * 2 * 8200 * 2, false);
            for (size_t i = 0; i < D; ++i) {
                bsw_gtask t;
                memset(&t, 0, sizeof(t));
                t.qlen = (int)gw.q[i].size(); t.tlen = (int)gw.tg[i].size(); t.query = big.put(gw.q[i]); t.target = big.put(gw.tg[i]); t.w = 2000;
                gw.t.push_back(t);
                cw.t[i].query = big.put(cw.q[i]);
            }
            global_split(ctx, p, gw, n, 512, "z_global", &sub[0]);
            cigar_split(ctx, p, ref, cw, n, 512, 2048, f, "z_cigar", &sub[2]);
            sub[1] = sub[3] = 2;                              /* (not part of this invocation) */
        } else if (which == "b") {                            /* more than 2^28 target bases under KSW_XSUBO */
            /* 9 distinct windows, one of them without KSW_XSUBO (the loops count its bases towards the bound and give it no
             * slice): 4 134 of the 4 651 tasks carry a slice, 270.9 M entries */
            const size_t n = 4651;
            arena_t big(10 * 65600, false);
            { awork w; tiny_align(w, big, g, r, 9, 65535, 9); align_split(ctx, p, w, n, "b_align", &sub[1]); }
            { mwork w; tiny_matesw(w, big, g, r, 9, 65535, 9); matesw_split(ctx, p, ref, w, n, f, "b_matesw", &sub[3]); }
            sub[0] = sub[2] = 2;
        } else
            CHECK(false, "f4split count|z|b");
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "f4split: %zu HIP objects left alive after bsw_destroy", hipdbl::live_objects());
    fclose(f);
    printf("f4split %s: sub-batches global %llu align %llu cigar %llu matesw %llu\n", which.c_str(), (unsigned long long)sub[0], (unsigned long long)sub[1],
           (unsigned long long)sub[2], (unsigned long long)sub[3]);
    return 0;
}

/* ---- f4scalar: the scalar queue's three kinds at once ---- */
static int f4scalar_mode()
{
    fresh(1);
    genome1_t g;
    g.make(60001, 5);
    const int T = 12, ROUNDS = 40;
    struct scoring { int8_t mat[25]; int od, ed, oi, ei; };
    scoring sc[3];
    const int ab[3][2] = {{1, 4}, {2, 3}, {1, 2}};
    const int gp[3][4] = {{6, 1, 6, 1}, {5, 2, 7, 1}, {4, 1, 4, 1}};
    for (int s = 0; s < 3; ++s) {
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) sc[s].mat[i * 5 + j] = (int8_t)((i == 4 || j == 4) ? -1 : i == j ? ab[s][0] : -ab[s][1]);
        sc[s].od = gp[s][0]; sc[s].ed = gp[s][1]; sc[s].oi = gp[s][2]; sc[s].ei = gp[s][3];
    }
    std::vector<int> bad(T, 0);
    std::atomic<int> offender_bad{0}, done{0};
    std::vector<std::thread> th;
    for (int k = 0; k < T; ++k)
        th.emplace_back([&, k]() {
            rng_t r(300 + (uint64_t)k);
            for (int round = 0; round < ROUNDS; ++round) {
                const scoring &S = sc[(k + round) % 3];
                const int tl = r.in(40, 200);
                const int64_t at = r.below((int)(g.l_pac - tl - 1));
                std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl), q = mutate(r, tg, 0.05, 0.03);
                const int ql = (int)q.size(), w = abs(ql - tl) + 5;
                const int call = (k + round) % 5;
                if (call == 0 || call == 1) {
                    int nc = 0, wnc = 0;
                    uint32_t *cg = nullptr, *wcg = nullptr;
                    int got, want;
                    if (call == 0) {
                        got = ksw_global2(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, w, &nc, &cg);
                        want = ksw_global2_ref(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, w, &wnc, &wcg, nullptr);
                    } else {
                        got = ksw_global(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, w, &nc, &cg);
                        want = ksw_global2_ref(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.od, S.ed, w, &wnc, &wcg, nullptr);
                    }
                    if (got != want || nc != wnc || (nc && memcmp(cg, wcg, (size_t)nc * 4) != 0)) ++bad[(size_t)k];
                    free(cg); free(wcg);
                } else if (call == 2 || call == 3) {
                    const int ql2 = std::min(ql, 120);
                    const int xtra = KSW_XSUBO | KSW_XSTART | (round % 2 ? KSW_XBYTE : 0) | 10;
                    int32_t want[7];
                    kswr_t got;
                    if (call == 2) {
                        got = ksw_align2(ql2, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, xtra, nullptr);
                        ksw_align2_ref(ql2, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, xtra, want, nullptr);
                    } else {
                        got = ksw_align(ql2, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, xtra, nullptr);
                        ksw_align2_ref(ql2, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.od, S.ed, xtra, want, nullptr);
                    }
                    const int32_t g7[7] = {got.score, got.te, got.qe, got.score2, got.te2, got.tb, got.qb};
                    if (memcmp(g7, want, sizeof(want)) != 0) ++bad[(size_t)k];
                } else {
                    int gg[6], rr[6];
                    gg[0] = ksw_extend2(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, 100, 5, 100, 30, &gg[1], &gg[2], &gg[3], &gg[4], &gg[5]);
                    rr[0] = ksw_extend2_ref(ql, q.data(), tl, tg.data(), 5, S.mat, S.od, S.ed, S.oi, S.ei, 100, 5, 100, 30, &rr[1], &rr[2], &rr[3], &rr[4], &rr[5], BSW_VARIANT_H, nullptr);
                    if (memcmp(gg, rr, sizeof(gg)) != 0) ++bad[(size_t)k];
                }
            }
            ++done;
        });
    int offender_calls = 0;
    std::thread off([&]() {                                    /* one caller's over-limit task: only its own call fails */
        std::vector<uint8_t> q(g.bases.begin(), g.bases.begin() + 2000), tg(g.bases.begin() + 10, g.bases.begin() + 2300);
        while (done.load() < T || offender_calls < 3) {
            const kswr_t a = ksw_align2(2000, q.data(), 2290, tg.data(), 5, sc[offender_calls % 3].mat, 6, 1, 6, 1, KSW_XSTART, nullptr);
            if (a.score != -1) ++offender_bad;
            ++offender_calls;
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
    });
    for (auto &t : th) t.join();
    off.join();
    for (int k = 0; k < T; ++k) CHECK(bad[(size_t)k] == 0, "f4scalar: thread %d got %d answers that differ from the oracle's", k, bad[(size_t)k]);
    CHECK(offender_bad.load() == 0, "f4scalar: %d of the offender's %d over-limit calls did not answer score -1", offender_bad.load(), offender_calls);
    uint64_t calls = 0, trips = 0;
    bsw_scalar_stats(&calls, &trips);
    CHECK(calls == (uint64_t)(T * ROUNDS + offender_calls), "bsw_scalar_stats: %llu calls, made %d", (unsigned long long)calls, T * ROUNDS + offender_calls);
    CHECK(trips >= 1 && trips < calls, "bsw_scalar_stats: %llu trips for %llu calls: nothing was coalesced", (unsigned long long)trips, (unsigned long long)calls);
    printf("f4scalar: %llu calls in %llu trips, offender calls %d\n", (unsigned long long)calls, (unsigned long long)trips, offender_calls);
    return 0;
}

/* ---- faults: call k of a clean run's C fails, for every k ---- */
struct f4_outputs {
    std::vector<bsw_gresult> g; std::vector<uint32_t> gc;
    std::vector<bsw_kswr> a;
    std::vector<bsw_cresult> c; std::vector<uint32_t> cc; std::vector<char> cm;
    std::vector<bsw_mresult> m;
    bool operator==(const f4_outputs &o) const
    {
        if (g.size() != o.g.size() || a.size() != o.a.size() || c.size() != o.c.size() || m.size() != o.m.size()) return false;
        if (!g.empty() && memcmp(g.data(), o.g.data(), g.size() * sizeof(bsw_gresult)) != 0) return false;
        for (size_t i = 0; i < g.size(); ++i)
            for (int k = 0; k < g[i].n_cigar; ++k) if (gc[i * 48 + (size_t)k] != o.gc[i * 48 + (size_t)k]) return false;
        if (!a.empty() && memcmp(a.data(), o.a.data(), a.size() * sizeof(bsw_kswr)) != 0) return false;
        if (!c.empty() && memcmp(c.data(), o.c.data(), c.size() * sizeof(bsw_cresult)) != 0) return false;
        for (size_t i = 0; i < c.size(); ++i) {
            for (int k = 0; k < c[i].n_cigar; ++k) if (cc[i * 64 + (size_t)k] != o.cc[i * 64 + (size_t)k]) return false;
            if (strcmp(&cm[i * 512], &o.cm[i * 512]) != 0) return false;
        }
        if (!m.empty() && memcmp(m.data(), o.m.data(), m.size() * sizeof(bsw_mresult)) != 0) return false;
        return true;
    }
};

static int f4faults_mode(const std::string &call)
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(90001, 13);
    const size_t n = 180;
    sweep_t s;
    s.releases = {"hipFree", "hipHostFree", "hipGetLastError"};        /* releases whose return code is ignored by design */
    s.tickets = false;
    s.exact = true;
    for (int reg = 0; reg < 2; ++reg) {                        /* both memory kinds: the gather and the direct branch */
        f4_outputs clean;
        fault_sweep(s, 1, [&](sweep_t &s) {
            const unsigned long long k = s.k;
            rng_t r(31);
            arena_t ar(n * 900 + 8192, reg != 0);
            gwork gw; awork aw; cwork cw; mwork mw;
            if (call == "global") make_global(gw, ar, g, r, n);
            else if (call == "align") make_align(aw, ar, g, r, n);
            else if (call == "cigar") make_cigar(cw, ar, g, r, n);
            else if (call == "matesw") make_matesw(mw, ar, g, r, n);
            else CHECK(false, "faults global|align|cigar|matesw");
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 3000);
            bsw_ref *ref = upload(ctx, g);
            auto run = [&](f4_outputs &o) {
                o = f4_outputs();
                if (call == "global") { o.g.assign(n, bsw_gresult{0, 0}); o.gc.assign(n * 48, 0); return bsw_global_batch(ctx, &p, gw.t.data(), n, 48, o.g.data(), o.gc.data()); }
                if (call == "align") { o.a.resize(n); memset(o.a.data(), 0, n * sizeof(bsw_kswr)); return bsw_align_batch(ctx, &p, aw.t.data(), n, o.a.data()); }
                if (call == "cigar") {
                    o.c.resize(n); memset(o.c.data(), 0, n * sizeof(bsw_cresult)); o.cc.assign(n * 64, 0); o.cm.assign(n * 512, 0);
                    return bsw_cigar_ref_batch(ctx, &p, ref, cw.t.data(), n, 64, o.cc.data(), 512, o.cm.data(), o.c.data());
                }
                o.m.resize(n); memset(o.m.data(), 0, n * sizeof(bsw_mresult));
                return bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), n, o.m.data());
            };
            s.arm();
            f4_outputs first, again;
            const int rc = run(first);
            s.judge({{rc, rc ? bsw_last_error(ctx) : ""}});
            if (k == 0) {
                clean = first;
                if (call == "cigar") {
                    int two = 0;
                    for (const bsw_cresult &c : clean.c) two += c.tries >= 2 && c.status == 0;
                    CHECK(two >= 10 && hipdbl::calls("launch_global") + hipdbl::calls("launch_global_long") >= 3, "the cigar batch of the fault sweep needs no second try");
                }
                printf("faults %s, %s memory: C = %llu\n", call.c_str(), reg ? "registered" : "pageable", (unsigned long long)s.C);
            } else if (rc == BSW_OK)                           /* no failure happened, or that of a release */
                CHECK(first == clean, "k=%llu: %s failed, the call reported success and its results differ", k, s.fname.c_str());
            const int rc2 = run(again);                         /* the same call on the same context */
            CHECK(rc2 == BSW_OK, "k=%llu (%s failed): the same call repeated -> %d (%s)", k, s.fname.c_str(), rc2, bsw_last_error(ctx));
            CHECK(again == clean, "k=%llu (%s failed): the same call repeated is not bit-exact", k, s.fname.c_str());
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
        });
    }
    printf("faults %s: C = %llu, injection points visited = %llu, failed calls %llu, ignored releases %llu, skipped 0\n", call.c_str(), (unsigned long long)s.Csum,
           (unsigned long long)s.visited, (unsigned long long)s.failed, (unsigned long long)s.ignored);
    s.done();
    return 0;
}

/* ---- cuts: the sub-batch cutter on its own.  Every property is stated over the costs, not by cutting a second time: a task joins
 * a span only while no bound objects (probed with its probe values against what the span has accumulated), and a span that ends
 * before n ends because a bound objects to the next task.  A round keeps one bound tight and the others out of reach, so that the
 * bound that closed a span is known. ---- */
static int cuts_mode()
{
    enum { TASKS, Z, SEQ, BL, OUT, WORK, KINDS };
    const char *names[KINDS] = {"tasks", "z", "seq", "bl", "out", "work"};
    uint64_t closed_by[KINDS] = {0, 0, 0, 0, 0, 0}, spans_seen = 0;
    rng_t r(2024);
    for (int round = 0; round < 6000; ++round) {
        const int tight = round % (KINDS + 1);                /* KINDS: every bound in reach at once */
        const size_t n = round < 8 ? (size_t)round / 4 : (size_t)r.below(70);       /* n = 0 and n = 1 first */
        std::vector<span_cost> c(n);
        for (span_cost &x : c) {
            x.z_probe = (uint64_t)r.below(50); x.z = r.below(4) ? x.z_probe : 0;
            x.bl_probe = (uint64_t)r.below(50); x.bl = r.below(4) ? x.bl_probe : 0;
            x.seq = (uint64_t)r.below(50); x.work = (uint64_t)r.below(60);
        }
        span_caps caps;                                       /* the hosts' own: out of reach of these costs */
        auto in_reach = [&](int k) { return tight == k || tight == KINDS; };
        if (in_reach(TASKS)) caps.tasks = (uint64_t)r.in(1, 9);
        if (in_reach(Z)) caps.z = (uint64_t)r.in(30, 200);
        if (in_reach(SEQ)) caps.seq = (uint64_t)r.in(30, 200);
        if (in_reach(BL)) caps.bl = (uint64_t)r.in(30, 200);
        if (in_reach(OUT)) { caps.out_per_task = (uint64_t)r.in(1, 16); caps.out = (uint64_t)r.in(8, 120); }
        if (in_reach(WORK)) caps.work = (uint64_t)r.in(1, 300);
        if (n == 1) {                                         /* one task over every cap: a span of its own */
            c[0] = span_cost{1000, 1000, 1000, 1000, 1000, 1000};
            caps.tasks = 1; caps.z = caps.seq = caps.bl = caps.work = 10; caps.out_per_task = 50; caps.out = 10;
        }
        const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) { return c[i]; }, caps);
        CHECK(n || spans.empty(), "cuts: %zu spans for no task", spans.size());
        CHECK(n != 1 || spans.size() == 1, "cuts: %zu spans for one task", spans.size());
        size_t at = 0;
        for (const chunk_span &s : spans) {
            CHECK(s.base == at && s.cnt >= 1 && s.base + s.cnt <= n, "cuts: span [%zu, +%zu) behind %zu of %zu tasks", s.base, s.cnt, at, n);
            at += s.cnt;
            ++spans_seen;
            /* objections to task j joining what the span holds by then; j == end: to the task behind the span */
            uint64_t z = 0, sq = 0, bl = 0, wk = 0;
            auto objections = [&](size_t j, bool *why) {
                why[TASKS] = j - s.base >= caps.tasks;
                why[Z] = z + c[j].z_probe > caps.z; why[SEQ] = sq + c[j].seq > caps.seq; why[BL] = bl + c[j].bl_probe > caps.bl;
                why[OUT] = (uint64_t)(j - s.base + 1) * caps.out_per_task > caps.out;
                why[WORK] = wk >= caps.work;
                int k = 0;
                for (int i = 0; i < KINDS; ++i) k += why[i] ? 1 : 0;
                return k;
            };
            bool why[KINDS];
            for (size_t j = s.base; j < s.base + s.cnt; ++j) {
                if (j > s.base) {
                    CHECK(objections(j, why) == 0, "cuts: task %zu joined span [%zu, +%zu) over a bound (round %d)", j, s.base, s.cnt, round);
                    CHECK(wk < caps.work, "cuts: span [%zu, +%zu) went on at task %zu with its work target reached", s.base, s.cnt, j);
                }
                z += c[j].z; sq += c[j].seq; bl += c[j].bl; wk += c[j].work;
            }
            if (s.cnt > 1)                                    /* no hard cap is exceeded but by a single task */
                CHECK(s.cnt <= caps.tasks && z <= caps.z && sq <= caps.seq && bl <= caps.bl && (uint64_t)s.cnt * caps.out_per_task <= caps.out,
                      "cuts: span [%zu, +%zu) exceeds a hard cap (round %d)", s.base, s.cnt, round);
            if (s.base + s.cnt < n) {
                const int k = objections(s.base + s.cnt, why);
                CHECK(k >= 1, "cuts: span [%zu, +%zu) of %zu tasks was closed with room for the next task (round %d)", s.base, s.cnt, n, round);
                if (tight == WORK) CHECK(why[WORK] && wk >= caps.work && wk - c[s.base + s.cnt - 1].work < caps.work,
                                         "cuts: span [%zu, +%zu) holds %llu of work under a target of %llu", s.base, s.cnt, (unsigned long long)wk, (unsigned long long)caps.work);
                if (k == 1)
                    for (int i = 0; i < KINDS; ++i) closed_by[i] += why[i] ? 1 : 0;
            }
        }
        CHECK(at == n, "cuts: the spans cover %zu of %zu tasks", at, n);
    }
    for (int i = 0; i < KINDS; ++i) CHECK(closed_by[i] >= 20, "cuts: the %s bound alone closed %llu spans", names[i], (unsigned long long)closed_by[i]);
    printf("cuts: ok, %llu spans, closed by tasks %llu z %llu seq %llu bl %llu out %llu work %llu\n", (unsigned long long)spans_seen, (unsigned long long)closed_by[TASKS],
           (unsigned long long)closed_by[Z], (unsigned long long)closed_by[SEQ], (unsigned long long)closed_by[BL], (unsigned long long)closed_by[OUT], (unsigned long long)closed_by[WORK]);
    return 0;
}

/* ---- rejects: what bsw_align_batch, bsw_matesw_ref_batch and ksw_align2 / ksw_align refuse in 8-bit mode (include/bwa_sw_mi355.h
 * at KSW_XBYTE), per task, and that the neighbouring cases run and equal the oracle ---- */
static int rejects_mode()
{
    fresh(1);
    genome1_t g;
    g.make(40001, 9);
    rng_t r(4242);
    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
    bsw_ref *ref = nullptr;
    CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
    const size_t N = 7;
    arena_t ar(N * 1400 + 8192, false);
    awork aw;
    make_align(aw, ar, g, r, N);
    mwork mw;
    make_matesw(mw, ar, g, r, N);
    for (size_t i = 0; i < N; ++i) {                                   /* every window runs */
        bsw_mtask &t = mw.t[i];
        if (t.l_ms == 0) { t.l_ms = 1; t.mate = g.bases.data(); }
        t.rb = 100 + 50 * (int64_t)i; t.re = t.rb + t.l_ms + 120;
    }
    struct kase { const char *what; int lo; int od, ed, oi, ei; bool byte_last, byte_all; int want; const char *needle; };
    /* lo: -1 the default matrix, else every entry drawn from lo + 1 .. 7 and one entry set to lo */
    const kase K[] = {
        {"min 2, one 8-bit task", 2, 6, 1, 6, 1, true, false, BSW_E_INVAL, "smallest entry is 2"},
        {"min 2, 16-bit", 2, 6, 1, 6, 1, false, false, BSW_OK, ""},
        {"min 1, one 8-bit task", 1, 6, 1, 6, 1, true, false, BSW_E_INVAL, "smallest entry is 1"},
        {"min 0, 8-bit", 0, 6, 1, 6, 1, true, true, BSW_OK, ""},
        {"o_del + e_del = 256, one 8-bit task", -1, 255, 1, 6, 1, true, false, BSW_E_LIMIT, "above 255"},
        {"o_del + e_del = 256, 16-bit", -1, 255, 1, 6, 1, false, false, BSW_OK, ""},
        {"o_ins + e_ins = 256, one 8-bit task", -1, 6, 1, 200, 56, true, false, BSW_E_LIMIT, "above 255"},
        {"both sums 255, 8-bit", -1, 250, 5, 254, 1, true, true, BSW_OK, ""},
    };
    size_t refused = 0, ran = 0;
    for (const kase &k : K) {
        bsw_params p = default_params();
        if (k.lo >= 0) {
            for (int i = 0; i < 25; ++i) p.mat[i] = (int8_t)r.in(k.lo + 1, 7);
            p.mat[7] = (int8_t)k.lo;
        }
        p.o_del = k.od; p.e_del = k.ed; p.o_ins = k.oi; p.e_ins = k.ei;
        for (size_t i = 0; i < N; ++i) {
            const int x = ((k.byte_all || (k.byte_last && i + 1 == N)) ? KSW_XBYTE : 0) | KSW_XSUBO | KSW_XSTART | 19;
            aw.t[i].xtra = x; mw.t[i].xtra = x;
        }
        char tag[32];
        snprintf(tag, sizeof(tag), "task %zu", N - 1);
        if (k.want == BSW_OK) {
            check_align(ctx, p, aw, k.what);                       /* runs, and equals the oracle */
            run_matesw(ctx, p, ref, mw, nullptr, k.what);
            ++ran;
        } else {
            std::vector<bsw_kswr> ares(N);
            int rc = bsw_align_batch(ctx, &p, aw.t.data(), N, ares.data());
            CHECK(rc == k.want && strstr(bsw_last_error(ctx), k.needle) && strstr(bsw_last_error(ctx), "KSW_XBYTE") && strstr(bsw_last_error(ctx), tag),
                  "%s: bsw_align_batch -> %d (%s), wanted %d with '%s'", k.what, rc, bsw_last_error(ctx), k.want, k.needle);
            std::vector<bsw_mresult> mres(N);
            rc = bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), N, mres.data());
            CHECK(rc == k.want && strstr(bsw_last_error(ctx), k.needle) && strstr(bsw_last_error(ctx), "KSW_XBYTE") && strstr(bsw_last_error(ctx), tag),
                  "%s: bsw_matesw_ref_batch -> %d (%s), wanted %d with '%s'", k.what, rc, bsw_last_error(ctx), k.want, k.needle);
            ++refused;
        }
        /* the scalar ABI: the last task as ksw_align2's call (score -1 = the call's failure), ksw_align where both kinds share their penalties */
        const bsw_atask &t = aw.t[N - 1];
        int32_t want[7];
        ksw_align2_ref(t.qlen, aw.q[N - 1].data(), t.tlen, aw.tg[N - 1].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, t.xtra, want, nullptr);
        const kswr_t got = ksw_align2(t.qlen, (uint8_t *)aw.q[N - 1].data(), t.tlen, (uint8_t *)aw.tg[N - 1].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, t.xtra, nullptr);
        const int32_t g7[7] = {got.score, got.te, got.qe, got.score2, got.te2, got.tb, got.qb};
        if (k.want == BSW_OK) CHECK(memcmp(g7, want, sizeof(want)) == 0, "%s: ksw_align2 score %d te %d, the oracle's %d %d", k.what, got.score, got.te, want[0], want[1]);
        else CHECK(got.score == -1, "%s: ksw_align2 answered score %d, not the call's failure", k.what, got.score);
        if (k.od == k.oi && k.ed == k.ei) {
            const kswr_t g1 = ksw_align(t.qlen, (uint8_t *)aw.q[N - 1].data(), t.tlen, (uint8_t *)aw.tg[N - 1].data(), 5, p.mat, p.o_del, p.e_del, t.xtra, nullptr);
            CHECK(k.want == BSW_OK ? g1.score == want[0] : g1.score == -1, "%s: ksw_align answered score %d", k.what, g1.score);
        }
    }
    bsw_ref_free(ctx, ref);
    bsw_destroy(ctx);
    printf("rejects: %zu cases refused, %zu ran\n", refused, ran);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rejects") return rejects_mode();
    if (mode == "f4" && argc > 2) return f4_mode(argv[2]);
    if (mode == "f4split" && argc > 3) return f4split_mode(argv[2], argv[3]);
    if (mode == "f4scalar") return f4scalar_mode();
    if (mode == "faults" && argc > 2) return f4faults_mode(argv[2]);
    if (mode == "cuts") return cuts_mode();
    fprintf(stderr, "usage: host_f4 f4 FILE | f4split count|z|b FILE | f4scalar | faults global|align|cigar|matesw | cuts | rejects\n");
    return 2;
}
