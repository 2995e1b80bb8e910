/* host_patch.cpp — bsw_patch_ref_batch, bsw_patch_ref_submit_t and bsw_patch_reads_submit_t (mem_patch_reg: bsw_cigar.hip, its
 * tickets through bsw_batch.hip's pipeline) on the host-memory HIP stand-in, plain and under ASan / UBSan or TSan (TEST INFRASTRUCTURE;
 * tests/test_patch_double_cpu.py builds it with its row in tests/_host_double_build.py and runs it).  A stand-alone program: nothing is
 * preloaded, no GPU is opened.
 *
 *   host_patch parity   the batch call and both ticket forms on 1, 2 and 3 devices, registered and pageable reads, against the C
 *                       oracle's ksw_global2 for the score and a C restatement of mem_patch_reg's arithmetic around it
 *   host_patch checks   every validation code; nothing is queued by a rejected call; the argument, reference and BSW_E_BUSY
 *                       answers of all nine entry points of the CIGAR, mate-rescue and patch stages
 *   host_patch cuts     (under BSW_F4_PATCH_WORK) the batch call's sub-batches and the tickets' chunks
 *   host_patch mixed    a patch ticket in flight beside an extension and a CIGAR ticket; the fifth submit is BUSY; bsw_reads_free
 *                       is BUSY until the reads ticket is collected
 *   host_patch faults   every HIP / launcher call of one submit of each patch form fails in turn
 */
#include <climits>
#include "host_ref_patch.h"

/* ---- the workload: reads of 150 / 250 / a few long bases off both strands, cut into two regions around an indel ---- */
struct pwork {
    std::vector<std::vector<uint8_t>> reads;
    std::vector<bsw_ptask> t;
    std::vector<bsw_rd_ptask> rt;
    std::vector<bsw_presult> want;
    std::vector<const uint8_t *> ptr;
    std::vector<int32_t> len;
    uint8_t *arena = nullptr;
    bool registered = false;
    size_t n_run = 0, n_short = 0, n_rev = 0, by_status[3] = {0, 0, 0};
    ~pwork() { if (registered) bsw_host_free(arena); else free(arena); }
    pwork() = default;
    pwork(const pwork &) = delete;
};

static void make_patch(pwork &w, const genome_t &g, const bsw_params &p, rng_t &r, size_t n, bool registered)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < n; ++i) {
        const int kind = (int)(i % 16);
        const bool rev = (i / 16) % 2 == 1;
        int len = i % 3 ? 150 : 250;
        if (kind == 15 && i % 5 == 0) len = i % 2 ? 1030 : 2100;           /* the LDS-ring classes */
        int64_t x = (rev ? L : 0) + 200 + r.below((int)(L - len - 600));
        if (kind == 9) x = L - len + 20;                                   /* the joined interval bridges l_pac: no alignment */
        const int cut = r.in(45, len - 45);
        int d = kind == 7 || kind == 8 ? 0 : r.in(0, 6);                   /* 7, 8: the no-gap shortcut and its neighbour */
        if (len > 1000) d = 2;
        const bool ins = r.below(2) == 1;
        std::vector<uint8_t> q(g.both.begin() + x, g.both.begin() + x + cut);
        if (ins) for (int k = 0; k < d; ++k) q.push_back((uint8_t)r.below(4));
        const int dele = ins ? 0 : d, nins = ins ? d : 0;
        const int tail = len - cut - nins;
        q.insert(q.end(), g.both.begin() + x + cut + dele, g.both.begin() + x + cut + dele + tail);
        for (auto &c : q) if (r.unit() < 0.005) c = (uint8_t)((c + 1 + r.below(3)) & 3);
        if (kind == 10) for (auto &c : q) if (r.unit() < 0.03) c = 4;      /* Ns */
        bsw_ptask t;
        memset(&t, 0, sizeof(t));
        t.l_query = len;
        const int aqb = r.in(0, 5), aqe = cut + r.in(-8, 8), bqe = len - r.in(0, 5);
        int bqb = cut + nins + r.in(-8, 8);
        if (kind == 7 || kind == 8) bqb = aqe + r.in(-4, 4);
        t.a = bsw_preg{x + aqb, x + aqe, aqb, aqe, aqe - aqb - r.in(0, 6), r.in(0, 20)};
        const int64_t brb = x + cut + dele + (bqb - cut - nins);
        t.b = bsw_preg{brb, brb + (bqe - bqb), bqb, bqe, bqe - bqb - r.in(0, 6), r.in(0, 20)};
        if (kind == 7) t.a.w = t.b.w = 0;
        if (kind == 8) { t.a.w = 0; t.b.w = 1; }
        if (kind == 11 && !rev) { t.b.rb += L; t.b.re += L; }              /* the other strand */
        if (kind == 12) { t.b.qb = t.a.qb; t.b.qe = t.a.qb + (bqe - bqb); }       /* not colinear */
        if (kind == 13) { const int sh = r.in(250, 600); t.b.rb += sh; t.b.re += sh; }      /* beyond the band */
        if (kind == 14) for (size_t k = (size_t)std::min(aqe, bqb); k < q.size(); ++k) q[k] = (uint8_t)r.below(4);       /* junk: the ratio fails */
        w.reads.push_back(q);
        w.t.push_back(t);
    }
    size_t bytes = 64;
    for (auto &q : w.reads) bytes += q.size() + 3;
    w.registered = registered;
    w.arena = (uint8_t *)(registered ? bsw_host_alloc(bytes) : malloc(bytes));
    CHECK(w.arena, "arena");
    memset(w.arena, 0, bytes);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        memcpy(w.arena + at, w.reads[i].data(), w.reads[i].size());
        w.t[i].query = w.arena + at;
        at += w.reads[i].size() + (i % 4);                                 /* every alignment of a read's first byte */
        bsw_rd_ptask rt;
        memset(&rt, 0, sizeof(rt));
        rt.read = (uint32_t)i; rt.a = w.t[i].a; rt.b = w.t[i].b;
        w.rt.push_back(rt);
        w.ptr.push_back(w.reads[i].data());
        w.len.push_back((int32_t)w.reads[i].size());
        bool sc = false;
        w.want.push_back(ref_patch(p, g, w.reads[i].data(), w.t[i].a, w.t[i].b, &sc));
        const bsw_presult &x = w.want.back();
        ++w.by_status[x.status];
        if (x.status != 1) { ++w.n_run; w.n_short += sc; w.n_rev += w.t[i].a.rb >= L; }
    }
}

static void same_p(const std::vector<bsw_presult> &got, const pwork &w, size_t n, const char *what)
{
    for (size_t i = 0; i < n; ++i)
        if (memcmp(&got[i], &w.want[i], sizeof(bsw_presult)) != 0)
            CHECK(false, "%s: task %zu of %zu: got score %d w %d gscore %d status %d, want %d %d %d %d", what, i, n, got[i].score, got[i].w, got[i].gscore,
                  got[i].status, w.want[i].score, w.want[i].w, w.want[i].gscore, w.want[i].status);
}

static std::vector<bsw_presult> fresh_out(size_t n)
{
    std::vector<bsw_presult> o(n + 1);
    memset(o.data(), 0x5a, o.size() * sizeof(bsw_presult));
    return o;
}
static void guard_ok(const std::vector<bsw_presult> &o, const char *what)
{
    CHECK(o.back().score == 0x5a5a5a5a && o.back().status == 0x5a5a5a5a, "%s: a write behind the caller's array", what);
}

/* the three forms on one context; returns the chunks the two tickets ran */
static uint64_t three_forms(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const pwork &w, const char *what)
{
    const size_t n = w.t.size();
    std::vector<bsw_presult> o = fresh_out(n);
    int rc = bsw_patch_ref_batch(ctx, &p, ref, w.t.data(), n, o.data());
    CHECK(rc == BSW_OK, "%s: bsw_patch_ref_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    guard_ok(o, what);
    same_p(o, w, n, what);
    const uint64_t c0 = stats_of(ctx).chunks;
    std::vector<bsw_presult> o1 = fresh_out(n), o2 = fresh_out(n);
    bsw_ticket t1 = 0, t2 = 0;
    rc = bsw_patch_ref_submit_t(ctx, &p, ref, w.t.data(), n, o1.data(), &t1);
    CHECK(rc == BSW_OK && t1, "%s: bsw_patch_ref_submit_t -> %d (%s)", what, rc, bsw_last_error(ctx));
    bsw_reads *rd = upload_reads(ctx, w);
    rc = bsw_patch_reads_submit_t(ctx, &p, ref, rd, w.rt.data(), n, o2.data(), &t2);
    CHECK(rc == BSW_OK && t2 && t2 != t1, "%s: bsw_patch_reads_submit_t -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "%s: bsw_reads_free while the reads ticket is uncollected", what);
    CHECK(bsw_wait_ticket(ctx, t1) == BSW_OK, "%s: the pointer ticket: %s", what, bsw_last_error(ctx));
    CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "%s: bsw_reads_free while the reads ticket is uncollected", what);
    CHECK(bsw_wait_ticket(ctx, t2) == BSW_OK, "%s: the reads ticket: %s", what, bsw_last_error(ctx));
    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "%s: bsw_reads_free after the ticket was collected: %s", what, bsw_last_error(ctx));
    guard_ok(o1, what);
    guard_ok(o2, what);
    CHECK(memcmp(o1.data(), o.data(), n * sizeof(bsw_presult)) == 0, "%s: the pointer ticket differs from the batch call", what);
    CHECK(memcmp(o2.data(), o.data(), n * sizeof(bsw_presult)) == 0, "%s: the reads ticket differs from the batch call", what);
    return stats_of(ctx).chunks - c0;
}

static int parity_mode()
{
    bsw_params p = default_params();
    genome_t g;
    g.make(70001, 5);
    for (int reg = 0; reg < 2; ++reg)
        for (int D : {1, 2, 3}) {
            fresh(D);
            {
                rng_t r(40 + (uint64_t)D);
                pwork w;
                make_patch(w, g, p, r, 640, reg != 0);
                CHECK(w.by_status[0] >= 100 && w.by_status[1] >= 100 && w.by_status[2] >= 40 && w.n_short >= 20 && w.n_rev >= 100,
                      "the workload: statuses %zu %zu %zu, shortcut %zu, reverse %zu", w.by_status[0], w.by_status[1], w.by_status[2], w.n_short, w.n_rev);
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, D, 256, 2, 20000);
                bsw_ref *ref = upload(ctx, g);
                three_forms(ctx, p, ref, w, reg ? "registered reads" : "pageable reads");
                /* n == 0 completes at once, with and without a ticket */
                bsw_ticket t = 0;
                CHECK(bsw_patch_ref_batch(ctx, &p, ref, nullptr, 0, nullptr) == BSW_OK, "an empty batch");
                CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, nullptr, 0, nullptr, &t) == BSW_OK && t && bsw_test(ctx, t) == 1 && bsw_wait_ticket(ctx, t) == BSW_OK, "an empty submit");
                CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, nullptr, 0, nullptr, nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "an empty submit without a ticket");
                /* a batch in which nothing passes the pre-tests makes no HIP call at all */
                std::vector<bsw_ptask> none;
                for (size_t i = 0; i < w.t.size(); ++i) if (w.want[i].status == 1 && !(w.t[i].a.rb < g.l_pac && w.t[i].b.re > g.l_pac && w.t[i].b.rb < g.l_pac)) none.push_back(w.t[i]);
                std::vector<bsw_presult> o = fresh_out(none.size());
                const uint64_t packs = hipdbl::calls("launch_pack");
                CHECK(bsw_patch_ref_batch(ctx, &p, ref, none.data(), none.size(), o.data()) == BSW_OK, "a batch of rejected pairs: %s", bsw_last_error(ctx));
                CHECK(hipdbl::calls("launch_pack") == packs, "a batch of rejected pairs reached the device");
                for (size_t i = 0; i < none.size(); ++i) CHECK(o[i].status == 1 && !o[i].score && !o[i].w && !o[i].gscore, "a rejected pair's record");
                /* a general matrix and four distinct penalties */
                bsw_params p2 = p;
                const int8_t m5[25] = {3, -4, -2, -5, -1, -3, 2, -6, -2, -1, -5, -3, 4, -4, -2, -2, -6, -3, 2, -1, -1, -2, -1, -2, -1};
                memcpy(p2.mat, m5, 25);
                p2.o_del = 5; p2.e_del = 2; p2.o_ins = 7; p2.e_ins = 1;
                pwork w2;
                rng_t r2(77);
                make_patch(w2, g, p2, r2, 200, reg != 0);
                three_forms(ctx, p2, ref, w2, "general matrix");
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
            }
            CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
        }
    printf("parity ok\n");
    return 0;
}

/* ---- what the nine entry points of the three stages against the resident reference (CIGAR, mate rescue, region patch; each as a
 * batch call, a ticket and a ticket by read index) share in front of their own checks: a NULL p, a NULL result array with n > 0
 * and a reference of another context answer BSW_E_INVAL, write no ticket and queue nothing; with BSW_MAX_INFLIGHT tickets
 * uncollected every ticket form answers BSW_E_BUSY, and one by read index gives its block back.  Task `good` of w runs. ---- */
static void nine_entry_points(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_ref *oref, bsw_reads *rd, const pwork &w, size_t good)
{
    const bsw_ptask &pt = w.t[good];
    bsw_ctask ct;
    memset(&ct, 0, sizeof(ct));
    ct.query = pt.query + pt.a.qb; ct.l_query = pt.b.qe - pt.a.qb; ct.w = w.want[good].w; ct.rb = pt.a.rb; ct.re = pt.b.re; ct.min_score = INT_MIN; ct.max_tries = 1;
    bsw_rd_ctask rct;
    memset(&rct, 0, sizeof(rct));
    rct.read = (uint32_t)good; rct.qb = pt.a.qb; rct.qe = pt.b.qe; rct.w = ct.w; rct.rb = ct.rb; rct.re = ct.re; rct.min_score = INT_MIN; rct.max_tries = 1;
    bsw_mtask mt;
    memset(&mt, 0, sizeof(mt));
    mt.mate = pt.query; mt.l_ms = pt.l_query; mt.rb = pt.a.rb; mt.re = pt.b.re; mt.xtra = KSW_XSTART | 10; mt.min_score = 19;
    bsw_rd_mtask rmt;
    memset(&rmt, 0, sizeof(rmt));
    rmt.read = (uint32_t)good; rmt.rb = mt.rb; rmt.re = mt.re; rmt.xtra = mt.xtra; rmt.min_score = mt.min_score;
    const bsw_rd_ptask &rpt = w.rt[good];
    bsw_cresult cres[1];
    bsw_mresult mres[1];
    bsw_presult pres[1];
    uint32_t cig[64];
    /* one task through an entry point: pp and rf as given, no result array when !res; tk == NULL for the batch calls */
    struct entry {
        const char *name;
        bool ticket, reads;
        std::function<int(const bsw_params *, const bsw_ref *, bool, bsw_ticket *)> call;
    };
    const entry entries[9] = {
        {"bsw_cigar_ref_batch", false, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *) { return bsw_cigar_ref_batch(ctx, pp, rf, &ct, 1, 64, cig, 0, nullptr, res ? cres : nullptr); }},
        {"bsw_cigar_ref_submit_t", true, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_cigar_ref_submit_t(ctx, pp, rf, &ct, 1, 64, cig, 0, nullptr, res ? cres : nullptr, tk); }},
        {"bsw_cigar_reads_submit_t", true, true, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_cigar_reads_submit_t(ctx, pp, rf, rd, &rct, 1, 64, cig, 0, nullptr, res ? cres : nullptr, tk); }},
        {"bsw_matesw_ref_batch", false, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *) { return bsw_matesw_ref_batch(ctx, pp, rf, &mt, 1, res ? mres : nullptr); }},
        {"bsw_matesw_ref_submit_t", true, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_matesw_ref_submit_t(ctx, pp, rf, &mt, 1, res ? mres : nullptr, tk); }},
        {"bsw_matesw_reads_submit_t", true, true, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_matesw_reads_submit_t(ctx, pp, rf, rd, &rmt, 1, res ? mres : nullptr, tk); }},
        {"bsw_patch_ref_batch", false, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *) { return bsw_patch_ref_batch(ctx, pp, rf, &pt, 1, res ? pres : nullptr); }},
        {"bsw_patch_ref_submit_t", true, false, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_patch_ref_submit_t(ctx, pp, rf, &pt, 1, res ? pres : nullptr, tk); }},
        {"bsw_patch_reads_submit_t", true, true, [&](const bsw_params *pp, const bsw_ref *rf, bool res, bsw_ticket *tk) { return bsw_patch_reads_submit_t(ctx, pp, rf, rd, &rpt, 1, res ? pres : nullptr, tk); }},
    };
    const uint64_t submits0 = stats_of(ctx).submits;
    for (const entry &en : entries) {
        const struct { const char *what; const bsw_params *pp; const bsw_ref *rf; bool res; } bad[3] = {
            {"a NULL p", nullptr, ref, true}, {"a NULL result array", &p, ref, false}, {"the reference of another context", &p, oref, true}};
        for (const auto &b : bad) {
            const uint64_t calls = hipdbl::overall_calls();
            bsw_ticket tk = 77;
            const int rc = en.call(b.pp, b.rf, b.res, &tk);
            CHECK(rc == BSW_E_INVAL, "%s with %s -> %d (%s)", en.name, b.what, rc, bsw_last_error(ctx));
            CHECK(*bsw_last_error(ctx), "%s with %s: no text", en.name, b.what);
            CHECK(!en.ticket || tk == 0, "%s with %s wrote ticket %llu", en.name, b.what, (unsigned long long)tk);
            CHECK(bsw_inflight(ctx) == 0 && hipdbl::overall_calls() == calls, "%s with %s queued something", en.name, b.what);
        }
    }
    /* BSW_MAX_INFLIGHT tickets live (complete or not: uncollected), none of them by read index */
    std::vector<bsw_presult> lo = fresh_out(BSW_MAX_INFLIGHT);
    bsw_ticket lt[BSW_MAX_INFLIGHT];
    for (int k = 0; k < BSW_MAX_INFLIGHT; ++k)
        CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, &pt, 1, &lo[(size_t)k], &lt[k]) == BSW_OK && lt[k], "live ticket %d: %s", k, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == BSW_MAX_INFLIGHT, "%d tickets live", bsw_inflight(ctx));
    for (const entry &en : entries) {
        bsw_ticket tk = 77;
        const int rc = en.call(&p, ref, true, &tk);
        CHECK(rc == BSW_E_BUSY, "%s beside %d live tickets -> %d (%s)", en.name, BSW_MAX_INFLIGHT, rc, bsw_last_error(ctx));
        CHECK(!en.ticket || tk == 0, "%s answered BSW_E_BUSY and wrote ticket %llu", en.name, (unsigned long long)tk);
        CHECK(bsw_inflight(ctx) == BSW_MAX_INFLIGHT && stats_of(ctx).submits == submits0 + BSW_MAX_INFLIGHT, "%s: BSW_E_BUSY changed something", en.name);
    }
    for (int k = 0; k < BSW_MAX_INFLIGHT; ++k) {
        CHECK(bsw_wait_ticket(ctx, lt[k]) == BSW_OK, "live ticket %d: %s", k, bsw_last_error(ctx));
        CHECK(memcmp(&lo[(size_t)k], &w.want[good], sizeof(bsw_presult)) == 0, "live ticket %d: its result", k);
    }
    CHECK(bsw_inflight(ctx) == 0, "tickets left");
    /* (the caller frees rd next: a refused submit by read index that kept the block would make that BSW_E_BUSY) */
}

/* ---- every validation code ---- */
static int checks_mode()
{
    const bsw_params p = default_params();
    genome_t g;
    g.make(200001, 6);
    fresh(2);
    {
        rng_t r(3);
        pwork w;
        make_patch(w, g, p, r, 32, false);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 20000), *other = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 20000);
        bsw_ref *ref = upload(ctx, g), *oref = upload(other, g);
        bsw_reads *rd = upload_reads(ctx, w), *ord = upload_reads(other, w);
        size_t good = 0;
        while (w.want[good].status == 1) ++good;
        std::vector<bsw_presult> o = fresh_out(4);
        int tried = 0;
        /* a task list of [good, bad]: all three forms answer `code`, write no ticket, queue nothing */
        auto expect = [&](int code, const char *what, const bsw_params &pp, std::function<void(bsw_preg &, bsw_preg &, bsw_ptask &, bsw_rd_ptask &)> spoil, bool pointer_only = false, bool reads_only = false) {
            bsw_ptask t[2] = {w.t[good], w.t[good]};
            bsw_rd_ptask rt[2] = {w.rt[good], w.rt[good]};
            spoil(t[1].a, t[1].b, t[1], rt[1]);
            rt[1].a = t[1].a; rt[1].b = t[1].b;
            const uint64_t calls = hipdbl::overall_calls();
            bsw_ticket tk = 77;
            if (!reads_only) {
                CHECK(bsw_patch_ref_batch(ctx, &pp, ref, t, 2, o.data()) == code, "%s: bsw_patch_ref_batch -> not %d (%s)", what, code, bsw_last_error(ctx));
                CHECK(*bsw_last_error(ctx), "%s: no text", what);
                CHECK(bsw_patch_ref_submit_t(ctx, &pp, ref, t, 2, o.data(), &tk) == code && tk == 0, "%s: bsw_patch_ref_submit_t -> not %d (%s)", what, code, bsw_last_error(ctx));
            }
            if (!pointer_only) {
                tk = 77;
                CHECK(bsw_patch_reads_submit_t(ctx, &pp, ref, rd, rt, 2, o.data(), &tk) == code && tk == 0, "%s: bsw_patch_reads_submit_t -> not %d (%s)", what, code, bsw_last_error(ctx));
            }
            CHECK(bsw_inflight(ctx) == 0 && hipdbl::overall_calls() == calls, "%s: a rejected call queued something", what);
            ++tried;
        };
        typedef bsw_preg R;
        typedef bsw_ptask T;
        typedef bsw_rd_ptask RT;
        expect(BSW_E_INVAL, "NULL read", p, [](R &, R &, T &t, RT &) { t.query = nullptr; }, true);
        expect(BSW_E_INVAL, "a.rb >= a.re", p, [](R &a, R &, T &, RT &) { a.re = a.rb; });
        expect(BSW_E_INVAL, "b.rb >= b.re", p, [](R &, R &b, T &, RT &) { b.re = b.rb - 1; });
        expect(BSW_E_INVAL, "a.qb < 0", p, [](R &a, R &, T &, RT &) { a.qb = -1; });
        expect(BSW_E_INVAL, "a.qb >= a.qe", p, [](R &a, R &, T &, RT &) { a.qe = a.qb; });
        expect(BSW_E_INVAL, "b.qe > l_query", p, [](R &, R &b, T &t, RT &) { b.qe = t.l_query + 1; });
        expect(BSW_E_INVAL, "b.qb >= b.qe", p, [](R &, R &b, T &, RT &) { b.qb = b.qe; });
        expect(BSW_E_INVAL, "a.rb > b.rb", p, [](R &a, R &b, T &, RT &) { std::swap(a.rb, b.rb); std::swap(a.re, b.re); });
        expect(BSW_E_INVAL, "a.w < 0", p, [](R &a, R &, T &, RT &) { a.w = -1; });
        expect(BSW_E_INVAL, "b.w < 0", p, [](R &, R &b, T &, RT &) { b.w = -1; });
        expect(BSW_E_INVAL, "a.score + b.score <= 0", p, [](R &a, R &b, T &, RT &) { a.score = -b.score; });
        bsw_params pw = p;
        pw.w = -1;
        expect(BSW_E_INVAL, "p->w < 0", pw, [](R &, R &, T &, RT &) {});
        expect(BSW_E_INVAL, "read >= n_reads", p, [&](R &, R &, T &, RT &rt) { rt.read = (uint32_t)w.rt.size(); }, false, true);
        CHECK(tried == 13, "cases");
        /* limits: only for a task that passes the pre-tests */
        {
            const int LQ = BSW_GLOBAL_MAX_QLEN + 1;
            std::vector<uint8_t> big((size_t)LQ + 10);
            for (int i = 0; i < LQ + 10; ++i) big[(size_t)i] = g.both[(size_t)(1000 + i)];
            bsw_ptask t;
            memset(&t, 0, sizeof(t));
            t.query = big.data(); t.l_query = LQ + 10;
            t.a = R{1000, 1000 + 4000, 0, 4000, 3900, 5};
            t.b = R{1000 + 4000, 1000 + LQ, 4000, LQ, LQ - 4100, 0};
            CHECK(bsw_patch_ref_batch(ctx, &p, ref, &t, 1, o.data()) == BSW_E_LIMIT, "8 192 joined bases: %s", bsw_last_error(ctx));
            bsw_ticket tk = 77;
            CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, &t, 1, o.data(), &tk) == BSW_E_LIMIT && tk == 0, "8 192 joined bases as a ticket");
            bsw_ptask u = t;                                                /* ... the same task failing a pre-test is no error and never runs */
            u.b.qb = u.a.qb;
            const uint64_t packs = hipdbl::calls("launch_pack");
            CHECK(bsw_patch_ref_batch(ctx, &p, ref, &u, 1, o.data()) == BSW_OK && o[0].status == 1 && hipdbl::calls("launch_pack") == packs, "a long task that fails a pre-test");
            t.b.qe = LQ - 1; t.b.re = 1000 + LQ - 1;                       /* 8 191: accepted */
            CHECK(bsw_patch_ref_batch(ctx, &p, ref, &t, 1, o.data()) == BSW_OK && o[0].status != 1, "8 191 joined bases: %s", bsw_last_error(ctx));
            const bsw_presult want = ref_patch(p, g, big.data(), t.a, t.b);
            CHECK(memcmp(&o[0], &want, sizeof(want)) == 0, "8 191 joined bases: %d %d %d %d, want %d %d %d %d", o[0].score, o[0].w, o[0].gscore, o[0].status, want.score, want.w, want.gscore, want.status);
            /* a joined reference interval beyond BSW_MAX_TLEN: regions long enough for the band and the ratio to pass */
            bsw_params pl = p;
            pl.w = 20000;
            std::vector<uint8_t> rdq(8000);
            for (size_t i = 0; i < rdq.size(); ++i) rdq[i] = g.both[2000 + i];
            bsw_ptask v;
            memset(&v, 0, sizeof(v));
            v.query = rdq.data(); v.l_query = 8000;
            v.a = R{2000, 2000 + 33000, 0, 4000, 3000, 0};
            v.b = R{2000 + 33000, 2000 + BSW_MAX_TLEN + 1, 4000, 8000, 3000, 0};
            int wv = 0;
            CHECK(bsw_patch_pretest(&pl, g.l_pac, &v.a, &v.b, &wv) == 1, "the long interval passes the pre-tests");
            CHECK(bsw_patch_ref_batch(ctx, &pl, ref, &v, 1, o.data()) == BSW_E_LIMIT, "a joined interval of 65 536 bases: %s", bsw_last_error(ctx));
        }
        /* the reference or the read block of another context */
        bsw_ticket tk = 77;
        CHECK(bsw_patch_ref_batch(ctx, &p, oref, w.t.data(), 2, o.data()) == BSW_E_INVAL, "a foreign reference");
        CHECK(bsw_patch_ref_submit_t(ctx, &p, oref, w.t.data(), 2, o.data(), &tk) == BSW_E_INVAL && tk == 0, "a foreign reference as a ticket");
        CHECK(bsw_patch_reads_submit_t(ctx, &p, ref, ord, w.rt.data(), 2, o.data(), &tk) == BSW_E_INVAL && tk == 0, "a foreign read block");
        CHECK(bsw_patch_reads_submit_t(ctx, &p, ref, nullptr, w.rt.data(), 2, o.data(), &tk) == BSW_E_INVAL, "no read block");
        CHECK(bsw_patch_ref_batch(ctx, nullptr, ref, w.t.data(), 2, o.data()) == BSW_E_INVAL && bsw_patch_ref_batch(ctx, &p, ref, w.t.data(), 2, nullptr) == BSW_E_INVAL, "NULL arguments");
        CHECK(bsw_patch_ref_batch(nullptr, &p, ref, w.t.data(), 2, o.data()) == BSW_E_INVAL, "no context");
        CHECK(bsw_inflight(ctx) == 0, "nothing was queued");
        nine_entry_points(ctx, p, ref, oref, rd, w, good);
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK && bsw_reads_free(other, ord) == BSW_OK, "a rejected reads submit gives its block back");
        bsw_ref_free(ctx, ref);
        bsw_ref_free(other, oref);
        bsw_destroy(ctx);
        bsw_destroy(other);
    }
    CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    printf("checks ok\n");
    return 0;
}

/* ---- cuts: BSW_F4_PATCH_WORK (read once per process: the test sets it) cuts the batch call and the tickets ---- */
static int cuts_mode()
{
    CHECK(getenv("BSW_F4_PATCH_WORK"), "run under BSW_F4_PATCH_WORK");
    const bsw_params p = default_params();
    genome_t g;
    g.make(70001, 5);
    fresh(2);
    {
        rng_t r(9);
        pwork w;
        make_patch(w, g, p, r, 480, true);
        const int devices[2] = {0, 0};                                     /* one ordinal listed twice */
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 20000, devices);
        bsw_ref *ref = upload(ctx, g);
        const uint64_t packs = hipdbl::calls("launch_pack");
        std::vector<bsw_presult> o = fresh_out(w.t.size());
        CHECK(bsw_patch_ref_batch(ctx, &p, ref, w.t.data(), w.t.size(), o.data()) == BSW_OK, "bsw_patch_ref_batch: %s", bsw_last_error(ctx));
        same_p(o, w, w.t.size(), "sub-batches");
        const uint64_t sub = hipdbl::calls("launch_pack") - packs;
        CHECK(sub >= 5, "the batch call ran %llu sub-batches", (unsigned long long)sub);
        const uint64_t chunks = three_forms(ctx, p, ref, w, "cut tickets");
        CHECK(chunks >= 10, "the two tickets ran %llu chunks", (unsigned long long)chunks);
        printf("cuts: %llu sub-batches, %llu chunks of two tickets\n", (unsigned long long)sub, (unsigned long long)chunks);
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    printf("cuts ok\n");
    return 0;
}

/* ---- mixed: beside an extension and a CIGAR ticket ---- */
static int mixed_mode()
{
    const bsw_params p = default_params();
    genome_t g;
    g.make(70001, 5);
    fresh(2);
    {
        rng_t r(21);
        pwork w;
        make_patch(w, g, p, r, 320, true);
        workload we;
        make_workload(we, 1500, 150, 9, true);
        const std::vector<bsw_result> want_e = expected(p, we.tasks.data(), 1500);
        /* bwa_gen_cigar2 with its CIGAR on the intervals of the pairs that run: its score is gscore */
        std::vector<bsw_ctask> ct;
        std::vector<size_t> of;
        for (size_t i = 0; i < w.t.size(); ++i) {
            if (w.want[i].status == 1) continue;
            bsw_ctask c;
            memset(&c, 0, sizeof(c));
            c.query = w.t[i].query + w.t[i].a.qb; c.l_query = w.t[i].b.qe - w.t[i].a.qb; c.w = w.want[i].w; c.rb = w.t[i].a.rb; c.re = w.t[i].b.re;
            c.min_score = INT_MIN; c.max_tries = 1;
            ct.push_back(c);
            of.push_back(i);
        }
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 20000);
        bsw_ref *ref = upload(ctx, g);
        bsw_reads *rd = upload_reads(ctx, w);
        std::vector<bsw_result> eo(1500);
        std::vector<bsw_cresult> co(ct.size());
        std::vector<bsw_presult> po = fresh_out(w.t.size()), ro = fresh_out(w.t.size()), extra = fresh_out(w.t.size());
        bsw_ticket t[4] = {0, 0, 0, 0}, t5 = 77;
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), 1500, eo.data(), &t[0]) == BSW_OK, "extension: %s", bsw_last_error(ctx));
        CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, ct.data(), ct.size(), 64, nullptr, 0, nullptr, co.data(), &t[1]) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
        CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, w.t.data(), w.t.size(), po.data(), &t[2]) == BSW_OK, "patch: %s", bsw_last_error(ctx));
        CHECK(bsw_patch_reads_submit_t(ctx, &p, ref, rd, w.rt.data(), w.rt.size(), ro.data(), &t[3]) == BSW_OK, "patch by read index: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 4 && t[0] && t[1] && t[2] && t[3], "four tickets");
        const bsw_stats s0 = stats_of(ctx);
        CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, w.t.data(), w.t.size(), extra.data(), &t5) == BSW_E_BUSY && t5 == 0, "the fifth submit");
        CHECK(bsw_patch_reads_submit_t(ctx, &p, ref, rd, w.rt.data(), w.rt.size(), extra.data(), &t5) == BSW_E_BUSY && t5 == 0, "the fifth submit by read index");
        CHECK(bsw_patch_ref_batch(ctx, &p, ref, w.t.data(), w.t.size(), extra.data()) == BSW_E_BUSY, "the synchronous call beside tickets");
        CHECK(bsw_inflight(ctx) == 4 && stats_of(ctx).submits == s0.submits, "BSW_E_BUSY changes nothing");
        CHECK(extra[0].score == 0x5a5a5a5a, "a refused submit wrote results");
        CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with the reads ticket in flight");
        for (int k : {2, 0}) {
            CHECK(bsw_wait_ticket(ctx, t[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with the reads ticket uncollected");
        }
        CHECK(bsw_wait_ticket(ctx, t[3]) == BSW_OK, "the reads ticket: %s", bsw_last_error(ctx));
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free once the reads ticket is collected: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, t[1]) == BSW_OK, "the CIGAR ticket: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 0, "tickets left");
        same_p(po, w, w.t.size(), "the patch ticket beside others");
        same_p(ro, w, w.t.size(), "the reads patch ticket beside others");
        CHECK(memcmp(eo.data(), want_e.data(), 1500 * sizeof(bsw_result)) == 0, "the extension ticket beside a patch ticket");
        for (size_t k = 0; k < ct.size(); ++k)
            CHECK(co[k].status == 0 && co[k].score == w.want[of[k]].gscore, "CIGAR task %zu: score %d, the patch's gscore %d", k, co[k].score, w.want[of[k]].gscore);
        /* the fifth submit works once a ticket has been collected */
        CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, w.t.data(), w.t.size(), extra.data(), &t5) == BSW_OK && t5 && bsw_wait_ticket(ctx, t5) == BSW_OK, "a submit after the wait");
        same_p(extra, w, w.t.size(), "a submit after the wait");
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    printf("mixed ok\n");
    return 0;
}

/* ---- faults: call k of a submit of each patch form fails, for every k ---- */
static int faults_mode()
{
    const bsw_params p = default_params();
    genome_t g;
    g.make(70001, 5);
    sweep_t s;
    /* releases whose code is ignored by design; a slot thread's hipSetDevice when the slot gets no chunk of these one-chunk
       tickets (it tries again in front of its next job) */
    s.releases = {"hipSetDevice", "hipFree", "hipHostFree", "hipGetLastError", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister", "hipEventQuery"};
    s.min_visited = 60; s.min_failed = 50;
    for (int reg = 0; reg < 2; ++reg)
        fault_sweep(s, 2, [&](sweep_t &s) {
            const unsigned long long k = s.k;
            rng_t r(31);
            pwork w;
            make_patch(w, g, p, r, 96, reg != 0);
            const size_t n = w.t.size();
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 4000);
            bsw_ref *ref = upload(ctx, g);
            bsw_reads *rd = upload_reads(ctx, w);
            std::vector<bsw_presult> o0 = fresh_out(n), o1 = fresh_out(n), o2 = fresh_out(n);
            s.arm();
            bsw_ticket t[2] = {0, 0};
            const int rb = bsw_patch_ref_batch(ctx, &p, ref, w.t.data(), n, o0.data());
            const std::string tb = rb ? bsw_last_error(ctx) : "";
            int rs[2], rc[3];
            std::string text[3];
            rs[0] = bsw_patch_ref_submit_t(ctx, &p, ref, w.t.data(), n, o1.data(), &t[0]);
            rs[1] = bsw_patch_reads_submit_t(ctx, &p, ref, rd, w.rt.data(), n, o2.data(), &t[1]);
            /* (the pipeline's own start may be what fails: then the submit answers, no ticket is made) */
            for (int j = 0; j < 2; ++j) {
                rc[j] = rs[j] ? rs[j] : bsw_wait_ticket(ctx, t[j]);
                text[j] = rc[j] ? bsw_last_error(ctx) : "";
            }
            rc[2] = rb; text[2] = tb;
            s.judge({{rc[0], text[0]}, {rc[1], text[1]}, {rc[2], text[2]}});
            if (rc[2] == BSW_OK) same_p(o0, w, n, "a batch call that reported success");
            if (rc[0] == BSW_OK) same_p(o1, w, n, "a ticket that reported success");
            if (rc[1] == BSW_OK) same_p(o2, w, n, "a reads ticket that reported success");
            if (k == 0) printf("faults, %s memory: C = %llu\n", reg ? "registered" : "pageable", (unsigned long long)s.C);
            CHECK(bsw_inflight(ctx) == 0, "tickets left");
            /* the context is alive (an injected return code never kills it): every form once more, bit-exact */
            CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "k=%llu: bsw_reads_free after the tickets: %s", k, bsw_last_error(ctx));
            three_forms(ctx, p, ref, w, "after the failure");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
        });
    printf("faults: injection points visited = %llu, a call failed %llu times, ignored %llu\n", (unsigned long long)s.visited, (unsigned long long)s.failed, (unsigned long long)s.ignored);
    s.done();
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "parity") return parity_mode();
    if (mode == "checks") return checks_mode();
    if (mode == "cuts") return cuts_mode();
    if (mode == "mixed") return mixed_mode();
    if (mode == "faults") return faults_mode();
    fprintf(stderr, "usage: host_patch parity | checks | cuts | mixed | faults\n");
    return 2;
}
