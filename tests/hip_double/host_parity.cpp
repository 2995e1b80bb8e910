/* host_parity.cpp — the whole host path of the library on the host-memory HIP stand-in, under ASan / UBSan or TSan: every
 * result equal to the oracle's, byte for byte, in task order (TEST INFRASTRUCTURE; tests/test_host_double_cpu.py).
 *   host_parity cross     resident / submit / packed / extend_batch over n x kernel x read length x memory kind x variant
 *   host_parity ref       bsw_extend_ref and bsw_submit_ref against the resident reference
 *   host_parity wire      the 256 KiB / 16 KiB wire format end to end
 *   host_parity scalar    the drop-in ksw_extend2 from 8 threads
 *   host_parity devices   2, 3 and 8 devices, and one ordinal listed twice
 *   host_parity big K     120 000 two-sided 250 bp seeds as a resident batch under kernel mode K (0 AUTO, 1 WAVE, 2 LANE)
 *   host_parity tables    the class of probe seeds under this program's class tables (compared with the built library's), and
 *                         the stand-ins' align and global class tables (compared with the kernel sources' initialisers)
 */
#include <algorithm>
#include <set>
#include "host_common.h"

static const size_t NS[] = {0, 1, 63, 64, 65, 5000};
static const int KERNELS[] = {BSW_KERNEL_AUTO, BSW_KERNEL_LANE, BSW_KERNEL_WAVE};

static bsw_params params_of(int variant)
{
    bsw_params p;
    bsw_default_params(&p);
    p.variant = variant;
    return p;
}

static void run_resident(bsw_ctx *ctx, const bsw_params &p, const workload &w, const std::vector<bsw_result> &want, const char *what)
{
    const size_t n = w.tasks.size();
    bsw_dev_batch *b = nullptr;
    int rc = bsw_upload(ctx, &p, w.tasks.data(), n, &b);
    CHECK(rc == BSW_OK, "%s: bsw_upload -> %d (%s)", what, rc, bsw_last_error(ctx));
    rc = bsw_run(ctx, b);
    CHECK(rc == BSW_OK, "%s: bsw_run -> %d (%s)", what, rc, bsw_last_error(ctx));
    std::vector<bsw_result> got(n + 1);
    memset(got.data(), 0x5a, got.size() * sizeof(bsw_result));
    rc = bsw_download(ctx, b, got.data());
    CHECK(rc == BSW_OK, "%s: bsw_download -> %d (%s)", what, rc, bsw_last_error(ctx));
    same_results(got.data(), want.data(), n, what);
    bsw_free_batch(ctx, b);
}

static void run_submit(bsw_ctx *ctx, const bsw_params &p, const workload &w, const std::vector<bsw_result> &want, bool packed, bool reg_out, const char *what)
{
    const size_t n = w.tasks.size();
    bsw_result *got = (bsw_result *)(reg_out ? bsw_host_alloc((n + 1) * sizeof(bsw_result)) : malloc((n + 1) * sizeof(bsw_result)));
    memset(got, 0x5a, (n + 1) * sizeof(bsw_result));
    std::vector<bsw_task> pt;
    uint64_t *parena = nullptr;
    const bsw_task *tasks = w.tasks.data();
    if (packed) {
        const size_t cap = bsw_pack_tasks_bound(tasks, n);
        parena = (uint64_t *)(w.registered ? bsw_host_alloc(cap) : malloc(cap));
        pt.resize(n ? n : 1);
        CHECK(bsw_pack_tasks(tasks, n, parena, cap, pt.data()) >= 0, "%s: bsw_pack_tasks", what);
        tasks = pt.data();
    }
    int rc = packed ? bsw_submit_packed(ctx, &p, tasks, n, got) : bsw_submit(ctx, &p, tasks, n, got);
    CHECK(rc == BSW_OK, "%s: submit -> %d (%s)", what, rc, bsw_last_error(ctx));
    rc = bsw_wait(ctx);
    CHECK(rc == BSW_OK, "%s: bsw_wait -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 0, "%s: submits left in flight", what);
    same_results(got, want.data(), n, what);
    if (parena) { if (w.registered) bsw_host_free(parena); else free(parena); }
    if (reg_out) bsw_host_free(got); else free(got);
}

static void run_ext_batch(bsw_ctx *ctx, const bsw_params &p, const workload &w, const char *what)
{
    std::vector<bsw_ext_task> xt;
    for (size_t i = 0; i < w.tasks.size(); ++i) {
        const bsw_task &t = w.tasks[i];
        if (t.rqlen < 1) continue;
        bsw_ext_task x;
        memset(&x, 0, sizeof(x));
        x.query = t.rquery; x.target = t.rtarget; x.qlen = t.rqlen; x.tlen = t.rtlen;
        x.w = (i % 3 == 0) ? 30 : 100; x.end_bonus = (i % 5 == 0) ? 0 : 5; x.h0 = t.h0;
        xt.push_back(x);
    }
    const size_t n = xt.size();
    std::vector<bsw_ext> got(n + 1), want(n + 1);
    if (p.variant == BSW_VARIANT_RTL) rtl_ref_ext_batch(&p, xt.data(), n, want.data());
    else bsw_ext_batch_ref(&p, xt.data(), n, want.data(), 8);
    const int rc = bsw_extend_batch(ctx, &p, xt.data(), n, got.data());
    CHECK(rc == BSW_OK, "%s: bsw_extend_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    for (size_t i = 0; i < n; ++i) CHECK(memcmp(&got[i], &want[i], sizeof(bsw_ext)) == 0, "%s: ext record %zu of %zu differs (score %d / %d)", what, i, n, got[i].score, want[i].score);
}

static int cross()
{
    size_t cases = 0;
    for (int variant : {BSW_VARIANT_H, BSW_VARIANT_M, BSW_VARIANT_RTL})
        for (int read_len : {150, 250})
            for (int reg = 0; reg < 2; ++reg) {
                if (variant != BSW_VARIANT_H && !(read_len == 150 && reg == 1)) continue;     /* (M and RTL: one read length, one memory kind) */
                for (size_t n : NS)
                    for (int kernel : KERNELS) {
                        char what[160];
                        snprintf(what, sizeof(what), "variant %d, %d bp, %s, n %zu, kernel %d", variant, read_len, reg ? "registered" : "pageable", n, kernel);
                        fresh(1);
                        {
                            const bsw_params p = params_of(variant);
                            workload w;
                            make_workload(w, n, read_len, 11 + n + (uint64_t)read_len, reg != 0);
                            const std::vector<bsw_result> want = expected(p, w.tasks.data(), n);
                            bsw_ctx *ctx = make_ctx(kernel, 1, 256);      /* 5 000 seeds: 20 chunks */
                            run_resident(ctx, p, w, want, (std::string("resident, ") + what).c_str());
                            run_submit(ctx, p, w, want, false, reg != 0, (std::string("bsw_submit, ") + what).c_str());
                            run_submit(ctx, p, w, want, true, reg != 0, (std::string("bsw_submit_packed, ") + what).c_str());
                            if (read_len == 150) run_ext_batch(ctx, p, w, (std::string("bsw_extend_batch, ") + what).c_str());
                            bsw_destroy(ctx);
                        }
                        CHECK(hipdbl::live_objects() == 0, "%s: %zu HIP objects left alive after bsw_destroy", what, hipdbl::live_objects());
                        ++cases;
                    }
            }
    printf("cross: %zu cases\n", cases);
    return 0;
}

/* ---- the resident reference ---- */
struct ref_workload {
    std::vector<uint8_t> pac;
    int64_t l_pac = 0;
    std::vector<bsw_ref_task> rt;
    uint8_t *arena = nullptr;
    bool registered = false;
    std::vector<bsw_task> tasks;                     /* the same seeds as host tasks (expected results) */
    std::vector<uint8_t> seqs;
    ~ref_workload() { if (registered) bsw_host_free(arena); else free(arena); }
};

static void make_ref_workload(ref_workload &w, const bsw_params &p, size_t n, int read_len, uint64_t seed, bool registered)
{
    bsw_synth_spec sp;
    memset(&sp, 0, sizeof(sp));
    sp.seed = seed; sp.read_len = read_len; sp.seed_len_min = 19; sp.seed_len_max = 40; sp.sub_rate = 0.03; sp.indel_rate = 0.008;
    sp.n_rate = 0.004; sp.junk_frac = 0.1; sp.a = 1; sp.w = 100; sp.o = 6; sp.e = 1;
    w.l_pac = 60001;
    w.pac.assign((size_t)((w.l_pac + 3) >> 2), 0);
    w.rt.resize(n ? n : 1);
    const size_t alen = n * (size_t)read_len + 64;
    w.registered = registered;
    w.arena = (uint8_t *)(registered ? bsw_host_alloc(alen) : malloc(alen));
    memset(w.arena, 0, alen);
    CHECK(bsw_synth_ref_generate(&sp, &p, w.l_pac, w.pac.data(), n, w.rt.data(), w.arena, alen) >= 0, "bsw_synth_ref_generate");
    w.rt.resize(n);
    /* mem_chain2aln on the host: the window's bases, one task per seed */
    size_t need = 0;
    for (size_t i = 0; i < n; ++i) need += (size_t)(w.rt[i].rmax1 - w.rt[i].rmax0) + bsw_seed_scratch_bytes(&w.rt[i].seed, w.rt[i].rmax0) + 16;
    w.seqs.assign(need + 16, 0);
    w.tasks.resize(n);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        bsw_ref_task &r = w.rt[i];
        r.tag = (uint32_t)i;
        uint8_t *rseq = w.seqs.data() + at;
        const int64_t got = bsw_pac_get_seq(w.l_pac, w.pac.data(), r.rmax0, r.rmax1, rseq);
        CHECK(got == r.rmax1 - r.rmax0, "bsw_pac_get_seq");
        at += (size_t)got;
        const size_t sl = bsw_seed_scratch_bytes(&r.seed, r.rmax0);
        CHECK(bsw_seed_to_task(&p, &r.seed, r.l_query, r.query, r.rmax0, r.rmax1, rseq, w.seqs.data() + at, sl, r.tag, &w.tasks[i]) == BSW_OK, "bsw_seed_to_task");
        w.tasks[i].init_score = r.init_score;
        at += sl;
    }
}

static int ref_mode()
{
    size_t cases = 0;
    for (int read_len : {150, 250})
        for (int reg = 0; reg < 2; ++reg)
            for (size_t n : NS)
                for (int kernel : KERNELS) {
                    char what[160];
                    snprintf(what, sizeof(what), "%d bp, %s, n %zu, kernel %d", read_len, reg ? "registered" : "pageable", n, kernel);
                    fresh(1);
                    {
                        const bsw_params p = params_of(BSW_VARIANT_H);
                        ref_workload w;
                        make_ref_workload(w, p, n, read_len, 5 + n, reg != 0);
                        const std::vector<bsw_result> want = expected(p, w.tasks.data(), n);
                        bsw_ctx *ctx = make_ctx(kernel, 1, 256);
                        bsw_ref *ref = nullptr;
                        CHECK(bsw_ref_upload(ctx, w.pac.data(), w.l_pac, &ref) == BSW_OK, "%s: bsw_ref_upload: %s", what, bsw_last_error(ctx));
                        std::vector<bsw_result> got(n + 1);
                        int rc = bsw_extend_ref(ctx, &p, ref, w.rt.data(), n, got.data());
                        CHECK(rc == BSW_OK, "bsw_extend_ref, %s -> %d (%s)", what, rc, bsw_last_error(ctx));
                        same_results(got.data(), want.data(), n, (std::string("bsw_extend_ref, ") + what).c_str());
                        memset(got.data(), 0x5a, got.size() * sizeof(bsw_result));
                        rc = bsw_submit_ref(ctx, &p, ref, w.rt.data(), n, got.data());
                        CHECK(rc == BSW_OK, "bsw_submit_ref, %s -> %d (%s)", what, rc, bsw_last_error(ctx));
                        rc = bsw_wait(ctx);
                        CHECK(rc == BSW_OK, "bsw_submit_ref + bsw_wait, %s -> %d (%s)", what, rc, bsw_last_error(ctx));
                        same_results(got.data(), want.data(), n, (std::string("bsw_submit_ref, ") + what).c_str());
                        bsw_ref_free(ctx, ref);
                        bsw_destroy(ctx);
                    }
                    CHECK(hipdbl::live_objects() == 0, "%s: %zu HIP objects left alive", what, hipdbl::live_objects());
                    ++cases;
                }
    printf("ref: %zu cases\n", cases);
    return 0;
}

/* ---- the wire format ---- */
static int wire_mode()
{
    for (int variant : {BSW_VARIANT_H, BSW_VARIANT_RTL}) {
        fresh(1);
        {
            bsw_params p = params_of(variant);
            p.zdrop = 0;
            workload w;
            make_workload(w, 2400, 150, 77, false);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 0);
            std::vector<std::vector<uint32_t>> ins, outs, wants;
            size_t lo = 0;
            while (lo < w.tasks.size()) {
                std::vector<uint32_t> words(BSW_REFBATCH_IN_WORDS, 0);
                const int k = bsw_refbatch_encode(&p, w.tasks.data() + lo, std::min<size_t>(w.tasks.size() - lo, BSW_REFBATCH_MAX_TASKS), words.data());
                CHECK(k > 0, "bsw_refbatch_encode -> %d", k);
                /* what the batch says, decoded on the host, through the oracle */
                bsw_params p2;
                std::vector<bsw_task> t2(BSW_REFBATCH_MAX_TASKS);
                std::vector<uint8_t> seqbuf((size_t)BSW_REFBATCH_IN_WORDS * 8 + 64);
                const int k2 = bsw_refbatch_decode(words.data(), &p2, t2.data(), t2.size(), seqbuf.data(), seqbuf.size());
                CHECK(k2 == k, "bsw_refbatch_decode -> %d, encoded %d", k2, k);
                p2.variant = variant; p2.zdrop = 0;
                const std::vector<bsw_result> want = expected(p2, t2.data(), (size_t)k);
                std::vector<uint32_t> ww(BSW_REFBATCH_OUT_WORDS, 0);
                CHECK(bsw_refbatch_encode_results(want.data(), (size_t)k, ww.data()) >= 0, "bsw_refbatch_encode_results");
                ins.push_back(words); wants.push_back(ww); outs.emplace_back(BSW_REFBATCH_OUT_WORDS, 0x5a5a5a5au);
                lo += (size_t)k;
            }
            CHECK(ins.size() >= 3, "only %zu wire batches", ins.size());
            std::vector<uint32_t> one(BSW_REFBATCH_OUT_WORDS, 0x5a5a5a5au);
            int rc = bsw_refbatch_run(ctx, ins[0].data(), one.data(), variant, 0);
            CHECK(rc >= 0, "bsw_refbatch_run -> %d (%s)", rc, bsw_last_error(ctx));
            CHECK(one == wants[0], "bsw_refbatch_run: result batch differs from the oracle's (variant %d)", variant);
            for (size_t b = 0; b < ins.size(); ++b) CHECK(bsw_refbatch_submit(ctx, ins[b].data(), outs[b].data()) == BSW_OK, "bsw_refbatch_submit: %s", bsw_last_error(ctx));
            rc = bsw_refbatch_wait(ctx, variant, 0);
            CHECK(rc == (int)ins.size(), "bsw_refbatch_wait -> %d (%s)", rc, bsw_last_error(ctx));
            for (size_t b = 0; b < ins.size(); ++b) CHECK(outs[b] == wants[b], "bsw_refbatch_wait: result batch %zu differs from the oracle's (variant %d)", b, variant);
            bsw_destroy(ctx);
        }
        CHECK(hipdbl::live_objects() == 0, "wire: %zu HIP objects left alive", hipdbl::live_objects());
    }
    printf("wire: ok\n");
    return 0;
}

/* ---- the drop-in scalar ABI from 8 threads ---- */
static int scalar_mode()
{
    fresh(1);
    workload w;
    make_workload(w, 1600, 150, 123, false, true);
    const bsw_params p = params_of(BSW_VARIANT_H);
    std::vector<std::thread> th;
    std::vector<int> bad(8, 0);
    for (int k = 0; k < 8; ++k)
        th.emplace_back([&, k]() {
            for (size_t i = (size_t)k; i < w.tasks.size(); i += 8) {
                const bsw_task &t = w.tasks[i];
                int g[6], r[6];
                g[0] = ksw_extend2(t.rqlen, t.rquery, t.rtlen, t.rtarget, 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, 100, 5, 100, t.h0, &g[1], &g[2], &g[3], &g[4], &g[5]);
                r[0] = ksw_extend2_ref(t.rqlen, t.rquery, t.rtlen, t.rtarget, 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, 100, 5, 100, t.h0, &r[1], &r[2], &r[3], &r[4], &r[5], BSW_VARIANT_H, nullptr);
                if (memcmp(g, r, sizeof(g)) != 0) ++bad[(size_t)k];
            }
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < 8; ++k) CHECK(bad[(size_t)k] == 0, "ksw_extend2: thread %d got %d calls that differ from the oracle", k, bad[(size_t)k]);
    uint64_t calls = 0, trips = 0;
    bsw_scalar_stats(&calls, &trips);
    CHECK(calls == w.tasks.size() && trips >= 1 && trips <= calls, "bsw_scalar_stats: %llu calls, %llu trips", (unsigned long long)calls, (unsigned long long)trips);
    printf("scalar: %llu calls in %llu trips\n", (unsigned long long)calls, (unsigned long long)trips);
    return 0;
}

/* ---- several devices ---- */
static int devices_mode(const char *sysfs)
{
    struct devcase { int visible, n; int dev[8]; };
    const devcase cases[] = {{2, 2, {0, 1}}, {3, 3, {2, 0, 1}}, {8, 8, {0, 1, 2, 3, 4, 5, 6, 7}}, {2, 3, {1, 0, 1}}};
    for (const devcase &dc : cases) {
        fresh(dc.visible);
        {
            const bsw_params p = params_of(BSW_VARIANT_H);
            const size_t n = 5000;
            workload w;
            make_workload(w, n, 150, 900 + (uint64_t)dc.n, true);
            const std::vector<bsw_result> want = expected(p, w.tasks.data(), n);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, dc.n, 256, 2, 20000, dc.dev);
            if (sysfs) {
                for (int k = 0; k < dc.n; ++k) {
                    char bdf[64];
                    int node = -2, ncpu = -1;
                    CHECK(bsw_device_placement(ctx, k, bdf, sizeof(bdf), &node, &ncpu) == BSW_OK, "bsw_device_placement");
                    char wantbdf[64];
                    snprintf(wantbdf, sizeof(wantbdf), "0000:%02x:00.0", 0xA1 + 0x0B * dc.dev[k]);
                    CHECK(strcmp(bdf, wantbdf) == 0, "device %d: PCI address %s, expected %s", k, bdf, wantbdf);
                    CHECK(node == dc.dev[k] % 2, "device %d: NUMA node %d, the sysfs stand-in says %d", k, node, dc.dev[k] % 2);
                    CHECK(ncpu == 1, "device %d: %d CPUs next to it, the sysfs stand-in lists one CPU", k, ncpu);
                }
            }
            run_submit(ctx, p, w, want, false, true, "devices: bsw_submit");
            run_submit(ctx, p, w, want, true, true, "devices: bsw_submit_packed");
            /* each device computed a disjoint set of seeds, together all of them — twice: two submits */
            std::set<int> distinct(dc.dev, dc.dev + dc.n);
            std::vector<int> seen(n, 0);
            for (int d : distinct) {
                const std::vector<uint32_t> tags = standin::device_tags(d);
                std::set<uint32_t> mine(tags.begin(), tags.end());
                CHECK(!mine.empty(), "device %d computed nothing", d);
                CHECK(tags.size() == 2 * mine.size(), "device %d: %zu records computed for %zu distinct seeds in two submits", d, tags.size(), mine.size());
                for (uint32_t t : mine) { CHECK(t < n, "tag %u", t); ++seen[t]; }
            }
            for (size_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "seed %zu was computed on %d devices", i, seen[i]);
            bsw_destroy(ctx);
        }
        /* the resident reference on every device a chunk fetches from (launch_pack's stand-in checks where the copy lives) */
        {
            const bsw_params p = params_of(BSW_VARIANT_H);
            ref_workload w;
            make_ref_workload(w, p, 3000, 150, 31, true);
            const std::vector<bsw_result> want = expected(p, w.tasks.data(), 3000);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, dc.n, 256, 2, 20000, dc.dev);
            bsw_ref *ref = nullptr;
            CHECK(bsw_ref_upload(ctx, w.pac.data(), w.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
            std::vector<bsw_result> got(3001);
            int rc = bsw_submit_ref(ctx, &p, ref, w.rt.data(), 3000, got.data());
            if (!rc) rc = bsw_wait(ctx);
            CHECK(rc == BSW_OK, "devices: bsw_submit_ref -> %d (%s)", rc, bsw_last_error(ctx));
            same_results(got.data(), want.data(), 3000, "devices: bsw_submit_ref");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
        }
        CHECK(hipdbl::live_objects() == 0, "devices: %zu HIP objects left alive", hipdbl::live_objects());
    }
    printf("devices: ok\n");
    return 0;
}

/* ---- one large resident batch per kernel mode ---- */
static int big_mode(int kernel)
{
    fresh(1);
    uint64_t beyond = 0, max_end = 0;
    const size_t n = 120000;
    {
        const bsw_params p = params_of(BSW_VARIANT_H);
        workload w;
        make_workload(w, n, 250, 4242, false, false, 0.0001);      /* (a sequencer's N rate, 2 - 3 % of the reads: the host's sample then lets the N list pay) */
        const std::vector<bsw_result> want = expected(p, w.tasks.data(), n);
        bsw_ctx *ctx = make_ctx(kernel, 1, 0, 4, 280000);     /* (one worker computes 120 000 seeds with the oracle: no watchdog; LIMIT is the bound) */
        run_resident(ctx, p, w, want, "big resident batch");
        bsw_destroy(ctx);
        beyond = standin::bins_beyond_4n16();
        max_end = standin::max_order_end();
    }
    CHECK(hipdbl::live_objects() == 0, "big: %zu HIP objects left alive", hipdbl::live_objects());
    printf("big: kernel %d, n %zu, N list ends at %llu, 4n+16 = %zu, beyond %llu\n", kernel, n, (unsigned long long)max_end, 4 * n + 16, (unsigned long long)beyond);
    return 0;
}

/* ---- which segment a probe batch lands in under THIS program's class tables ---- */
static int tables_mode()
{
    bsw_params p;
    bsw_default_params(&p);
    std::vector<uint8_t> bases(16384, 1);
    for (int kernel : {BSW_KERNEL_WAVE, BSW_KERNEL_LANE})
        for (int q = 1; q <= 8191; q = q < 300 ? q + 1 : q + 61) {
            bsw_task t;
            memset(&t, 0, sizeof(t));
            t.rquery = bases.data(); t.rtarget = bases.data(); t.rqlen = q; t.rtlen = q + 5; t.h0 = 20; t.init_score = -1;
            std::vector<uint32_t> seg(BSW_PLAN_SEGS + 1);
            CHECK(bsw_plan_batch(&p, &t, 1, kernel, 1, nullptr, seg.data()) >= 0, "bsw_plan_batch");
            int at = -1;
            for (int s = 0; s < BSW_PLAN_SEGS - 1; ++s)
                if (s != 8 && seg[s + 1] > seg[s]) { at = s; break; }
            printf("table %d %d %d\n", kernel, q, at);
        }
    printf("alignclasses %d\n", standin::align_class_count());
    for (int byte = 0; byte < 2; ++byte)
        for (int q = 0; q <= BSW_ALIGN_MAX_QLEN + 1; ++q) printf("alignclass %d %d %d\n", byte, q, standin::align_class_of(q, byte));
    printf("globalclasses %d\n", standin::global_class_count());
    for (int c = 0; c < standin::global_class_count(); ++c) printf("globalclass %d %d\n", c, standin::global_class_cols(c));
    printf("globallongclasses %d\n", standin::global_long_class_count());
    for (int c = 0; c < standin::global_long_class_count(); ++c) printf("globallong %d %d\n", c, standin::global_long_ring(c));
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cross") return cross();
    if (mode == "ref") return ref_mode();
    if (mode == "wire") return wire_mode();
    if (mode == "scalar") return scalar_mode();
    if (mode == "devices") return devices_mode(getenv("BSW_SYSFS_PCI"));
    if (mode == "big" && argc > 2) return big_mode(atoi(argv[2]));
    if (mode == "tables") return tables_mode();
    fprintf(stderr, "usage: host_parity cross|ref|wire|scalar|devices|big K|tables\n");
    return 2;
}
