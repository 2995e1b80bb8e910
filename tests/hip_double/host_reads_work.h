/* host_reads_work.h — a resident read block and the three *_reads_* workloads over it, with the pointer forms' results as
 * expected values.  Shared by host_reads and host_reads_async.  TEST INFRASTRUCTURE. */
#ifndef BSW_HOST_READS_WORK_H
#define BSW_HOST_READS_WORK_H

#include <memory>
#include "host_f4_tickets.h"
#include "launchers_reads.h"

struct block_t {
    std::vector<std::vector<uint8_t>> reads;
    std::vector<const uint8_t *> ptr;
    std::vector<int32_t> len;
    void add(const std::vector<uint8_t> &r) { reads.push_back(r); }
    void seal()
    {
        ptr.clear(); len.clear();
        for (auto &r : reads) { ptr.push_back(r.empty() ? nullptr : r.data()); len.push_back((int32_t)r.size()); }
    }
    bsw_reads *upload(bsw_ctx *ctx)
    {
        seal();
        bsw_reads *rd = nullptr;
        const int rc = bsw_reads_upload(ctx, ptr.data(), len.data(), reads.size(), &rd);
        CHECK(rc == BSW_OK && rd, "bsw_reads_upload -> %d (%s)", rc, bsw_last_error(ctx));
        return rd;
    }
};

/* extension: reads cut out of the genome with substitutions and a few Ns, one seed each; the pointer form points into the block's
 * own host copies.  qbeg / the right flank take every length from 0 up, so both flank starts take every phase. */
struct ework {
    std::vector<bsw_ref_task> t;
    std::vector<bsw_rd_task> rt;
};
inline void make_ext(ework &w, block_t &blk, const genome1_t &g, rng_t &r, size_t n, int read_len)
{
    const size_t first = blk.reads.size();
    for (size_t i = 0; i < n; ++i) {
        const int L = read_len > 0 ? read_len : r.in(20, 260);
        const int64_t x = 40 + r.below((int)(g.l_pac - L - 80));
        blk.add(mutate(r, g.seq(x, x + L), 0.03, 0.0, i % 7 == 0 ? 0.02 : 0.0));
        blk.reads.back().resize((size_t)L, 2);
        const int sl = std::min(19, L);
        bsw_rd_task t;
        memset(&t, 0, sizeof(t));
        t.read = (uint32_t)(first + i);
        t.init_score = -1;
        t.seed.qbeg = (i % 9 == 0) ? 0 : (i % 9 == 1) ? L - sl : r.below(L - sl + 1);
        t.seed.len = sl;
        t.seed.rbeg = x + t.seed.qbeg;
        t.rmax0 = x - 30; t.rmax1 = x + L + 30;
        t.tag = (uint32_t)i;
        w.rt.push_back(t);
    }
    blk.seal();
    for (size_t i = 0; i < n; ++i) {
        const bsw_rd_task &s = w.rt[i];
        bsw_ref_task t;
        memset(&t, 0, sizeof(t));
        t.query = blk.ptr[s.read]; t.l_query = blk.len[s.read]; t.init_score = s.init_score; t.seed = s.seed; t.rmax0 = s.rmax0; t.rmax1 = s.rmax1; t.tag = s.tag;
        w.t.push_back(t);
    }
}

/* the CIGAR workload's slices inside longer reads (qb at every phase), the rescue workload's mates as reads */
inline void to_reads(const cwork &cw, const mwork &mw, rng_t &r, block_t &blk, std::vector<bsw_rd_ctask> &ct, std::vector<bsw_rd_mtask> &mt)
{
    for (size_t i = 0; i < cw.t.size(); ++i) {
        const int front = (int)(i % 17), back = (int)((i * 7) % 5);
        std::vector<uint8_t> rdv;
        for (int k = 0; k < front; ++k) rdv.push_back((uint8_t)r.below(5));
        rdv.insert(rdv.end(), cw.q[i].begin(), cw.q[i].end());
        for (int k = 0; k < back; ++k) rdv.push_back((uint8_t)r.below(5));
        bsw_rd_ctask t;
        memset(&t, 0, sizeof(t));
        t.read = (uint32_t)blk.reads.size();
        t.qb = front; t.qe = front + cw.t[i].l_query; t.w = cw.t[i].w; t.rb = cw.t[i].rb; t.re = cw.t[i].re;
        t.w_cap = cw.t[i].w_cap; t.min_score = cw.t[i].min_score; t.max_tries = cw.t[i].max_tries;
        blk.add(rdv);
        ct.push_back(t);
    }
    for (size_t i = 0; i < mw.t.size(); ++i) {
        bsw_rd_mtask t;
        memset(&t, 0, sizeof(t));
        t.read = (uint32_t)blk.reads.size();
        t.is_rev = mw.t[i].is_rev; t.rb = mw.t[i].rb; t.re = mw.t[i].re; t.xtra = mw.t[i].xtra; t.min_score = mw.t[i].min_score;
        blk.add(mw.m[i]);
        mt.push_back(t);
    }
}

inline int submit_rc(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, const std::vector<bsw_rd_ctask> &t, c_out &o, bsw_ticket *tk)
{
    o.init(t.size());
    return bsw_cigar_reads_submit_t(ctx, &p, ref, rd, t.data(), t.size(), MAXC, o.cig.data(), MAXMD, o.md.data(), o.res.data(), tk);
}
inline int submit_rm(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, const std::vector<bsw_rd_mtask> &t, std::vector<bsw_mresult> &o, bsw_ticket *tk)
{
    m_init(o, t.size());
    return bsw_matesw_reads_submit_t(ctx, &p, ref, rd, t.data(), t.size(), o.data(), tk);
}

struct scenario {
    genome1_t g;
    cwork cw;
    mwork mw;
    ework ew;
    block_t blk;
    std::vector<bsw_rd_ctask> ct;
    std::vector<bsw_rd_mtask> mt;
    std::unique_ptr<arena_t> arc, arm;
    want_t want;                                     /* the pointer forms' synchronous calls */
    std::vector<bsw_result> want_e;                  /* the pointer form's submit */
    void make(size_t n, size_t ne, uint64_t seed, int read_len = 0)
    {
        g.make(150001, seed);
        rng_t r(seed + 5);
        arc.reset(new arena_t(n * 300 + 8192, false));
        arm.reset(new arena_t(n * 400 + 8192, false));
        make_cigar(cw, *arc, g, r, n);
        make_matesw(mw, *arm, g, r, n);
        to_reads(cw, mw, r, blk, ct, mt);
        make_ext(ew, blk, g, r, ne, read_len);
        int longest = 0;
        for (auto &rd : blk.reads) longest = std::max(longest, (int)rd.size());
        standin_reads::set_max_query_len(longest);
    }
    void expect(const bsw_params &p)
    {
        expected_f4(p, g, cw, mw, want);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
        bsw_ref *ref = upload(ctx, g);
        want_e.resize(ew.t.size() + 1);
        CHECK(bsw_submit_ref_t(ctx, &p, ref, ew.t.data(), ew.t.size(), want_e.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "bsw_submit_ref_t: %s", bsw_last_error(ctx));
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
};

#endif
