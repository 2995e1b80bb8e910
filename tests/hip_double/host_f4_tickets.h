/* host_f4_tickets.h — the ticket forms of host_f4_work.h's CIGAR and mate-rescue workloads: result holders, submits, the
 * synchronous calls as expected values.  Shared by host_f4_stream, host_reads and host_reads_async.  TEST INFRASTRUCTURE. */
#ifndef BSW_HOST_F4_TICKETS_H
#define BSW_HOST_F4_TICKETS_H

#include "host_f4_work.h"

static const int MAXC = 64, MAXMD = 512;

struct c_out {
    std::vector<bsw_cresult> res;
    std::vector<uint32_t> cig;
    std::vector<char> md;
    void init(size_t n)
    {
        res.resize(n + 1); cig.assign(n * MAXC + 1, 0xdeadbeefu); md.assign(n * MAXMD + 1, '#');
        memset(res.data(), 0x5a, res.size() * sizeof(bsw_cresult));
    }
};

/* every byte of the result records (the _pad fields included), the CIGAR words a result announces, the MD strings */
inline bool same_c(const c_out &a, const c_out &b, size_t n, std::string *why = nullptr)
{
    char buf[160];
    for (size_t i = 0; i < n; ++i) {
        if (memcmp(&a.res[i], &b.res[i], sizeof(bsw_cresult)) != 0) {
            snprintf(buf, sizeof(buf), "record %zu of %zu (score %d / %d, tries %d / %d, status %d / %d)", i, n, a.res[i].score, b.res[i].score, a.res[i].tries, b.res[i].tries,
                     a.res[i].status, b.res[i].status);
            if (why) *why = buf;
            return false;
        }
        const int nc = std::min(std::max(a.res[i].n_cigar, 0), MAXC);
        if (nc && memcmp(&a.cig[i * MAXC], &b.cig[i * MAXC], (size_t)nc * 4) != 0) { if (why) *why = "CIGAR of record " + std::to_string(i); return false; }
        if (a.res[i].status == 0 && strcmp(&a.md[i * MAXMD], &b.md[i * MAXMD]) != 0) { if (why) *why = "MD of record " + std::to_string(i); return false; }
    }
    return a.cig[n * MAXC] == 0xdeadbeefu && a.md[n * MAXMD] == '#' && b.cig[n * MAXC] == 0xdeadbeefu && b.md[n * MAXMD] == '#';
}

inline bool same_m(const std::vector<bsw_mresult> &a, const std::vector<bsw_mresult> &b, size_t n)
{
    return n == 0 || memcmp(a.data(), b.data(), n * sizeof(bsw_mresult)) == 0;
}

inline void m_init(std::vector<bsw_mresult> &r, size_t n)
{
    r.resize(n + 1);
    memset(r.data(), 0x5a, r.size() * sizeof(bsw_mresult));
}

inline int submit_c(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const cwork &w, c_out &o, bsw_ticket *t)
{
    o.init(w.t.size());
    return bsw_cigar_ref_submit_t(ctx, &p, ref, w.t.data(), w.t.size(), MAXC, o.cig.data(), MAXMD, o.md.data(), o.res.data(), t);
}

inline int submit_m(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const mwork &w, std::vector<bsw_mresult> &o, bsw_ticket *t)
{
    m_init(o, w.t.size());
    return bsw_matesw_ref_submit_t(ctx, &p, ref, w.t.data(), w.t.size(), o.data(), t);
}

inline void sync_c(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const cwork &w, c_out &o)
{
    o.init(w.t.size());
    const int rc = bsw_cigar_ref_batch(ctx, &p, ref, w.t.data(), w.t.size(), MAXC, o.cig.data(), MAXMD, o.md.data(), o.res.data());
    CHECK(rc == BSW_OK, "bsw_cigar_ref_batch -> %d (%s)", rc, bsw_last_error(ctx));
}

inline void sync_m(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const mwork &w, std::vector<bsw_mresult> &o)
{
    m_init(o, w.t.size());
    const int rc = bsw_matesw_ref_batch(ctx, &p, ref, w.t.data(), w.t.size(), o.data());
    CHECK(rc == BSW_OK, "bsw_matesw_ref_batch -> %d (%s)", rc, bsw_last_error(ctx));
}

/* the expected values of one workload pair: the synchronous calls on a one-device context */
struct want_t {
    c_out c;
    std::vector<bsw_mresult> m;
};
inline void expected_f4(const bsw_params &p, const genome1_t &g, const cwork &cw, const mwork &mw, want_t &want)
{
    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
    bsw_ref *ref = upload(ctx, g);
    sync_c(ctx, p, ref, cw, want.c);
    sync_m(ctx, p, ref, mw, want.m);
    bsw_ref_free(ctx, ref);
    bsw_destroy(ctx);
}

#endif
