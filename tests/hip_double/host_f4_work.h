/* host_f4_work.h — the workloads of the global, align, CIGAR and mate-rescue hosts and the calls that run them, shared by
 * host_f4, host_f4_stream, host_reads and host_reads_async: a kind, strand or retry count added here runs in all of them.
 * TEST INFRASTRUCTURE. */
#ifndef BSW_HOST_F4_WORK_H
#define BSW_HOST_F4_WORK_H

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include "host_common.h"
#include "../../bwa-mem-sw_amd/csrc/bsw_f4_host.h"

extern "C" void ksw_align2_ref(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int o_del, int e_del,
                               int o_ins, int e_ins, int xtra, int32_t *out, uint64_t *cells);

/* a genome, one strand of it stored, and its 2-bit pac (bwa's layout: base x in bits ((~x & 3) << 1) of byte x >> 2) */
struct genome1_t {
    int64_t l_pac = 0;
    std::vector<uint8_t> bases, pac;
    void make(int64_t n, uint64_t seed)
    {
        rng_t r(seed);
        l_pac = n;
        bases.resize((size_t)n);
        for (auto &b : bases) b = (uint8_t)r.below(4);
        pac.assign((size_t)((n + 3) >> 2), 0);
        for (int64_t x = 0; x < n; ++x) pac[(size_t)(x >> 2)] |= (uint8_t)(bases[(size_t)x] << ((~x & 3) << 1));
    }
    /* bns_get_seq for an interval that lies on one strand */
    std::vector<uint8_t> seq(int64_t rb, int64_t re) const
    {
        std::vector<uint8_t> out;
        for (int64_t x = rb; x < re; ++x) out.push_back(x >= l_pac ? (uint8_t)(3 - bases[(size_t)(2 * l_pac - 1 - x)]) : bases[(size_t)x]);
        return out;
    }
};

inline std::vector<uint8_t> mutate(rng_t &r, const std::vector<uint8_t> &src, double sub, double indel, double nrate = 0.0)
{
    std::vector<uint8_t> out;
    for (size_t i = 0; i < src.size(); ++i) {
        const double u = r.unit();
        if (u < indel / 2) continue;                                       /* deletion from the read */
        if (u < indel) out.push_back((uint8_t)r.below(4));                 /* insertion */
        uint8_t b = src[i];
        if (r.unit() < sub) b = (uint8_t)((b + 1 + r.below(3)) & 3);
        if (nrate > 0 && r.unit() < nrate) b = 4;
        out.push_back(b);
    }
    if (out.empty()) out.push_back(src.empty() ? 0 : src[0]);
    return out;
}

inline std::vector<uint8_t> revcomp(const std::vector<uint8_t> &s)
{
    std::vector<uint8_t> o(s.rbegin(), s.rend());
    for (auto &c : o) c = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4;
    return o;
}

/* the caller's sequence bytes: one arena, registered (bsw_host_alloc: the hosts' `direct` branch) or pageable (the gather branch) */
struct arena_t {
    uint8_t *p = nullptr;
    size_t cap = 0, at = 0;
    bool registered = false;
    arena_t(size_t bytes, bool reg) : cap(bytes + 64), registered(reg)
    {
        p = (uint8_t *)(reg ? bsw_host_alloc(cap) : malloc(cap));
        CHECK(p, "arena of %zu bytes", cap);
        memset(p, 0, cap);
    }
    ~arena_t() { if (registered) bsw_host_free(p); else free(p); }
    arena_t(const arena_t &) = delete;
    const uint8_t *put(const std::vector<uint8_t> &s)
    {
        CHECK(at + s.size() <= cap, "arena full");
        uint8_t *q = p + at;
        if (!s.empty()) memcpy(q, s.data(), s.size());
        at += s.size();
        return q;
    }
};

inline std::string digits(const uint8_t *s, int n)
{
    std::string o;
    for (int i = 0; i < n; ++i) o += (char)('0' + s[i]);
    return o.empty() ? "-" : o;
}

inline void write_genome(FILE *f, const genome1_t &g, const bsw_params &p)
{
    fprintf(f, "genome %lld ", (long long)g.l_pac);
    for (uint8_t b : g.pac) fprintf(f, "%02x", b);
    fprintf(f, "\nparams");
    for (int i = 0; i < 25; ++i) fprintf(f, " %d", p.mat[i]);
    fprintf(f, " %d %d %d %d\n", p.o_del, p.e_del, p.o_ins, p.e_ins);
}

/* ---- global ---- */
struct gwork {
    std::vector<bsw_gtask> t;
    std::vector<std::vector<uint8_t>> q, tg;
};

static const int G_LONG[] = {63, 64, 127, 128, 255, 256, 400, 511, 512, 700, 1023, 1024, 1100, 1500};

inline void make_global(gwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        int tl = (i % 23 == 5) ? G_LONG[(i / 23) % (sizeof(G_LONG) / sizeof(int))] : r.in(1, 62);
        const int64_t at = r.below((int)(g.l_pac - tl - 1));
        std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl);
        std::vector<uint8_t> q = mutate(r, tg, 0.05, tl > 300 ? 0.01 : 0.04, 0.01);
        if (tl > 62 && (int)q.size() != tl && tl != 400 && tl != 700 && tl != 1100 && tl != 1500) q.resize((size_t)tl, 1);   /* (class edges: the query length decides) */
        w.q.push_back(q);
        w.tg.push_back(tg);
    }
    for (size_t i = 0; i < n; ++i) {
        bsw_gtask t;
        memset(&t, 0, sizeof(t));
        t.qlen = (int)w.q[i].size(); t.tlen = (int)w.tg[i].size();
        t.query = ar.put(w.q[i]); t.target = ar.put(w.tg[i]);
        const int d = abs(t.qlen - t.tlen);
        t.w = d + 3 + (int)(i % 17);
        if (t.tlen == 1100) t.w = 200;                                    /* ring classes 0 (narrow bands), 1 (n_col 401) and 3 (1201) */
        if (t.tlen == 1500) t.w = 600;
        w.t.push_back(t);
    }
}

inline void check_global(bsw_ctx *ctx, const bsw_params &p, const gwork &w, int max_cigar, bool want_cigar, const char *what)
{
    const size_t n = w.t.size();
    std::vector<bsw_gresult> res(n + 1);
    std::vector<uint32_t> cig(n * (size_t)max_cigar + 1, 0xdeadbeefu);
    memset(res.data(), 0x5a, res.size() * sizeof(bsw_gresult));
    const int rc = bsw_global_batch(ctx, &p, w.t.data(), n, max_cigar, res.data(), want_cigar ? cig.data() : nullptr);
    CHECK(rc == BSW_OK, "%s: bsw_global_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    for (size_t i = 0; i < n; ++i) {
        int nc = 0;
        uint32_t *cg = nullptr;
        const int score = ksw_global2_ref(w.t[i].qlen, w.q[i].data(), w.t[i].tlen, w.tg[i].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, w.t[i].w, &nc, &cg, nullptr);
        CHECK(res[i].score == score, "%s: task %zu of %zu (%d x %d, w %d): score %d, the oracle's %d", what, i, n, w.t[i].qlen, w.t[i].tlen, w.t[i].w, res[i].score, score);
        if (want_cigar) {
            CHECK(res[i].n_cigar == (nc <= max_cigar ? nc : -nc), "%s: task %zu of %zu: n_cigar %d, the oracle's %d (room %d)", what, i, n, res[i].n_cigar, nc, max_cigar);
            if (nc <= max_cigar)
                for (int k = 0; k < nc; ++k) CHECK(cig[i * (size_t)max_cigar + (size_t)k] == cg[k], "%s: task %zu of %zu: CIGAR word %d differs", what, i, n, k);
        } else
            CHECK(res[i].n_cigar == 0, "%s: task %zu: n_cigar %d without a CIGAR buffer", what, i, res[i].n_cigar);
        free(cg);
    }
}

/* ---- local alignment ---- */
struct awork {
    std::vector<bsw_atask> t;
    std::vector<std::vector<uint8_t>> q, tg;
};

static const int A_LONG[] = {128, 129, 160, 161, 256, 257, 512, 513, 1024};

inline int xtra_for(size_t i, int qlen)
{
    int x = (i & 1) ? KSW_XBYTE : 0;
    if (i % 5 != 4) x |= KSW_XSUBO | (qlen > 30 ? 19 : 3);
    if (i % 3 != 2) x |= KSW_XSTART;
    if (i % 11 == 10) x = (x & KSW_XBYTE) | KSW_XSTOP | 12;
    return x;
}

inline void make_align(awork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        const int ql = (i % 19 == 3) ? A_LONG[(i / 19) % (sizeof(A_LONG) / sizeof(int))] : r.in(1, 128);
        const int tl = ql + r.in(0, 200);
        const int64_t at = r.below((int)(g.l_pac - tl - 1));
        std::vector<uint8_t> tg(g.bases.begin() + at, g.bases.begin() + at + tl);
        const int off = r.below(tl - ql + 1);
        std::vector<uint8_t> piece(tg.begin() + off, tg.begin() + off + ql);
        std::vector<uint8_t> q = mutate(r, piece, 0.05, 0.02, 0.01);
        q.resize((size_t)ql, 2);
        if (i % 7 == 0 && tl >= 2 * ql + 4) std::copy(piece.begin(), piece.end(), tg.begin() + (tl - ql));       /* a planted repeat: score2 */
        w.q.push_back(q);
        w.tg.push_back(tg);
    }
    for (size_t i = 0; i < n; ++i) {
        bsw_atask t;
        memset(&t, 0, sizeof(t));
        t.qlen = (int)w.q[i].size(); t.tlen = (int)w.tg[i].size();
        t.query = ar.put(w.q[i]); t.target = ar.put(w.tg[i]);
        t.xtra = xtra_for(i, t.qlen);
        w.t.push_back(t);
    }
}

inline void check_align(bsw_ctx *ctx, const bsw_params &p, const awork &w, const char *what)
{
    const size_t n = w.t.size();
    std::vector<bsw_kswr> res(n + 1);
    memset(res.data(), 0x5a, res.size() * sizeof(bsw_kswr));
    const int rc = bsw_align_batch(ctx, &p, w.t.data(), n, res.data());
    CHECK(rc == BSW_OK, "%s: bsw_align_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    for (size_t i = 0; i < n; ++i) {
        int32_t want[7];
        ksw_align2_ref(w.t[i].qlen, w.q[i].data(), w.t[i].tlen, w.tg[i].data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, w.t[i].xtra, want, nullptr);
        CHECK(memcmp(&res[i], want, sizeof(want)) == 0, "%s: task %zu of %zu (%d x %d, xtra 0x%x): score %d te %d qe %d score2 %d te2 %d tb %d qb %d, the oracle's %d %d %d %d %d %d %d",
              what, i, n, w.t[i].qlen, w.t[i].tlen, (unsigned)w.t[i].xtra, res[i].score, res[i].te, res[i].qe, res[i].score2, res[i].te2, res[i].tb, res[i].qb,
              want[0], want[1], want[2], want[3], want[4], want[5], want[6]);
    }
}

/* ---- bwa_gen_cigar2 on the resident reference ---- */
struct cwork {
    std::vector<bsw_ctask> t;
    std::vector<std::vector<uint8_t>> q;
};

/* a read of [rb, re) (in the strand's own order) whose path leaves the diagonal by `off` bases between two indels */
inline std::vector<uint8_t> offset_read(rng_t &r, const std::vector<uint8_t> &rs, int off)
{
    std::vector<uint8_t> o(rs.begin(), rs.begin() + 40);
    o.insert(o.end(), rs.begin() + 40 + off, rs.begin() + 100);            /* a deletion of `off` bases ... */
    for (int k = 0; k < off; ++k) o.push_back((uint8_t)r.below(4));        /* ... and an insertion of as many */
    o.insert(o.end(), rs.begin() + 100, rs.end());
    return o;
}

inline void make_cigar(cwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t n)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < n; ++i) {
        bsw_ctask t;
        memset(&t, 0, sizeof(t));
        t.min_score = INT_MIN; t.max_tries = 1; t.w = 100;
        const int kind = (int)(i % 13);
        const bool rev = (i / 13) % 2 == 1;
        int rl = r.in(60, 150);
        if (kind == 11) rl = (i % 3 == 0) ? 1100 : r.in(200, 600);
        if (kind >= 7 && kind <= 9) rl = 150;
        int64_t rb = (rev ? L : 0) + r.below((int)(L - rl - 1));
        int64_t re = rb + rl;
        std::vector<uint8_t> q;
        if (kind == 2) { rb = L - 30; re = L + 40; q = g.seq(100, 170); }                 /* bridges l_pac: status 1 */
        else if (kind == 3) { re = rb - (i % 2); q = g.seq(100, 170); }                   /* empty interval: status 1 */
        else if (kind == 4) {
            if (i % 2) { rb = 2 * L - 20; re = 2 * L + 30; q = g.seq(100, 150); }         /* leaves [0, 2 l_pac): status 1 */
            else q.clear();                                                              /* an empty read: status 1 */
        } else {
            const std::vector<uint8_t> rs = g.seq(rb, re);                               /* (reverse strand: bwa reverses both) */
            std::vector<uint8_t> fw;
            if (kind == 5 || kind == 6) {                                                /* the no-gap shortcut */
                fw = mutate(r, rs, kind == 6 ? 0.2 : 0.03, 0.0, 0.01);
                fw.resize(rs.size(), 0);
                t.w = 0;
                if (kind == 6) { t.w_cap = 50; t.max_tries = 2 + (int)(i % 2); t.min_score = (i % 4 < 2) ? rl : -1000; }
            } else if (kind >= 7 && kind <= 9) {                                         /* retries: 1, 2 and 3 tries */
                const std::vector<uint8_t> rr = rev ? std::vector<uint8_t>(rs.rbegin(), rs.rend()) : rs;
                std::vector<uint8_t> o = offset_read(r, rr, kind == 7 ? 2 : kind == 8 ? 4 : 8);
                fw = rev ? std::vector<uint8_t>(o.rbegin(), o.rend()) : o;
                t.w = 2; t.w_cap = 64; t.max_tries = 3; t.min_score = 100;
                if (i % 5 == 0) t.max_tries = 2;
            } else
                fw = mutate(r, rs, 0.03, kind == 10 ? 0.06 : 0.01, kind == 1 ? 0.02 : 0.0);
            /* a reverse-strand read arrives in READ order: the reverse of what aligns to bns_get_seq(rb, re) reversed */
            q = fw;
            if ((kind == 0 || kind == 12) && i % 4 == 0) t.w = 5;
        }
        w.q.push_back(q);
        t.l_query = (int)q.size(); t.rb = rb; t.re = re;
        w.t.push_back(t);
    }
    for (size_t i = 0; i < n; ++i) w.t[i].query = w.q[i].empty() ? nullptr : ar.put(w.q[i]);
}

inline void run_cigar(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const cwork &w, int max_cigar, int max_md, bool want_cigar, bool want_md,
                      FILE *f, const char *what, size_t emit_first = SIZE_MAX, std::vector<bsw_cresult> *res_out = nullptr,
                      std::vector<uint32_t> *cig_out = nullptr, std::vector<char> *md_out = nullptr)
{
    const size_t n = w.t.size();
    std::vector<bsw_cresult> res(n + 1);
    std::vector<uint32_t> cig(n * (size_t)max_cigar + 1, 0xdeadbeefu);
    std::vector<char> md(n * (size_t)max_md + 1, '#');
    memset(res.data(), 0x5a, res.size() * sizeof(bsw_cresult));
    const int rc = bsw_cigar_ref_batch(ctx, &p, ref, w.t.data(), n, max_cigar, want_cigar ? cig.data() : nullptr, max_md, want_md ? md.data() : nullptr, res.data());
    CHECK(rc == BSW_OK, "%s: bsw_cigar_ref_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(cig[n * (size_t)max_cigar] == 0xdeadbeefu && md[n * (size_t)max_md] == '#', "%s: a write behind the caller's arrays", what);
    if (f) {
        const size_t m = std::min(n, emit_first);
        fprintf(f, "cigarcase %zu %d %d %d %d %s\n", m, max_cigar, max_md, want_cigar ? 1 : 0, want_md ? 1 : 0, what);
        for (size_t i = 0; i < m; ++i) {
            const bsw_ctask &t = w.t[i];
            const bsw_cresult &r = res[i];
            fprintf(f, "c %s %lld %lld %d %d %d %d | %d %d %d %d %d %d %d %d |", digits(t.query, t.l_query).c_str(), (long long)t.rb, (long long)t.re, t.w, t.w_cap,
                    t.min_score, t.max_tries, r.score, r.n_cigar, r.nm, r.md_len, r.w, r.tries, r.status, r._pad);
            if (want_cigar)
                for (int k = 0; k < r.n_cigar && k < max_cigar; ++k) fprintf(f, " %u", cig[i * (size_t)max_cigar + (size_t)k]);
            fprintf(f, " | ");
            if (want_md) {
                const char *s = md.data() + i * (size_t)max_md;
                CHECK(memchr(s, 0, (size_t)max_md) != nullptr, "%s: task %zu: the MD slot holds no NUL", what, i);
                fprintf(f, "%s", *s ? s : "-");
            } else
                fprintf(f, "?");
            fprintf(f, "\n");
        }
    }
    if (res_out) *res_out = res;
    if (cig_out) *cig_out = cig;
    if (md_out) *md_out = md;
}

/* ---- mate rescue ---- */
struct mwork {
    std::vector<bsw_mtask> t;
    std::vector<std::vector<uint8_t>> m;
};

inline void make_matesw(mwork &w, arena_t &ar, const genome1_t &g, rng_t &r, size_t n)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < n; ++i) {
        bsw_mtask t;
        memset(&t, 0, sizeof(t));
        const int kind = (int)(i % 11);
        const bool strand = (i / 11) % 2 == 1;
        const int lm = (i % 19 == 3) ? A_LONG[(i / 19) % (sizeof(A_LONG) / sizeof(int))] : r.in(8, 150);
        const int tl = lm + r.in(20, 400);
        int64_t rb = (strand ? L : 0) + r.below((int)(L - tl - 1)), re = rb + tl;
        t.is_rev = (int)(i % 2);
        std::vector<uint8_t> win = g.seq(rb, re);
        const int off = r.below(tl - lm + 1);
        std::vector<uint8_t> piece(win.begin() + off, win.begin() + off + lm);
        std::vector<uint8_t> aligned = mutate(r, piece, kind == 9 ? 0.4 : 0.04, 0.02, 0.01);
        aligned.resize((size_t)lm, 1);
        std::vector<uint8_t> ms = t.is_rev ? revcomp(aligned) : aligned;   /* the mate in read order */
        if (kind == 2) { rb = L - 50; re = L + 60; }                       /* bridges l_pac */
        if (kind == 3) re = rb;                                           /* empty window */
        if (kind == 4 && i % 2) { rb = 2 * L - 40; re = 2 * L + 10; }      /* leaves [0, 2 l_pac) */
        if (kind == 4 && !(i % 2)) ms.clear();                             /* empty mate */
        t.xtra = KSW_XSUBO | KSW_XSTART | (i % 3 ? KSW_XBYTE : 0) | (i % 4 == 0 ? 5 : 19);
        if (i % 13 == 7) t.xtra &= ~KSW_XSUBO;
        t.min_score = i % 6 == 0 ? 60 : 19;
        t.l_ms = (int)ms.size(); t.rb = rb; t.re = re;
        w.m.push_back(ms);
        w.t.push_back(t);
    }
    for (size_t i = 0; i < n; ++i) w.t[i].mate = w.m[i].empty() ? nullptr : ar.put(w.m[i]);
}

inline void run_matesw(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const mwork &w, FILE *f, const char *what, size_t emit_first = SIZE_MAX,
                       std::vector<bsw_mresult> *res_out = nullptr)
{
    const size_t n = w.t.size();
    std::vector<bsw_mresult> res(n + 1);
    memset(res.data(), 0x5a, res.size() * sizeof(bsw_mresult));
    const int rc = bsw_matesw_ref_batch(ctx, &p, ref, w.t.data(), n, res.data());
    CHECK(rc == BSW_OK, "%s: bsw_matesw_ref_batch -> %d (%s)", what, rc, bsw_last_error(ctx));
    if (f) {
        const size_t m = std::min(n, emit_first);
        fprintf(f, "matecase %zu %s\n", m, what);
        for (size_t i = 0; i < m; ++i) {
            const bsw_mtask &t = w.t[i];
            const bsw_mresult &r = res[i];
            fprintf(f, "m %s %d %lld %lld %d %d | %d %d %d %d %d %d %d | %d %lld %lld %d %d %d %d %d %d\n", digits(t.mate, t.l_ms).c_str(), t.is_rev, (long long)t.rb,
                    (long long)t.re, t.xtra, t.min_score, r.aln.score, r.aln.te, r.aln.qe, r.aln.score2, r.aln.te2, r.aln.tb, r.aln.qb, r.status, (long long)r.rb,
                    (long long)r.re, r.qb, r.qe, r.score, r.csub, r.seedcov, r._pad);
        }
    }
    if (res_out) *res_out = res;
}

#endif
