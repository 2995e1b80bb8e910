/* host_ref_patch.h — what the host-double programs of the stages around mem_patch_reg share (host_patch, host_sdp,
 * host_chain2aln): the genome with both strands in bwa's coordinates, and mem_patch_reg restated in C.  TEST INFRASTRUCTURE. */
#ifndef BSW_HOST_REF_PATCH_H
#define BSW_HOST_REF_PATCH_H

#include <algorithm>
#include <cmath>
#include "host_common.h"

/* a genome, its 2-bit pac (bwa's layout) and both strands in bwa's coordinates */
struct genome_t {
    int64_t l_pac = 0;
    std::vector<uint8_t> both, pac;
    void make(int64_t n, uint64_t seed)
    {
        rng_t r(seed);
        l_pac = n;
        both.resize((size_t)(2 * n));
        for (int64_t x = 0; x < n; ++x) both[(size_t)x] = (uint8_t)r.below(4);
        for (int64_t x = n; x < 2 * n; ++x) both[(size_t)x] = (uint8_t)(3 - both[(size_t)(2 * n - 1 - x)]);
        pac.assign((size_t)((n + 3) >> 2), 0);
        for (int64_t x = 0; x < n; ++x) pac[(size_t)(x >> 2)] |= (uint8_t)(both[(size_t)x] << ((~x & 3) << 1));
    }
};

/* ---- mem_patch_reg restated in C from its text (bwamem.c, bwa >= 0.7.10, as recalled) ---- */
inline int ref_band(const bsw_params &p, int l_query, int rlen, int w_)
{
    const int max_ins = (int)((double)(((l_query + 1) >> 1) * p.mat[0] - p.o_ins) / p.e_ins + 1.);
    const int max_del = (int)((double)(((l_query + 1) >> 1) * p.mat[0] - p.o_del) / p.e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    int w = (max_gap + abs(rlen - l_query) + 1) >> 1;
    w = w < w_ ? w : w_;
    const int min_w = abs(rlen - l_query) + 3;
    return w > min_w ? w : min_w;
}

inline bsw_presult ref_patch(const bsw_params &p, const genome_t &g, const uint8_t *query, const bsw_preg &a, const bsw_preg &b, bool *shortcut = nullptr)
{
    const bsw_presult none = {0, 0, 0, 1};
    const int64_t l_pac = g.l_pac;
    if (shortcut) *shortcut = false;
    if (a.rb < l_pac && b.rb >= l_pac) return none;
    if (a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re) return none;
    int w = (int)((a.re - b.rb) - (a.qe - b.qb));
    w = w > 0 ? w : -w;
    double r = (double)(a.re - b.rb) / (b.re - a.rb) - (double)(a.qe - b.qb) / (b.qe - a.qb);
    r = r > 0. ? r : -r;
    if (a.re < b.rb || a.qe < b.qb) { if (w > p.w << 1 || r >= 0.05f) return none; }
    else { if (w > p.w << 2 || r >= 0.05f * 2) return none; }
    w += a.w + b.w;
    w = w < p.w << 2 ? w : p.w << 2;
    /* bwa_gen_cigar2, the score only */
    const int64_t rb = a.rb, re = b.re;
    const int lq = b.qe - a.qb;
    if (lq <= 0 || rb >= re || (rb < l_pac && re > l_pac) || rb < 0 || re > 2 * l_pac) return none;
    std::vector<uint8_t> q(query + a.qb, query + b.qe), t(g.both.begin() + rb, g.both.begin() + re);
    if (rb >= l_pac) { std::reverse(q.begin(), q.end()); std::reverse(t.begin(), t.end()); }
    int score = 0;
    if (lq == (int)(re - rb) && w == 0) {
        for (int i = 0; i < lq; ++i) score += p.mat[std::min<int>(t[(size_t)i], 4) * 5 + std::min<int>(q[(size_t)i], 4)];
        if (shortcut) *shortcut = true;
    } else {
        uint64_t cells = 0;
        score = ksw_global2_ref(lq, q.data(), (int)(re - rb), t.data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, ref_band(p, lq, (int)(re - rb), w), nullptr, nullptr, &cells);
    }
    const int q_s = (int)((double)(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * (b.score + a.score) + .499);
    const int r_s = (int)((double)(b.re - a.rb) / ((b.re - b.rb) + (a.re - a.rb)) * (b.score + a.score) + .499);
    const int ret = (double)score / (q_s > r_s ? q_s : r_s) < 0.90f ? 0 : score;
    return bsw_presult{ret, w, score, ret > 0 ? 0 : 2};
}

#endif
