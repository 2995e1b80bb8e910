// CPU model of bsw_lane2_rtl_kernel (TEST INFRASTRUCTURE): drives lane2r of the product header bsw_lane2_core.h — the
// variant-RTL row the GPU kernel is compiled from — with the wave-level glue restated in plain loops, as
// tests/lane2_model.cpp does for variants H and M.  That file is included whole, so the same shared object also runs the
// unchanged H / M path (lane2_model_run_qb) next to the RTL one: tests/test_lane2_rtl_model.py checks both.
// g++ -O2 -std=c++17 -shared -fPIC -I include -o lane2_rtl_model.so tests/lane2_rtl_model.cpp
#include "lane2_model.cpp"

// what the workload exercised, summed over the runs since the last reset (lane2_rtl_model_stats):
//   [0] rows on which the two seeds of a lane were both active with DIFFERENT beg inside the same 8-column block
//   [1] the same for end
//   [2] lanes whose two seeds both ran and stopped at least 32 rows apart
static uint64_t g_stats[3];

template <int QB, bool SYM>
struct rtl_wave_model {
    using L = lane2r<QB, SYM>;
    struct lane_t {
        typename L::state S;
        uint32_t qp[2][3][L::NW];       // query bit planes
        uint32_t wn[L::NC];             // N planes, interleaved per 16 columns
        const uint8_t *t[2];
        bool valid[2];
        uint32_t ti[2];
    };

    static void run(const bsw_params *p, const bsw_task *tasks, int side, const uint32_t *order, size_t n, size_t w0,
                    const int32_t *h0s, bsw_ext *out)
    {
        consts k;
        k.a = p->mat[0]; k.pb = -p->mat[1]; k.pn = -p->mat[24];
        k.o_del = p->o_del; k.e_del = p->e_del; k.oe_ins = p->o_ins + p->e_ins; k.e_ins = p->e_ins; k.zdrop = p->zdrop;
        fill_packed_consts(k);
        int mx = 0;
        for (int i = 0; i < 25; ++i) mx = mx > p->mat[i] ? mx : p->mat[i];
        std::vector<lane_t> ln(64);
        unir u;
        u.nblk = 0; u.anybite = false; u.zl = u.zh = 0;
        for (int l = 0; l < 64; ++l) {
            lane_t &a = ln[l];
            memset(a.qp, 0, sizeof(a.qp));
            for (int x = 0; x < 2; ++x) {
                const size_t slot = w0 + (size_t)l + 64 * (size_t)x;
                a.valid[x] = slot < n;
                a.ti[x] = a.valid[x] ? order[slot] : order[0];
                const bsw_task &T = tasks[a.ti[x]];
                int qlen = side ? T.rqlen : T.lqlen, tlen = side ? T.rtlen : T.ltlen;
                const uint8_t *q = side ? T.rquery : T.lquery;
                a.t[x] = side ? T.rtarget : T.ltarget;
                const int eb = side ? p->pen_clip3 : p->pen_clip5;
                int wl = side ? T.wlim_r : T.wlim_l;
                if (wl <= 0) {
                    int mi = (qlen * mx + eb - p->o_ins + p->e_ins) / p->e_ins, md = (qlen * mx + eb - p->o_del + p->e_del) / p->e_del;
                    if (mi < 1) mi = 1;
                    if (md < 1) md = 1;
                    wl = mi < md ? mi : md;
                }
                if (!a.valid[x]) tlen = 0;
                init_pair(a.S.p, x, qlen, tlen, h0s ? h0s[a.ti[x]] : T.h0, p->w < wl ? p->w : wl);
                for (int j = 0; j < qlen; ++j) {
                    const int c = q[j] > 4 ? 4 : q[j];
                    if (c & 1) a.qp[x][0][j >> 5] |= 1u << (j & 31);
                    if (c & 2) a.qp[x][1][j >> 5] |= 1u << (j & 31);
                    if (c & 4) { a.qp[x][2][j >> 5] |= 1u << (j & 31); if (a.valid[x]) u.nblk |= 1u << (j >> 3); }
                }
            }
            for (int c = 0; c < L::NC; ++c) {
                const uint32_t wa = (a.qp[0][2][c >> 1] >> (16 * (c & 1))) & 0xffffu, wb = (a.qp[1][2][c >> 1] >> (16 * (c & 1))) & 0xffffu;
                a.wn[c] = wa | (wb << 16);
            }
            L::init_row(a.S, k);
        }
        std::vector<rowp> rv(64);
        int last[64][2];
        for (int l = 0; l < 64; ++l) last[l][0] = last[l][1] = -1;
        for (int i = 0;; ++i) {
            bool any = false;
            u.jlo = 1 << 20; u.jhi = -1; u.jem = 1 << 20; u.jbm = 0;
            for (int l = 0; l < 64; ++l) {
                pairv &pv = ln[l].S.p;
                row_begin2(pv, i, rv[l]);
                for (int x = 0; x < 2; ++x) {
                    if (!half_of(rv[l].ACT, x)) continue;
                    any = true;
                    const int beg = half_of(pv.BEG, x), end = half_of(pv.END, x);
                    if (beg < u.jlo) u.jlo = beg;
                    if (beg > u.jbm) u.jbm = beg;
                    if (end > u.jhi) u.jhi = end;
                    if (end < u.jem) u.jem = end;
                }
            }
            if (!any) break;
            for (int l = 0; l < 64; ++l) {
                const pairv &pv = ln[l].S.p;
                if (half_of(rv[l].ACT, 0)) last[l][0] = i;
                if (half_of(rv[l].ACT, 1)) last[l][1] = i;
                if (!half_of(rv[l].ACT, 0) || !half_of(rv[l].ACT, 1)) continue;
                const int b0 = half_of(pv.BEG, 0), b1 = half_of(pv.BEG, 1), e0 = half_of(pv.END, 0), e1 = half_of(pv.END, 1);
                if (b0 != b1 && (b0 >> 3) == (b1 >> 3)) ++g_stats[0];
                if (e0 != e1 && (e0 >> 3) == (e1 >> 3)) ++g_stats[1];
            }
            for (int l = 0; l < 64; ++l) {
                lane_t &a = ln[l];
                int tb[2];
                for (int x = 0; x < 2; ++x) {
                    int b = half_of(rv[l].ACT, x) ? a.t[x][i] : 0;
                    tb[x] = b > 4 ? 4 : b;
                }
                auto qp = [&](int x, int b, uint32_t (&rm)[L::NW]) {
                    for (int wd = 0; wd < L::NW; ++wd) rm[wd] = L::base_match(a.qp[x][0][wd], a.qp[x][1][wd], a.qp[x][2][wd], b);
                };
                auto wn = [&](int c) { return a.wn[c]; };
                auto kp = [&](int b, uint32_t (&kw)[L::NW]) {
                    for (int wd = 0; wd < L::NW; ++wd) kw[wd] = L::keep_word(b, wd);
                };
                L::row_body(a.S, k, i, rv[l], u, tb, qp, kp, wn);
            }
        }
        for (int l = 0; l < 64; ++l)
            if (last[l][0] >= 0 && last[l][1] >= 0 && abs(last[l][0] - last[l][1]) >= 32) ++g_stats[2];
        for (int l = 0; l < 64; ++l)
            for (int x = 0; x < 2; ++x) {
                if (!ln[l].valid[x]) continue;
                const ext_out s = pair_result(ln[l].S.p, x);
                bsw_ext &e = out[ln[l].ti[x]];
                e.score = s.mx; e.qle = s.max_j + 1; e.tle = s.max_i + 1; e.gtle = s.max_ie + 1;
                e.gscore = s.gscore; e.max_off = s.max_off; e.aw = p->w; e.cells = s.cells;
            }
    }
};

// One band try of one side of tasks[order[0..n)] as bsw_lane2_rtl_kernel<QB> runs it: 128 seeds per wave, qb = 9 (72 columns)
// or 17 (136 columns); shared or separate gap penalties by the parameters.  The variant field of p is not read.
extern "C" int lane2_rtl_model_run(const bsw_params *p, const bsw_task *tasks, int side, const uint32_t *order, size_t n,
                                   const int32_t *h0s, bsw_ext *out, int qb)
{
    if (!p || !tasks || !order || !out) return -1;
    if (p->mat[1] > 0 || p->mat[24] > 0 || -p->mat[1] < -p->mat[24]) return -2;      /* the packed range */
    if (p->o_del + p->e_del > 255 || p->o_ins + p->e_ins > 255 || p->mat[0] - p->mat[1] > 255) return -2;
    const bool sym = p->o_del == p->o_ins && p->e_del == p->e_ins;
    for (size_t w0 = 0; w0 < n; w0 += 128) {
        if (qb == 17) { if (sym) rtl_wave_model<17, true>::run(p, tasks, side, order, n, w0, h0s, out); else rtl_wave_model<17, false>::run(p, tasks, side, order, n, w0, h0s, out); }
        else if (qb == 9) { if (sym) rtl_wave_model<9, true>::run(p, tasks, side, order, n, w0, h0s, out); else rtl_wave_model<9, false>::run(p, tasks, side, order, n, w0, h0s, out); }
        else return -3;
    }
    return 0;
}

extern "C" void lane2_rtl_model_stats(uint64_t *out3, int reset)
{
    for (int q = 0; q < 3; ++q) { out3[q] = g_stats[q]; if (reset) g_stats[q] = 0; }
}
