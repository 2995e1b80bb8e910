/* launchers.cpp — the bsw::launch_* / *_class_* interface of bsw_stage.h on the CPU (TEST INFRASTRUCTURE: an object file of the
 * sanitizer test programs, next to hip_double.cpp; never part of the library).
 *
 * A stand-in queues its work on the double's stream, so it runs in stream order on that stream's worker thread, and it reads and
 * writes only what the host staged in "device" memory: the task records, the packed words, the order lists.
 *   staging   launch_rebase, launch_pack (host bytes, rev_left, the resident reference with reverse complement), launch_wire_pack,
 *             launch_wire_results: restatements of the device halves in bsw_stage_kernel.hip from the record layouts.
 *   binning   launch_bin calls plan_fill_order(), the host's own replay of the device's rules (bsw_batch.hip): one function.
 *   DP        launch_wave / launch_lane walk exactly the list slice and count they are given, unpack the seed's sequences from
 *             the packed words and compute the whole record with the oracle (oracle/ksw_extend_ref.c; tests/ksw_extend_rtl_ref.c
 *             for BSW_VARIANT_RTL).  A seed's complete record is written whenever a launch lists it and the redo count stays 0:
 *             the kernels' redo protocol is not mimicked.  What the lists must get right is kept in a LEDGER per chunk (which
 *             seed, which side, how often) and checked when the chunk's results are copied out: every side listed exactly once,
 *             no index >= n, no slice behind bsw_plan_order_capacity(n).
 *   F4        launch_global / launch_global_long (oracle/ksw_global_ref.c), launch_align (oracle/ksw_align_ref.c; the query
 *             reverse-complemented first under BSW_AD_QRC) and launch_cigar_md (a plain restatement of the contract in the head
 *             comment of bsw_cigar_kernel.hip) serve bsw_global_batch, bsw_align_batch, bsw_cigar_ref_batch and
 *             bsw_matesw_ref_batch.  They walk exactly order[0..n), read the task records and packed words the host staged, and
 *             keep a ledger per result array and launch round (a round ends when the results are copied out): no index >= the
 *             task count of the chunk's pack launch, no task listed twice, every task inside its launch's class, the slices
 *             [z_off, +n_col * tlen) / [b_off, +tlen) of a round disjoint.  The first and the last byte / entry of every
 *             slice are written, so ASan is the witness that it lies inside the host's reservation.
 * The class tables below restate the kernels' (bsw_wave_kernel.hip kWaveClasses, bsw_lane_kernel.hip kLaneClassesAll, ...);
 * tests/test_host_double_cpu.py compares the plans they lead to with the built library's.
 */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"
#include "../../oracle/ksw_extend_ref.h"
#include "hip_double.h"
#include "launchers.h"

#include <algorithm>
#include <map>
#include <string>

extern "C" void rtl_ref_pair_batch(const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out);
extern "C" void ksw_align2_ref(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat, int o_del, int e_del,
                               int o_ins, int e_ins, int xtra, int32_t *out, uint64_t *cells);

namespace {

struct ledger_t {
    uint32_t n = 0;
    const uint32_t *order = nullptr;
    bsw_binparams bp{};
    std::vector<uint8_t> L, R, W;                   /* times the left / right side / the whole seed was listed by a launch */
};
struct book_t {
    std::mutex mu;
    std::map<const void *, std::shared_ptr<ledger_t>> by_tasks;
    std::map<const void *, const void *> owner;      /* result array (bsw_result or bsw_pair) -> the chunk's task records */
    std::map<int, std::vector<uint32_t>> tags;
    uint64_t checked = 0, beyond = 0, max_end = 0, waits = 0;
    /* the global / align / CIGAR hosts: one launch round per result array, the task count of the last pack launch per seq[] */
    struct round_t { const void *seq = nullptr; std::vector<uint8_t> seen; std::vector<std::pair<uint64_t, uint64_t>> slices; };
    std::map<const void *, round_t> f4;
    std::map<const void *, uint32_t> pack_n;
    uint64_t f4_rounds = 0, f4_tasks = 0;
};
book_t &B()
{
    static book_t *b = new book_t();
    return *b;
}

std::shared_ptr<ledger_t> ledger_of(const void *tasks)
{
    std::lock_guard<std::mutex> lk(B().mu);
    auto it = B().by_tasks.find(tasks);
    return it == B().by_tasks.end() ? nullptr : it->second;
}

/* the chunk's results leave the device: every side must have been listed exactly once */
void f4_round_ends(const void *src)
{
    book_t::round_t r;
    {
        std::lock_guard<std::mutex> lk(B().mu);
        auto it = B().f4.find(src);
        if (it == B().f4.end()) return;
        r = std::move(it->second);
        B().f4.erase(it);
        ++B().f4_rounds;
    }
    std::sort(r.slices.begin(), r.slices.end());
    for (size_t k = 1; k < r.slices.size(); ++k)
        if (r.slices[k].first < r.slices[k - 1].first + r.slices[k - 1].second)
            hipdbl::die("stand-in ledger: the scratch slices [%llu, +%llu) and [%llu, +%llu) of one launch round overlap", (unsigned long long)r.slices[k - 1].first,
                        (unsigned long long)r.slices[k - 1].second, (unsigned long long)r.slices[k].first, (unsigned long long)r.slices[k].second);
}

/* a launch of the global / align stand-ins lists task idx, with the scratch slice [off, +len) (len 0: none) */
void f4_note(const void *out, const void *seq, uint32_t idx, uint64_t off, uint64_t len, const char *who)
{
    std::lock_guard<std::mutex> lk(B().mu);
    auto pn = B().pack_n.find(seq);
    if (pn == B().pack_n.end()) hipdbl::die("stand-in %s: no pack launch has filled the seq[] it reads", who);
    if (idx >= pn->second) hipdbl::die("stand-in %s: list entry %u >= the chunk's %u tasks", who, idx, pn->second);
    book_t::round_t &r = B().f4[out];
    r.seq = seq;
    if (r.seen.size() < pn->second) r.seen.resize(pn->second, 0);
    if (r.seen[idx]++) hipdbl::die("stand-in %s: task %u is listed twice in one launch round", who, idx);
    if (len) r.slices.emplace_back(off, len);
    ++B().f4_tasks;
}

void on_d2h(const void *src, size_t)
{
    f4_round_ends(src);
    std::shared_ptr<ledger_t> lg;
    const bsw_dtask *tasks = nullptr;
    {
        std::lock_guard<std::mutex> lk(B().mu);
        auto o = B().owner.find(src);
        if (o == B().owner.end()) return;
        auto it = B().by_tasks.find(o->second);
        if (it == B().by_tasks.end()) return;
        lg = it->second;
        tasks = (const bsw_dtask *)o->second;
        ++B().checked;
    }
    for (uint32_t i = 0; i < lg->n; ++i) {
        const bsw_dtask &T = tasks[i];
        const int l = lg->L[i] + lg->W[i], r = lg->R[i] + lg->W[i];
        if (T.lqlen && l != 1) hipdbl::die("stand-in ledger: seed %u of %u: left side listed %d times (lane %d, whole %d)", i, lg->n, l, lg->L[i], lg->W[i]);
        if (T.rqlen && r != 1) hipdbl::die("stand-in ledger: seed %u of %u: right side listed %d times (lane %d, whole %d)", i, lg->n, r, lg->R[i], lg->W[i]);
        if (!T.lqlen && !T.rqlen && lg->W[i] != 1) hipdbl::die("stand-in ledger: seed %u of %u has no side and was listed %d times by the general kernels", i, lg->n, lg->W[i]);
        if (lg->L[i] > 1 || lg->R[i] > 1) hipdbl::die("stand-in ledger: seed %u of %u listed twice by lane launches", i, lg->n);
    }
    std::fill(lg->L.begin(), lg->L.end(), 0);        /* (a resident batch may run again) */
    std::fill(lg->R.begin(), lg->R.end(), 0);
    std::fill(lg->W.begin(), lg->W.end(), 0);
}

struct hook_installer { hook_installer() { hipdbl::set_d2h_hook(on_d2h); } } g_hook;

void unpack(const uint64_t *seq, uint32_t off, int len, std::vector<uint8_t> &dst)
{
    dst.resize((size_t)len);
    for (int k = 0; k < len; ++k) dst[(size_t)k] = (uint8_t)((seq[off + (uint32_t)(k >> 4)] >> (4 * (k & 15))) & 0xf);
}

bool words_have_n(const uint64_t *seq, uint32_t off, int len)
{
    for (int k = 0; k < len; ++k)
        if (((seq[off + (uint32_t)(k >> 4)] >> (4 * (k & 15))) & 0xf) >= 4) return true;
    return false;
}

/* one seed's record from what lies in device memory */
void compute(const bsw_dparams &P, int variant, const uint64_t *seq, const bsw_dtask &T, bsw_result *r)
{
    bsw_params p;
    memset(&p, 0, sizeof(p));
    memcpy(p.mat, P.mat, 25);
    p.o_del = P.o_del; p.e_del = P.e_del; p.o_ins = P.o_ins; p.e_ins = P.e_ins;
    p.w = P.w; p.pen_clip5 = P.pen_clip5; p.pen_clip3 = P.pen_clip3; p.zdrop = P.zdrop; p.max_band_try = P.max_band_try; p.variant = variant;
    std::vector<uint8_t> lq, lt, rq, rt;
    bsw_task t;
    memset(&t, 0, sizeof(t));
    if (T.lqlen) { unpack(seq, T.lq_off, T.lqlen, lq); unpack(seq, T.lt_off, T.ltlen, lt); t.lquery = lq.data(); t.ltarget = lt.data(); t.lqlen = T.lqlen; t.ltlen = T.ltlen; }
    if (T.rqlen) { unpack(seq, T.rq_off, T.rqlen, rq); unpack(seq, T.rt_off, T.rtlen, rt); t.rquery = rq.data(); t.rtarget = rt.data(); t.rqlen = T.rqlen; t.rtlen = T.rtlen; }
    t.h0 = T.h0; t.init_score = T.init_score; t.qbeg = T.qbeg; t.tag = T.tag; t.wlim_l = T.wlim_l; t.wlim_r = T.wlim_r;
    if (variant == BSW_VARIANT_RTL) rtl_ref_pair_batch(&p, &t, 1, r);
    else bsw_pair_ref(&p, &t, r);
}

void as_pair(const bsw_result &r, bsw_pair *pr) { memcpy(pr, &r, sizeof(bsw_pair)); }     /* (the record's first 32 bytes) */

/* a launch's list slice against the chunk's ledger; lg may be NULL (the small-batch path bins on the host) */
void check_slice(const ledger_t *lg, const uint32_t *order, uint32_t n, const char *who)
{
    if (!lg) return;
    const size_t cap = bsw_plan_order_capacity(lg->n);
    if (order < lg->order || (size_t)(order - lg->order) + n > cap)
        hipdbl::die("stand-in %s: list slice [%td, +%u) leaves the %zu words of order[] (n = %u)", who, order - lg->order, n, cap, lg->n);
}

void note_seed(const ledger_t *lg, uint32_t ti, const char *who)
{
    if (lg && ti >= lg->n) hipdbl::die("stand-in %s: list entry %u >= n = %u", who, ti, lg->n);
}

void remember(const void *res, const void *tasks, int dev, const std::vector<uint32_t> &tags)
{
    std::lock_guard<std::mutex> lk(B().mu);
    if (res) B().owner[res] = tasks;
    std::vector<uint32_t> &v = B().tags[dev];
    v.insert(v.end(), tags.begin(), tags.end());
}

int base_of_pac(const uint8_t *pac, int64_t l_pac, int64_t x)
{
    if (x >= l_pac) { const int64_t y = (l_pac << 1) - 1 - x; return 3 - ((pac[y >> 2] >> ((~y & 3) << 1)) & 3); }
    return (pac[x >> 2] >> ((~x & 3) << 1)) & 3;
}

}  // namespace

namespace standin {
void reset()
{
    std::lock_guard<std::mutex> lk(B().mu);
    B().by_tasks.clear(); B().owner.clear(); B().tags.clear(); B().f4.clear(); B().pack_n.clear();
    B().checked = B().beyond = B().max_end = B().waits = B().f4_rounds = B().f4_tasks = 0;
}
uint64_t f4_rounds() { std::lock_guard<std::mutex> lk(B().mu); return B().f4_rounds; }
uint64_t f4_tasks() { std::lock_guard<std::mutex> lk(B().mu); return B().f4_tasks; }
std::vector<uint32_t> device_tags(int dev) { std::lock_guard<std::mutex> lk(B().mu); return B().tags[dev]; }
uint64_t chunks_checked() { std::lock_guard<std::mutex> lk(B().mu); return B().checked; }
uint64_t bins_beyond_4n16() { std::lock_guard<std::mutex> lk(B().mu); return B().beyond; }
uint64_t max_order_end() { std::lock_guard<std::mutex> lk(B().mu); return B().max_end; }
uint64_t chain_waits() { std::lock_guard<std::mutex> lk(B().mu); return B().waits; }
}  // namespace standin

static int long_ring(int cls) { return 256 << cls; }
namespace standin {
int align_class_count() { return bsw::align_class_count(); }
int align_class_of(int qlen, int byte_mode) { return bsw::align_class_of(qlen, byte_mode); }
int global_class_count() { return bsw::global_class_count(); }
int global_class_cols(int cls) { return bsw::global_class_cols(cls); }
int global_long_class_count() { return bsw::GLOBAL_LONG_CLASSES; }
int global_long_ring(int cls) { return long_ring(cls); }
}  // namespace standin

#define STANDIN_GATE(name)                                  \
    do {                                                    \
        const hipError_t g_ = hipdbl::gate(name);           \
        if (g_ != hipSuccess) return g_;                    \
    } while (0)

namespace bsw {

/* ---- class tables (see the file header) ---- */
static const int kWave[] = {1, 2, 3, 4, 8, 16, 32, 128};
int wave_class_count() { return 8; }
int wave_class_cols(int c) { return kWave[c] * 64; }
static const int kLaneBits[] = {8, 8, 8, 16}, kLaneCols[] = {72, 136, 232, 136};
int lane_class_count() { return 4; }
int lane_class_cols(int c) { return kLaneCols[c]; }
int lane_class_bits(int c) { return kLaneBits[c]; }
bool lane_class_signals_tail(int c) { return c >= 0 && kLaneBits[c] == 8; }
bool lane_class_finishes(int c, const bsw_dparams &P, int variant)
{
    if (kLaneBits[c] != 8 || (variant != BSW_VARIANT_H && variant != BSW_VARIANT_M)) return false;
    const int a = P.mat[0], pb = -P.mat[1], pn = -P.mat[24];
    return a > 0 && pb >= 0 && pn >= 0 && pb >= pn && a + pb < 256 && P.o_del + P.e_del < 256 && P.o_ins + P.e_ins < 256;
}
static const struct { int byte, slen; } kAlign[] = {{1, 8}, {1, 10}, {1, 16}, {1, 32}, {1, 64}, {0, 16}, {0, 20}, {0, 32}, {0, 64}, {0, 128}};
int align_class_count() { return 10; }
int align_class_of(int qlen, int byte_mode)
{
    for (int c = 0; c < 10; ++c)
        if (kAlign[c].byte == (byte_mode ? 1 : 0) && qlen <= kAlign[c].slen * (byte_mode ? 16 : 8)) return c;
    return -1;
}
static const int kGlobal[] = {1, 2, 4, 8, 16};
int global_class_count() { return 5; }
int global_class_cols(int c) { return kGlobal[c] * 64; }

/* ---- staging ---- */
hipError_t launch_rebase(bsw_dtask *tasks, const bsw_rawoff *roff, uint32_t n, const bsw_rebase &rb_, hipStream_t s)
{
    STANDIN_GATE("launch_rebase");
    const bsw_rebase rb = rb_;
    hipdbl::enqueue(s, [=]() {
        for (uint32_t i = 0; i < n; ++i) {
            bsw_dtask &T = tasks[i];
            if (rb.use_ro) {
                T.lq_off = roff[i].lq + rb.delta; T.lt_off = roff[i].lt + rb.delta; T.rq_off = roff[i].rq + rb.delta; T.rt_off = roff[i].rt + rb.delta;
            } else {
                uint32_t k = i / rb.per;
                if (k >= rb.nr) k = rb.nr - 1u;
                T.lq_off += rb.base[k]; T.lt_off += rb.base[k]; T.rq_off += rb.base[k]; T.rt_off += rb.base[k];
            }
        }
    });
    return hipSuccess;
}

hipError_t launch_pack(const uint8_t *raw, const bsw_dtask *tasks, const bsw_rawoff *roff, uint32_t bias, uint32_t n, int rev_left,
                       const uint8_t *pac, int64_t l_pac, const bsw_refx *refx, uint64_t *seq, uint8_t *nflag, hipStream_t s)
{
    STANDIN_GATE("launch_pack");
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        if (pac && n && hipdbl::device_of_ptr(pac, (size_t)((l_pac + 3) >> 2)) != dev)
            hipdbl::die("stand-in launch_pack: the reference copy handed to a chunk of device %d does not live there", dev);
        {                                               /* a new chunk: a round a failed call left open ends unchecked */
            std::lock_guard<std::mutex> lk(B().mu);
            B().pack_n[seq] = n;
            for (auto it = B().f4.begin(); it != B().f4.end();) it = it->second.seq == seq ? B().f4.erase(it) : std::next(it);
        }
        for (uint32_t ti = 0; ti < n; ++ti) {
            const bsw_dtask &T = tasks[ti];
            int hasn = 0;
            for (int which = 0; which < 4; ++which) {
                const bool target = which & 1, left = which < 2;
                const int qlen = left ? T.lqlen : T.rqlen;
                const int len = target ? (qlen ? (left ? T.ltlen : T.rtlen) : 0) : qlen;
                const uint32_t woff = which == 0 ? T.lq_off : which == 1 ? T.lt_off : which == 2 ? T.rq_off : T.rt_off;
                if (!len) continue;
                const int nw = (len + 15) >> 4;
                for (int w = 0; w < nw; ++w) {
                    uint64_t v = 0;
                    for (int k = 16 * w; k < len && k < 16 * w + 16; ++k) {
                        uint64_t b;
                        if (pac && target) b = (uint64_t)base_of_pac(pac, l_pac, left ? refx[ti].xl - k : refx[ti].xr + k);
                        else {
                            const bsw_rawoff &R = roff[ti];
                            const uint32_t boff = (which == 0 ? R.lq : which == 1 ? R.lt : which == 2 ? R.rq : R.rt) - bias;
                            const uint8_t *base = raw + boff;
                            const uint8_t c = (rev_left && which == 0) ? *(base - k) : base[k];
                            b = c > 4 ? 4u : c;
                        }
                        v |= b << (4 * (k & 15));
                        if (!target && b >= 4) hasn |= left ? 1 : 2;
                    }
                    seq[woff + (uint32_t)w] = v;
                }
            }
            if (nflag) nflag[ti] = (uint8_t)hasn;
        }
    });
    return hipSuccess;
}

hipError_t launch_wire_pack(const uint32_t *wire, const bsw_dtask *tasks, const bsw_wireoff *woffs, uint32_t n, uint64_t *seq, hipStream_t s)
{
    STANDIN_GATE("launch_wire_pack");
    hipdbl::enqueue(s, [=]() {
        for (uint32_t ti = 0; ti < n; ++ti) {
            const bsw_dtask &T = tasks[ti];
            const bsw_wireoff &W = woffs[ti];
            /* stream order: leftQ, rightQ, leftT, rightT; 8 nibbles per word, the first base in bits [31:28] */
            const int len[4] = {T.lqlen, T.lqlen ? T.ltlen : 0, T.rqlen, T.rqlen ? T.rtlen : 0};
            const uint32_t woff[4] = {T.lq_off, T.lt_off, T.rq_off, T.rt_off};
            const uint32_t nib[4] = {W.nib, W.nib + W.lqlen + W.rqlen, W.nib + W.lqlen, W.nib + W.lqlen + W.rqlen + W.ltlen};
            for (int which = 0; which < 4; ++which)
                for (int w = 0; w < (len[which] + 15) >> 4; ++w) {
                    uint64_t v = 0;
                    for (int k = 16 * w; k < len[which] && k < 16 * w + 16; ++k) {
                        const uint32_t nb = nib[which] + (uint32_t)k;
                        uint64_t b = (wire[nb >> 3] >> (28 - 4 * (nb & 7u))) & 0xfu;
                        if (b > 4) b = 4;
                        v |= b << (4 * (k & 15));
                    }
                    seq[woff[which] + (uint32_t)w] = v;
                }
        }
    });
    return hipSuccess;
}

hipError_t launch_wire_results(const bsw_result *out, const bsw_wireoff *woffs, uint32_t n, uint32_t *wout, size_t wout_words, hipStream_t s)
{
    STANDIN_GATE("launch_wire_results");
    hipdbl::enqueue(s, [=]() {
        memset(wout, 0, wout_words * sizeof(uint32_t));
        for (uint32_t ti = 0; ti < n; ++ti) {
            const bsw_result &r = out[ti];
            uint32_t *R = wout + woffs[ti].out_word;
            R[0] = r.tag;
            R[1] = ((uint32_t)r.qe << 16) | ((uint32_t)r.qb & 0xffffu);
            R[2] = ((uint32_t)r.re << 16) | ((uint32_t)r.rb & 0xffffu);
            R[3] = ((uint32_t)r.truesc << 16) | ((uint32_t)r.score & 0xffffu);
            R[4] = (uint32_t)r.w;
        }
    });
    return hipSuccess;
}

/* ---- binning: the host plan's own order ---- */
hipError_t launch_bin(const bsw_binparams &bp_, const uint64_t *seq, const uint8_t *nflag, const bsw_dtask *tasks, uint32_t n, uint32_t *bins,
                      uint64_t *keys, uint32_t *order, hipStream_t s)
{
    STANDIN_GATE("launch_bin");
    if (n == 0) return hipSuccess;
    const bsw_binparams bp = bp_;
    hipdbl::enqueue(s, [=]() {
        auto lg = std::make_shared<ledger_t>();
        lg->n = n; lg->order = order; lg->bp = bp;
        lg->L.assign(n, 0); lg->R.assign(n, 0); lg->W.assign(n, 0);
        const size_t cap = bsw_plan_order_capacity(n);
        if (bp.nsplit && ((size_t)bp.nlist_off + bp.nlist_cap > cap || bp.nlist_cnt_at >= cap || (size_t)bp.fill_off + bp.fill_len > cap))
            hipdbl::die("stand-in launch_bin: the N list [%u, +%u), its counter at %u or the fill [%u, +%u) leave the %zu words of order[] (n = %u)",
                        bp.nlist_off, bp.nlist_cap, bp.nlist_cnt_at, bp.fill_off, bp.fill_len, cap, n);
        {
            std::lock_guard<std::mutex> lk(B().mu);
            B().by_tasks[tasks] = lg;
            const uint64_t end = (uint64_t)bp.nlist_off + bp.nlist_cap;
            if (bp.nsplit && end > B().max_end) B().max_end = end;
            if (bp.nsplit && end > 4ull * n + 16) ++B().beyond;
        }
        memset(bins, 0, BSW_BIN_WORDS * sizeof(uint32_t));      /* (the kernels' scratch: touched so that its size is checked) */
        memset(keys, 0, (size_t)n * sizeof(uint64_t));
        std::vector<uint8_t> nf(n);
        for (uint32_t i = 0; i < n; ++i)
            nf[i] = nflag ? nflag[i] : (uint8_t)((words_have_n(seq, tasks[i].lq_off, tasks[i].lqlen) ? 1 : 0) | (words_have_n(seq, tasks[i].rq_off, tasks[i].rqlen) ? 2 : 0));
        const uint32_t cnt = plan_fill_order(bp, tasks, n, nf.data(), order);
        if (bp.nsplit) order[bp.nlist_cnt_at] = cnt;
    });
    return hipSuccess;
}

/* ---- DP ---- */
hipError_t launch_wave(int cls, int variant, const bsw_dparams &P_, const uint64_t *seq, const bsw_dtask *tasks,
                       const uint32_t *order, uint32_t n, const uint32_t *n_dev, uint32_t *, bsw_result *out, hipStream_t s)
{
    STANDIN_GATE("launch_wave");
    if (n == 0) return hipSuccess;
    if (cls < 0 || cls >= wave_class_count()) return hipErrorInvalidValue;
    const bsw_dparams P = P_;
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        const auto lg = ledger_of(tasks);
        check_slice(lg.get(), order, n, "launch_wave");
        const uint32_t cnt = n_dev ? __atomic_load_n(n_dev, __ATOMIC_ACQUIRE) : n;
        if (cnt > n) hipdbl::die("stand-in launch_wave: the device-side count %u exceeds the launch's bound %u", cnt, n);
        std::vector<uint32_t> tags;
        for (uint32_t slot = 0; slot < cnt; ++slot) {
            const uint32_t ti = order[slot];
            if (ti == BSW_ORDER_NONE) hipdbl::die("stand-in launch_wave: an unfilled entry inside the counted part of a list (slot %u of %u)", slot, cnt);
            note_seed(lg.get(), ti, "launch_wave");
            const bsw_dtask &T = tasks[ti];
            if (std::max(T.lqlen, T.rqlen) + 1 > wave_class_cols(cls)) hipdbl::die("stand-in launch_wave: seed %u (%d / %d bases) does not fit class %d", ti, T.lqlen, T.rqlen, cls);
            compute(P, variant, seq, T, &out[ti]);
            if (lg) ++lg->W[ti];
            tags.push_back(T.tag);
        }
        remember(out, tasks, dev, tags);
    });
    return hipSuccess;
}

hipError_t launch_lane(int cls, int variant, const bsw_dparams &P_, int side, const uint64_t *seq, const bsw_dtask *tasks,
                       const uint32_t *order, uint32_t n, bsw_result *out, hipStream_t s, uint32_t *tail_flag, uint32_t *tail_target, const bsw_fin *fin_)
{
    STANDIN_GATE("launch_lane");
    if (tail_target) *tail_target = 1u;
    if (cls < 0 || cls >= lane_class_count() || side < 0 || side > 2) return hipErrorInvalidValue;
    const bsw_dparams P = P_;
    const bool has_fin = fin_ != nullptr;
    const bsw_fin fin = has_fin ? *fin_ : bsw_fin();
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        const auto lg = ledger_of(tasks);
        check_slice(lg.get(), order, n, "launch_lane");
        std::vector<uint32_t> tags;
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint32_t ti = order[slot];
            if (ti == BSW_ORDER_NONE) continue;             /* (a list's unused tail: bsw_binparams.nsplit) */
            note_seed(lg.get(), ti, "launch_lane");
            const bsw_dtask &T = tasks[ti];
            const int q = side == 0 ? T.lqlen : side == 1 ? T.rqlen : std::max(T.lqlen, T.rqlen);
            if (q + 1 > lane_class_cols(cls)) hipdbl::die("stand-in launch_lane: seed %u, side %d (%d bases) does not fit class %d", ti, side, q, cls);
            if (side != 2 && q == 0) hipdbl::die("stand-in launch_lane: seed %u is on the list of a side it does not have (side %d)", ti, side);
            compute(P, variant, seq, T, &out[ti]);
            if (has_fin && fin.on && fin.pairs) as_pair(out[ti], &fin.pairs[ti]);
            if (lg) { if (side != 1) ++lg->L[ti]; if (side != 0) ++lg->R[ti]; }
            if (side != 1 || !T.lqlen) tags.push_back(T.tag);      /* (once per seed: with its left side, or its only one) */
        }
        remember(out, tasks, dev, tags);
        if (has_fin && fin.pairs) remember(fin.pairs, tasks, dev, std::vector<uint32_t>());
        if (tail_flag) __atomic_store_n(tail_flag, 1u, __ATOMIC_RELEASE);
    });
    return hipSuccess;
}

hipError_t launch_wait_count(const uint32_t *flag, uint32_t target, uint32_t *expired, hipStream_t s)
{
    STANDIN_GATE("launch_wait_count");
    { std::lock_guard<std::mutex> lk(B().mu); ++B().waits; }
    hipdbl::enqueue(s, [=]() {
        const auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) < target) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {      /* the kernel's bound */
                if (expired) __atomic_fetch_add(expired, 1u, __ATOMIC_RELAXED);
                break;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    });
    return hipSuccess;
}

hipError_t launch_finalize(const bsw_dparams &, const bsw_dtask *tasks, const uint32_t *order, uint32_t n,
                           bsw_result *out, uint32_t *, uint32_t *, bsw_pair *pairs, hipStream_t s)
{
    STANDIN_GATE("launch_finalize");
    hipdbl::enqueue(s, [=]() {
        const auto lg = ledger_of(tasks);
        check_slice(lg.get(), order, n, "launch_finalize");
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint32_t ti = order[slot];
            if (ti == BSW_ORDER_NONE) continue;
            note_seed(lg.get(), ti, "launch_finalize");
            if (lg && !(lg->L[ti] | lg->R[ti])) hipdbl::die("stand-in launch_finalize: seed %u reached the pair decision with no side computed", ti);
            if (pairs) as_pair(out[ti], &pairs[ti]);
        }
        if (pairs) remember(pairs, tasks, -1, std::vector<uint32_t>());
    });
    return hipSuccess;
}

hipError_t launch_pairs_from_results(const uint32_t *order, uint32_t n, const uint32_t *n_dev, const bsw_result *out, bsw_pair *pairs, hipStream_t s)
{
    STANDIN_GATE("launch_pairs_from_results");
    if (n == 0) return hipSuccess;
    hipdbl::enqueue(s, [=]() {
        const uint32_t cnt = n_dev ? __atomic_load_n(n_dev, __ATOMIC_ACQUIRE) : n;
        if (cnt > n) hipdbl::die("stand-in launch_pairs_from_results: the device-side count %u exceeds the launch's bound %u", cnt, n);
        const void *tasks = nullptr;
        { std::lock_guard<std::mutex> lk(B().mu); auto it = B().owner.find(out); if (it != B().owner.end()) tasks = it->second; }
        for (uint32_t slot = 0; slot < cnt; ++slot) as_pair(out[order[slot]], &pairs[order[slot]]);
        if (tasks) remember(pairs, tasks, -1, std::vector<uint32_t>());
    });
    return hipSuccess;
}

/* ---- banded global alignment, local alignment, NM / MD (see the file header: F4) ---- */
static hipError_t global_standin(const char *who, int cols, int ring, const bsw_dparams &P_, const uint64_t *seq, const bsw_gdtask *tasks,
                                 const uint32_t *order, uint32_t n, uint8_t *z, uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    const bsw_dparams P = P_;
    hipdbl::enqueue(s, [=]() {
        std::vector<uint8_t> q, t;
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint32_t idx = order[slot];
            const bsw_gdtask &T = tasks[idx];
            const int n_col = T.qlen < 2 * T.w + 1 ? T.qlen : 2 * T.w + 1;
            if (cols && T.qlen + 1 > cols) hipdbl::die("stand-in %s: task %u (%d query bases) does not fit a class of %d columns", who, idx, T.qlen, cols);
            if (ring && n_col + 1 > ring) hipdbl::die("stand-in %s: task %u (band of %d columns) does not fit a ring of %d records", who, idx, n_col, ring);
            const uint64_t zlen = z ? (uint64_t)(n_col > 0 ? n_col : 0) * (uint64_t)T.tlen : 0;
            f4_note(out, seq, idx, T.z_off, zlen, who);
            if (zlen) { z[T.z_off] = 0; z[T.z_off + zlen - 1] = 0; }
            unpack(seq, T.q_off, T.qlen, q);
            unpack(seq, T.t_off, T.tlen, t);
            int nc = 0;
            uint32_t *cg = nullptr;
            bsw_gresult r;
            r.score = ksw_global2_ref(T.qlen, q.data(), T.tlen, t.data(), 5, P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, T.w, z ? &nc : nullptr, z ? &cg : nullptr, nullptr);
            r.n_cigar = nc <= max_cigar ? nc : -nc;
            if (z && cigars)
                for (int k = 0; k < nc && k < max_cigar; ++k) cigars[(size_t)idx * (size_t)max_cigar + (size_t)k] = cg[k];
            free(cg);
            out[idx] = r;
        }
    });
    return hipSuccess;
}

hipError_t launch_global_long(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *order, uint32_t n, uint8_t *z,
                              uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    STANDIN_GATE("launch_global_long");
    if (n == 0) return hipSuccess;
    if (cls < 0 || cls >= GLOBAL_LONG_CLASSES) return hipErrorInvalidValue;
    return global_standin("launch_global_long", 0, long_ring(cls), P, seq, tasks, order, n, z, cigars, max_cigar, out, s);
}

hipError_t launch_global(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *order, uint32_t n, uint8_t *z,
                         uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    if (n && cls >= global_class_count()) return launch_global_long(cls - global_class_count(), P, seq, tasks, order, n, z, cigars, max_cigar, out, s);
    STANDIN_GATE("launch_global");
    if (n == 0) return hipSuccess;
    if (cls < 0) return hipErrorInvalidValue;
    return global_standin("launch_global", global_class_cols(cls), 0, P, seq, tasks, order, n, z, cigars, max_cigar, out, s);
}

hipError_t launch_align(int cls, const bsw_dparams &P_, const uint64_t *seq, const bsw_adtask *tasks, const uint32_t *order, uint32_t n,
                        unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    STANDIN_GATE("launch_align");
    if (n == 0) return hipSuccess;
    if (cls < 0 || cls >= align_class_count()) return hipErrorInvalidValue;
    const bsw_dparams P = P_;
    hipdbl::enqueue(s, [=]() {
        std::vector<uint8_t> q, t;
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint32_t idx = order[slot];
            const bsw_adtask &T = tasks[idx];
            const int want = align_class_of(T.qlen, (T.xtra & KSW_XBYTE) != 0);
            if (want != cls) hipdbl::die("stand-in launch_align: task %u (%d query bases, xtra 0x%x) belongs to class %d and is listed for class %d", idx, T.qlen, (unsigned)T.xtra, want, cls);
            const uint64_t blen = (T.xtra & KSW_XSUBO) ? (uint64_t)T.tlen : 0;
            f4_note(out, seq, idx, T.b_off, blen, "launch_align");
            if (blen) { blist[T.b_off] = 0; blist[T.b_off + blen - 1] = 0; }
            unpack(seq, T.q_off, T.qlen, q);
            unpack(seq, T.t_off, T.tlen, t);
            if (T.pad & BSW_AD_QRC) {
                std::reverse(q.begin(), q.end());
                for (uint8_t &c : q) c = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4;
            }
            int32_t r[7];
            ksw_align2_ref(T.qlen, q.data(), T.tlen, t.data(), 5, P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, T.xtra, r, nullptr);
            memcpy(&out[idx], r, sizeof(bsw_kswr));
        }
    });
    return hipSuccess;
}

hipError_t launch_cigar_md(const bsw_dparams &P_, const uint64_t *seq, const bsw_cdtask *tasks, uint32_t n, uint32_t *cigars, int max_cigar,
                           const bsw_gresult *gres, char *md, int max_md, bsw_cresult *res, hipStream_t s)
{
    STANDIN_GATE("launch_cigar_md");
    if (n == 0) return hipSuccess;
    const bsw_dparams P = P_;
    hipdbl::enqueue(s, [=]() {
        std::vector<uint8_t> q, t;
        for (uint32_t ti = 0; ti < n; ++ti) {
            const bsw_cdtask &T = tasks[ti];
            char *slot = md ? md + (size_t)ti * (size_t)max_md : nullptr;
            uint32_t *cg = cigars + (size_t)ti * (size_t)max_cigar;
            bsw_cresult r;
            memset(&r, 0, sizeof(r));
            const bool nogap = (T.flags & BSW_CD_NOGAP) != 0;
            int n_cigar;
            if (T.flags & BSW_CD_STATUS) n_cigar = -1;
            else if (nogap) { n_cigar = 1; cg[0] = (uint32_t)T.qlen << 4; }
            else { r.score = gres[ti].score; n_cigar = gres[ti].n_cigar; }
            if (n_cigar < 0) {                               /* no alignment, or a CIGAR that did not fit: no NM, no MD */
                if (!(T.flags & BSW_CD_STATUS)) r.n_cigar = n_cigar;
                r.nm = -1;
                if (slot) slot[0] = 0;
                res[ti] = r;
                continue;
            }
            unpack(seq, T.q_off, T.qlen, q);
            unpack(seq, T.t_off, T.tlen, t);
            const char *letters = (T.flags & BSW_CD_REV) ? "TGCAN" : "ACGTN";
            std::string m;
            int x = 0, y = 0, u = 0, nm = 0, sc = 0;
            for (int k = 0; k < n_cigar; ++k) {
                const int op = (int)(cg[k] & 0xf), len = (int)(cg[k] >> 4);
                if (op == 0) {
                    for (int i = 0; i < len; ++i) {
                        const int qb = q[(size_t)(x + i)] < 4 ? q[(size_t)(x + i)] : 4, tb = t[(size_t)(y + i)] < 4 ? t[(size_t)(y + i)] : 4;
                        sc += P.mat[tb * 5 + qb];
                        if (qb != tb) { m += std::to_string(u); m += letters[tb]; u = 0; ++nm; }
                        else ++u;
                    }
                    x += len; y += len;
                } else if (op == 2) {
                    if (k > 0 && k < n_cigar - 1) {          /* a leading or trailing D is in neither MD nor NM */
                        m += std::to_string(u); m += '^';
                        for (int i = 0; i < len; ++i) m += letters[t[(size_t)(y + i)] < 4 ? t[(size_t)(y + i)] : 4];
                        u = 0; nm += len;
                    }
                    y += len;
                } else if (op == 1) { x += len; nm += len; }
            }
            m += std::to_string(u);
            if (nogap) r.score = sc;
            r.n_cigar = n_cigar;
            r.nm = nm;
            r.md_len = (int32_t)m.size();
            if (slot) {
                if ((int)m.size() < max_md) memcpy(slot, m.c_str(), m.size() + 1);
                else { slot[0] = 0; r.md_len = -((int32_t)m.size() + 1); }
            }
            r.tries = nogap ? ((T.more && r.score < T.min_score) ? 2 : 1) : 0;
            res[ti] = r;
        }
    });
    return hipSuccess;
}

}  // namespace bsw
