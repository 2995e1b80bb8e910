/* bsw_f4_host.h — internal: what global_chunk / align_chunk (bsw_f4.hip), cigar_chunk / patch_chunk (bsw_cigar.hip) and matesw_chunk
 * (bsw_matesw.hip) share, each written once: the span of the caller's bytes with the direct-DMA test, per-class task lists, kernel
 * routing and launch loops, reservations in a row, a task's layout as a one-sided seed, staging the sequences on a lane, reading a
 * lane back, cutting a call into sub-batches, and the entry prologue, the read-block wrapper and the work switch of the three
 * stages against the resident reference.  Nothing here
 * keeps state (but the one getenv of global_force_long): chunks run concurrently on slot threads.  Non-inline bodies: bsw_f4.hip. */
#ifndef BSW_F4_HOST_H
#define BSW_F4_HOST_H

#include "bsw_internal.h"

#include <initializer_list>

/* ---- what every entry point of the stages against the resident reference (bsw_cigar_ref_*, bsw_matesw_ref_*, bsw_patch_ref_*) does
 * first, in this order: its own argument test (bad_args, evaluated by the caller: "<what>: bad argument"), the reference belongs to
 * this context, then busy_check for a synchronous call, or "the context is dead" for a ticket form.  A synchronous call writes the
 * context's error text directly; a ticket form may run beside others and sets it under the context's lock (ctx_fail). ---- */
BSW_LOCAL int ref_entry_check(bsw_ctx *ctx, const char *what, bool bad_args, const bsw_ref *ref, bool ticket_form);
/* a *_reads_submit_t: takes the block, runs the stage's submit() and gives the block back when no ticket was made (the ticket owns
 * the block only once it exists: BSW_E_BUSY included) */
template <class F>
inline int reads_submit(bsw_ctx *ctx, const bsw_reads *rd, bsw_ticket *ticket, const char *what, F submit)
{
    if (!ctx) return BSW_E_INVAL;
    if (ticket) *ticket = 0;
    errs e;
    if (!rd) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: bad argument", what));
    if (!reads_acquire(ctx, rd)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: the read block was uploaded through another context, or is being freed", what));
    const int rc = submit();
    if (rc) reads_release(rd);
    return rc;
}
/* a chunk's work target from the environment (BSW_F4_*_WORK: tests, measurements): set and >= 1, else dflt.  The callers cache it. */
BSW_LOCAL uint64_t chunk_work_env(const char *name, uint64_t dflt);

/* ---- the caller's bytes a chunk references: their span and sum ---- */
struct raw_span {
    const uint8_t *lo = (const uint8_t *)UINTPTR_MAX, *hi = nullptr;
    uint64_t bytes = 0;               /* (before add(): the piece's offset in a gather) */
    void add(const uint8_t *p, size_t len)
    {
        if (!len) return;
        bytes += len;
        if (p < lo) lo = p;
        if (p + len > hi) hi = p + len;
    }
    size_t span() const { return hi ? (size_t)(hi - lo) : 0; }
    /* DMA the caller's arena as it lies: registered, addressable in 32 bits with `slack` bytes of read-ahead, not much larger than what it holds */
    bool direct(size_t slack) const
    {
        const size_t spanb = span();
        return spanb > 0 && spanb < (1ull << 32) - slack && spanb <= 2 * bytes + (1u << 20) && is_registered(lo, spanb);
    }
};

/* ---- tasks sorted by kernel class: class c owns order[begin(c) .. begin(c) + count(c)), in input order (a stable counting
 * sort).  Owns host memory a queued copy reads: declare it in front of the drain_on_failure guard. ---- */
struct class_lists {
    std::vector<uint32_t> order, cnt;
    /* entry i of k has class cls[i] and names task ids[i] (ids == NULL: task i) */
    void build(int n_classes, const uint32_t *cls, const uint32_t *ids, size_t k)
    {
        cnt.assign((size_t)n_classes + 1, 0u);
        for (size_t i = 0; i < k; ++i) ++cnt[(size_t)cls[i] + 1];
        for (int c = 0; c < n_classes; ++c) cnt[(size_t)c + 1] += cnt[(size_t)c];
        order.assign(k, 0u);
        std::vector<uint32_t> pos(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < k; ++i) order[pos[cls[i]]++] = ids ? ids[i] : (uint32_t)i;
    }
    int classes() const { return (int)cnt.size() - 1; }
    uint32_t begin(int c) const { return cnt[(size_t)c]; }
    uint32_t count(int c) const { return cnt[(size_t)c + 1] - cnt[(size_t)c]; }
};

/* ---- routing.  launch_global's class for a query of qlen bases under a band of n_col columns: the register classes by qlen,
 * behind them the LDS ring classes by n_col (every task under BSW_GLOBAL_LONG=1: fuzzing, rate A/B).  One per chunk. ---- */
BSW_LOCAL bool global_force_long();   /* the one read of BSW_GLOBAL_LONG */
struct global_route {
    const int ncls = bsw::global_class_count();
    const bool force_long = global_force_long();
    int classes() const { return ncls + bsw::GLOBAL_LONG_CLASSES; }
    int operator()(int qlen, int n_col) const
    {
        int c = 0;
        while (c < ncls && qlen + 1 > bsw::global_class_cols(c)) ++c;
        if (c == ncls || force_long) c = ncls + bsw::global_long_class_of(n_col);
        return c;
    }
};
/* an alignment's class among nall = ncls (bsw_align_kernel) + the LDS-row classes behind them; negative: none (the caller's BSW_E_LIMIT) */
inline int align_route(int al_mode, int qlen, bool byte_mode, int ncls, int nall)
{
    const int lc = align_long_route(al_mode, qlen, byte_mode);
    const int c = lc == -1 ? bsw::align_class_of(qlen, byte_mode) : lc < 0 ? -1 : ncls + lc;
    return c < nall ? c : -1;
}
/* what ksw_u8 has no byte for (include/bwa_sw_mi355.h at KSW_XBYTE): a matrix whose smallest entry is above 0 (the shift
 * 256 - min wraps and the stored profile byte with it), a gap open + extend beyond 255 (an 8-bit lane in bwa).  BSW_OK, or the
 * rejection of `what` task i whose flags are xtra; 16-bit mode has neither limit. */
inline int align_byte_mode_check(errs &e, const bsw_params *p, int xtra, const char *what, size_t i)
{
    if (!(xtra & KSW_XBYTE)) return BSW_OK;
    int mn = p->mat[0];
    for (int k = 1; k < 25; ++k) mn = std::min(mn, (int)p->mat[k]);
    if (mn > 0) return fail(e, BSW_E_INVAL, "%s task %zu: KSW_XBYTE with a scoring matrix whose smallest entry is %d > 0 (the 8-bit shift wraps; run it in 16-bit mode)", what, i, mn);
    if (p->o_del + p->e_del > 255 || p->o_ins + p->e_ins > 255)
        return fail(e, BSW_E_LIMIT, "%s task %zu: KSW_XBYTE with a gap open + extend above 255 (an 8-bit lane in bwa; run it in 16-bit mode)", what, i);
    return BSW_OK;
}

/* ---- growing several buffers in the order given, up to the first that fails: "<what>: <HIP's text>" with BSW_E_NOMEM (what: "device staging"
 * or "pinned staging").  An entry whose `on` is false is skipped. ---- */
struct reserve_req {
    void *buf;
    size_t need;
    hipError_t (*grow)(void *, size_t);
    template <class B>
    reserve_req(B &b, size_t n, bool on = true) : buf(on ? &b : nullptr), need(n), grow([](void *p, size_t k) { return ((B *)p)->reserve(k); }) {}
};
inline int reserve_all(errs &e, const char *what, std::initializer_list<reserve_req> list)
{
    for (const reserve_req &r : list) {
        const hipError_t he = r.buf ? r.grow(r.buf, r.need) : hipSuccess;
        if (he != hipSuccess) return fail(e, BSW_E_NOMEM, "%s: %s", what, hipGetErrorString(he));
    }
    return BSW_OK;
}

/* ---- one launch per class that holds a task, ascending; d_order: the device copy of cl.order; alo: the LDS-row kernel's classes
 * behind the ncls of bsw_align_kernel ---- */
BSW_LOCAL int launch_global_lists(errs &e, const class_lists &cl, const bsw_dparams &dp, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *d_order,
                                  uint8_t *z, uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s);
BSW_LOCAL int launch_align_lists(errs &e, const class_lists &cl, const align_long_ops *alo, const bsw_dparams &dp, const uint64_t *seq, const bsw_adtask *tasks,
                                 const uint32_t *d_order, unsigned long long *blist, bsw_kswr *out, hipStream_t s);
/* the global kernels on a lane's packed sequences: the host-built records gt[0..n) and cl.order go to the lane's g_tasks / g_order (a slot: through its
 * pinned h_in, at in_gt / in_order), counted in L.h2d, then launch_global_lists into the lane's g_res.  (global_chunk queues the same copies in front of
 * its pack launch and keeps that order.) */
BSW_LOCAL int upload_launch_global(errs &e, f4_lane &L, const class_lists &cl, const bsw_dparams &dp, const bsw_gdtask *gt, size_t n, size_t in_gt, size_t in_order,
                                   uint8_t *z, uint32_t *cigars, int max_cigar);

/* ---- staging the sequences of a chunk on a lane.  The caller: stage_records, fills h_tasks / h_roff (/ h_desc) with offsets of a gather
 * (raw_span::bytes as it goes), stage_raw, its own reservations, its drain_on_failure, stage_upload, its own records, stage_pack. ---- */
BSW_LOCAL int stage_records(errs &e, stage_t &st, size_t n, bool desc);
/* Task i against the resident reference as a one-sided seed of bsw_pack_kernel.  clear_records: a task that does not run.  lay_interval: lq query
 * bases from `at` (a byte offset into the raw bytes, or the base's position in the resident read store) against the reference interval [rb, re)
 * of rlen bases.  rev: left side only, the query read backwards from its last base and the target downwards from re - 1 — bwa's reversal of
 * both, for free; else right side only, the query read forwards and the target upwards from rb.  The sequences' words start at acc, which moves
 * on; returns where the query's and the target's begin. */
inline void clear_records(stage_t &st, size_t i)
{
    memset(&st.h_tasks.p[i], 0, sizeof(bsw_dtask));
    memset(&st.h_roff.p[i], 0, sizeof(bsw_rawoff));
    st.h_desc.p[i] = bsw_refx{0, 0};
}
struct interval_words { uint32_t qw, tw; };
inline interval_words lay_interval(stage_t &st, size_t i, int lq, int rlen, bool rev, uint32_t at, int64_t rb, int64_t re, uint64_t &acc)
{
    clear_records(st, i);
    bsw_dtask &d = st.h_tasks.p[i];
    const interval_words w{(uint32_t)acc, (uint32_t)(acc + nwords(lq))};
    acc += nwords(lq) + nwords(rlen);
    if (rev) {
        d.lq_off = w.qw; d.lt_off = w.tw; d.lqlen = (uint16_t)lq; d.ltlen = (uint16_t)rlen;
        st.h_roff.p[i].lq = at + (uint32_t)lq - 1u;
        st.h_desc.p[i].xl = re - 1;
    } else {
        d.rq_off = w.qw; d.rt_off = w.tw; d.rqlen = (uint16_t)lq; d.rtlen = (uint16_t)rlen;
        st.h_roff.p[i].rq = at;
        st.h_desc.p[i].xr = rb;
    }
    return w;
}
/* a task's sequence as the caller holds it: p[0..len), the field of its bsw_rawoff that names it (last: names its LAST byte, read backwards); len == 0: none */
struct raw_piece { const uint8_t *p; size_t len; uint32_t bsw_rawoff::*at; bool last; };
struct staged_raw {                   /* what crosses PCIe: the caller's arena from raw_span::lo, or h_raw (resident reads: nothing) */
    const uint8_t *src = nullptr;
    size_t bytes = 0;
    bool desc = false;
};
/* decides direct or gather; rewrites the offsets relative to the span, or gathers into h_raw (gather_empty: h_raw is reserved for a chunk without
 * a byte too — the host's own HIP call sequence); reserves the device side.  piece(i, k): piece k of the `pieces` of task i. */
template <class F>
inline int stage_raw(errs &e, stage_t &st, size_t n, const raw_span &sp, uint64_t words, bool desc, bool gather_empty, int pieces, F piece, staged_raw *out)
{
    int rc;
    const bool direct = sp.direct(RAW_SLACK);
    if (direct) {
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < pieces; ++k) {
                const raw_piece pc = piece(i, k);
                st.h_roff.p[i].*pc.at = pc.len ? (uint32_t)(pc.p - sp.lo) + (pc.last ? (uint32_t)pc.len - 1u : 0u) : 0u;
            }
    } else if (gather_empty || sp.bytes) {
        if ((rc = reserve_all(e, "pinned staging", {{st.h_raw, (size_t)sp.bytes + RAW_SLACK}})) != BSW_OK) return rc;
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < pieces; ++k) {
                const raw_piece pc = piece(i, k);
                if (pc.len) memcpy(st.h_raw.p + (st.h_roff.p[i].*pc.at - (pc.last ? (uint32_t)pc.len - 1u : 0u)), pc.p, pc.len);
            }
    }
    out->bytes = direct ? sp.span() : (size_t)sp.bytes;
    out->src = direct ? sp.lo : st.h_raw.p;
    out->desc = desc;
    return reserve_all(e, "device staging", {{st.d_raw, out->bytes + RAW_FRONT + RAW_SLACK}, {st.d_seq, (size_t)words + 4}, {st.d_tasks, n + 1}, {st.d_roff, n + 1},
                                             {st.d_desc, n + 1, desc}});
}
/* queues the raw bytes (behind RAW_FRONT), the task records, the offsets and the reference positions; counts them in L.h2d */
BSW_LOCAL int stage_upload(errs &e, f4_lane &L, const staged_raw &r, size_t n);
/* queues bsw_pack_kernel.  ref: targets fetched from the lane's copy of the reference at h_desc; rd: queries from the lane's copy of the resident
 * read block (BSW_PACK_STORE), behind an upload of it still in flight */
BSW_LOCAL int stage_pack(errs &e, f4_lane &L, size_t n, int flags, const bsw_ref *ref, const bsw_reads *rd);

/* ---- results back from a lane, behind everything queued on it: a slot lane copies into h_back at running offsets in front of the
 * wait that carries the watchdog, then into dst (dst == NULL: the caller reads them in h_back); the context's lane waits, then
 * copies blocking.  An entry without bytes is skipped.  The caller has reserved h_back. ---- */
struct back_copy { void *dst; const void *src; size_t bytes; };
BSW_LOCAL int lane_read_back(bsw_ctx *ctx, errs &e, f4_lane &L, std::initializer_list<back_copy> list);

/* ---- cutting a call's n tasks into sub-batches ---- */
struct span_cost {                    /* what one task adds to a sub-batch */
    uint64_t z, seq, bl, work;        /* backtrack bytes, sequence bytes, sub-optimal-list entries, work */
    /* What the bounds are probed with.  The hosts probe z and bl with the task's full size and accumulate only what the task is
     * given (bsw_global_batch without CIGARs: no backtrack bytes; a task without KSW_XSUBO: no list slice): kept as it is. */
    uint64_t z_probe, bl_probe;
};
struct span_caps {
    uint64_t tasks = 1u << 20, z = 4ull << 30, seq = 1ull << 31, bl = 1ull << 28;      /* hard: a sub-batch exceeds one only as a single task */
    uint64_t out_per_task = 0, out = UINT64_MAX;      /* hard: bytes of output per task x tasks */
    uint64_t work = UINT64_MAX;       /* soft: a sub-batch is closed once it HOLDS its share of the work, so no sliver is left over */
};
template <class F>
inline std::vector<chunk_span> cut_spans(size_t n, F cost_of, const span_caps &caps)
{
    std::vector<chunk_span> spans;
    for (size_t a = 0; a < n;) {
        size_t b = a;
        uint64_t zb = 0, sb = 0, bb = 0, wb = 0;
        while (b < n && b - a < caps.tasks) {
            const span_cost c = cost_of(b);
            if (b > a && (wb >= caps.work || zb + c.z_probe > caps.z || sb + c.seq > caps.seq || bb + c.bl_probe > caps.bl ||
                          (uint64_t)(b - a + 1) * caps.out_per_task > caps.out))
                break;
            zb += c.z; sb += c.seq; bb += c.bl; wb += c.work;
            ++b;
        }
        spans.push_back(chunk_span{a, b - a});
        a = b;
    }
    return spans;
}

#endif
