/*
 * bsw_reads_async.hip — the asynchronous upload of a resident read block: bsw_reads_upload_start / bsw_reads_test /
 * bsw_reads_wait / bsw_reads_image (part of the host side of libbwasw_mi355.so; shared types: bsw_internal.h).
 *
 * bsw_reads_upload (bsw_reads.hip) packs every read on the caller's thread and copies a pageable image while the caller sits in
 * the call.  Here the caller's thread only checks the reads, builds the {woff, len} table — all a *_reads_* submit needs for its
 * own checks — and reserves the device copies; the block is then cut into PIECES by raw bytes and every piece is queued once per
 * device on that device's queue (pipeline_submit_job, bsw_batch.hip).  A piece runs on a slot like a CIGAR or rescue chunk: the
 * slot's extension chunk in flight is handed over, the bytes cross PCIe as they lie (registered memory: one DMA of the span;
 * anything else: gathered into the slot's pinned staging), the records {raw offset, woff, len} follow through the slot's pinned
 * h_in, bsw_reads_pack_kernel packs them into that device's copy, and an event is recorded behind it.
 * A chunk that names the block makes its stream wait for those events (reads_order, bsw_internal.h): the order is kept on the
 * GPU, the slot thread only waits until the pieces of its device — which sit ahead of it in the same FIFO queue and wait for
 * nothing — have been enqueued.  The piece then waits for its own work (watchdog), so the slot's staging and the caller's bases
 * are free when it reports; the block is READY when every piece on every device has reported.
 *
 * bsw_reads_upload_start_enc takes the reads as FASTQ letters or as 4-bit words too: the pieces are then cut, spanned, gathered and
 * counted by the RAW bytes of a read as encoded (reads_raw_bytes), and the record tells the kernel which translation to run.
 *
 * An upload is no submit: no ticket, no place among BSW_MAX_INFLIGHT; at most BSW_READS_MAX_UPLOADS per context are in flight.
 */
#include "bsw_f4_host.h"
#include "bsw_reads_pack.h"

#define READS_MAX_WORDS ((1ull << 28) - (1ull << 13))     /* (bsw_reads.hip) */
#define READS_MAX_LEN 65535
#define BSW_READS_MAX_UPLOADS 2
/* raw bytes per piece: the smallest value on the plateau of the sweep in DESIGN.md §9 (profiles/reads_async_rate.json: row c at
 * 64 Ki .. 32 Mi bytes 31.4 / 29.8 / 27.7 / 24.5 / 26.2 / 26.6 / 24.6 / 27.0 / 26.9 / 30.6 ms — level from 512 KiB to 16 MiB).
 * BSW_READS_UP_BYTES replaces it, for tests and measurements only. */
#define READS_UP_BYTES (512u << 10)

static size_t up_piece_bytes()
{
    const char *v = getenv("BSW_READS_UP_BYTES");
    if (v && *v) {
        const long long b = atoll(v);
        if (b > 0) return (size_t)std::min<long long>(b, 1ll << 31);
    }
    return READS_UP_BYTES;
}

static void up_release(bsw_ctx *ctx, bsw_reads *r)
{
    for (size_t d = 0; d < r->d_words.size(); ++d) {
        if (!r->d_words[d] && !(r->up && d < r->up->ev.size())) continue;
        (void)hipSetDevice(ctx->devs[d].device);
        if (r->d_words[d]) (void)hipFree(r->d_words[d]);
        r->d_words[d] = nullptr;
        if (r->up && d < r->up->ev.size())
            for (hipEvent_t &ev : r->up->ev[d]) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    }
    (void)hipSetDevice(ctx->device0());
}

/* piece k of the block on the lane's device: everything up to the event behind the kernel.  *queued: some work of the piece
 * may be on the stream. */
static int up_enqueue(errs &e, f4_lane &L, bsw_reads *r, size_t k, bool *queued)
{
    reads_up &u = *r->up;
    stage_t &st = *L.st;
    hipStream_t s = L.s;
    hipError_t he;
    const size_t a = u.cut[k], b = u.cut[k + 1], n = b - a;
    uint64_t *store = r->d_words[L.dev] + BSW_READS_SLACK;
    if (k == 0) {                                    /* the slack either side of the reads, on the same stream in front of the event */
        *queued = true;
        HIPCHK(e, hipMemsetAsync(r->d_words[L.dev], 0, BSW_READS_SLACK * sizeof(uint64_t), s));
        HIPCHK(e, hipMemsetAsync(store + r->words, 0, BSW_READS_SLACK * sizeof(uint64_t), s));
    }
    raw_span sp;
    for (size_t i = a; i < b; ++i) sp.add(u.src[i], reads_raw_bytes(r->rd[i].len, u.enc));
    if ((he = L.h_in->reserve((n + 1) * sizeof(bsw_rdpack_rec))) != hipSuccess) return fail(e, BSW_E_NOMEM, "pinned staging: %s", hipGetErrorString(he));
    bsw_rdpack_rec *rec = (bsw_rdpack_rec *)L.h_in->p;
    const bool direct = sp.direct(BSW_RDPACK_RAW_SLACK);
    if (!direct && sp.bytes && (he = st.h_raw.reserve((size_t)sp.bytes + BSW_RDPACK_RAW_SLACK)) != hipSuccess)
        return fail(e, BSW_E_NOMEM, "pinned staging: %s", hipGetErrorString(he));
    uint64_t acc = 0;
    for (size_t i = a; i < b; ++i) {
        const int32_t len = r->rd[i].len;
        bsw_rdpack_rec &x = rec[i - a];
        const size_t rb = reads_raw_bytes(len, u.enc);
        x.woff = r->rd[i].woff; x.len = len; x.enc = (uint32_t)u.enc;
        /* (a packed read stays on an 8-byte boundary: its pointer and sp.lo are on one, and a gather adds multiples of 8) */
        x.raw_off = !len ? 0u : direct ? (uint32_t)(u.src[i] - sp.lo) : (uint32_t)acc;
        if (len && !direct) memcpy(st.h_raw.p + acc, u.src[i], rb);
        acc += (uint64_t)rb;
    }
    const size_t rawb = direct ? sp.span() : (size_t)sp.bytes;
    const size_t rec_words = (n * sizeof(bsw_rdpack_rec) + 7) / 8;
    if ((he = st.d_raw.reserve(rawb + BSW_RDPACK_RAW_SLACK)) != hipSuccess || (he = st.d_blob.reserve(rec_words + 2)) != hipSuccess)
        return fail(e, BSW_E_NOMEM, "device staging: %s", hipGetErrorString(he));
    *queued = true;
    if (rawb) {
        HIPCHK(e, hipMemcpyAsync(st.d_raw.p, direct ? sp.lo : st.h_raw.p, rawb, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(st.d_blob.p, rec, n * sizeof(bsw_rdpack_rec), hipMemcpyHostToDevice, s));
        HIPCHK(e, bsw::launch_reads_pack(st.d_raw.p, (const bsw_rdpack_rec *)st.d_blob.p, (uint32_t)n, store, s));
        L.h2d += rawb + n * sizeof(bsw_rdpack_rec);
    }
    HIPCHK(e, hipEventRecord(u.ev[L.dev][k], s));
    return BSW_OK;
}

/* a slot's job (slot_job_fn): piece k on the lane's device */
static void up_piece(bsw_ctx *ctx, f4_lane &L, void *arg, size_t k)
{
    bsw_reads *r = (bsw_reads *)arg;
    reads_up &u = *r->up;
    errs e;
    int rc = BSW_OK;
    bool queued = false;
    if (ctx->dead) rc = fail(e, BSW_E_HIP, "context is dead (an earlier wait for the GPU timed out)");      /* nothing more is queued on a hung device */
    else if (u.failed.load()) rc = fail(e, BSW_E_HIP, "aborted: another piece failed");
    else {
        const hipError_t he = hipSetDevice(ctx->devs[L.dev].device);      /* (the slot set it once; a piece writes another GPU's copy if that did not hold) */
        if (he != hipSuccess) rc = fail(e, BSW_E_HIP, "hipSetDevice: %s", hipGetErrorString(he));
        else rc = up_enqueue(e, L, r, k, &queued);
    }
    auto note = [&](int c, const errs &er) {         /* (u.mu held) the failure itself, not the pieces it made give up */
        const bool real = er.msg.compare(0, 7, "aborted") != 0;
        if (!u.rc || (real && u.err.msg.compare(0, 7, "aborted") == 0)) { u.rc = c; u.err = er; }
    };
    {
        std::lock_guard<std::mutex> lk(u.mu);
        if (rc) { u.failed = 1; note(rc, e); }
        ++u.enq[L.dev];                              /* the chunks that wait for this device's pieces go on (or fail) from here */
        u.cv.notify_all();
    }
    /* the piece's own work: the slot's staging and the caller's bases are free again once it is done; a failing piece drains
     * its stream before it reports */
    if (!rc) rc = sync_stream(ctx, e, L.s, L.ev);
    else if (queued) { errs quiet; (void)sync_stream(ctx, quiet, L.s, L.ev); }
    if (!rc && L.h2d_total) *L.h2d_total += L.h2d;   /* in bsw_host_stats before the block can be seen ready */
    std::lock_guard<std::mutex> lk(u.mu);
    if (rc) { u.failed = 1; note(rc, e); }
    if (--u.left == 0) ctx->uploads.fetch_sub(1);
    u.cv.notify_all();                               /* (under the lock: the block may be freed as soon as it is released) */
}

static int reads_start_any(const char *who, bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int enc, bsw_reads **out)
{
    if (!ctx) return BSW_E_INVAL;
    errs e;
    if (!out || ((!reads || !lens) && n_reads)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: NULL argument", who));
    *out = nullptr;
    if (!reads_enc_known(enc)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: encoding %d is none of BSW_READS_CODES, BSW_READS_ASCII, BSW_READS_PACKED", who, enc));
    if (ctx->dead) return ctx_fail(ctx, e, fail(e, BSW_E_HIP, "%s: context is dead (an earlier wait for the GPU timed out)", who));
    if (n_reads >= (1ull << 32)) return ctx_fail(ctx, e, fail(e, BSW_E_LIMIT, "%s: more than 2^32 - 1 reads", who));
    std::unique_ptr<bsw_reads> r(new bsw_reads());
    r->owner = ctx;
    r->rd.resize(n_reads);
    uint64_t words = 0, bases = 0;
    for (size_t i = 0; i < n_reads; ++i) {
        if (lens[i] < 0) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: read %zu: negative length", who, i));
        if (lens[i] && !reads[i]) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: read %zu: NULL read", who, i));
        if (lens[i] > READS_MAX_LEN) return ctx_fail(ctx, e, fail(e, BSW_E_LIMIT, "%s: read %zu: more than %d bases", who, i, READS_MAX_LEN));
        if (enc == BSW_READS_PACKED && lens[i] && ((uintptr_t)reads[i] & 7)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: read %zu: packed words not on an 8-byte boundary", who, i));
        r->rd[i] = bsw_reads::ent{(uint32_t)words, lens[i]};
        words += nwords(lens[i]);
        bases += (uint64_t)lens[i];
        if (words > READS_MAX_WORDS) return ctx_fail(ctx, e, fail(e, BSW_E_LIMIT, "%s: the block needs more than %llu packed words; split it", who, (unsigned long long)READS_MAX_WORDS));
    }
    r->words = words;
    r->bases = bases;
    const size_t G = ctx->devs.size();
    const size_t total = (size_t)words + 2 * BSW_READS_SLACK;
    r->d_words.assign(G, nullptr);
    if (bases) {                                     /* the pieces: whole reads, up to up_piece_bytes() raw bytes (as encoded) each */
        r->up.reset(new reads_up());
        reads_up &u = *r->up;
        u.src.resize(n_reads);
        for (size_t i = 0; i < n_reads; ++i) u.src[i] = (const uint8_t *)reads[i];
        u.enc = enc;
        const size_t per = up_piece_bytes();
        size_t acc = 0;
        u.cut.push_back(0);
        for (size_t i = 0; i < n_reads; ++i) {
            const size_t rb = reads_raw_bytes(lens[i], enc);
            if (acc && acc + rb > per) { u.cut.push_back(i); acc = 0; }
            acc += rb;
        }
        u.cut.push_back(n_reads);
        u.npieces = u.cut.size() - 1;
        u.enq.assign(G, 0);
        u.ev.assign(G, std::vector<hipEvent_t>(u.npieces, nullptr));
        u.left = G * u.npieces;
        if (ctx->uploads.fetch_add(1) >= BSW_READS_MAX_UPLOADS) {
            ctx->uploads.fetch_sub(1);
            return ctx_fail(ctx, e, fail(e, BSW_E_BUSY, "%s: %d uploads in flight already; wait for one first", who, BSW_READS_MAX_UPLOADS));
        }
    }
    /* the device copies and the events, here in the caller's thread: a failed start leaves none on any device */
    hipError_t he = hipSuccess;
    for (size_t d = 0; d < G && he == hipSuccess; ++d) {
        he = hipSetDevice(ctx->devs[d].device);
        if (he == hipSuccess) he = hipMalloc((void **)&r->d_words[d], total * sizeof(uint64_t));
        if (r->up)
            for (size_t k = 0; k < r->up->npieces && he == hipSuccess; ++k) he = hipEventCreateWithFlags(&r->up->ev[d][k], hipEventDisableTiming);
        else if (he == hipSuccess) {                 /* no base at all: only slack, zeroed now — the block is ready at once */
            hipStream_t up = nullptr;
            he = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
            if (he == hipSuccess) he = hipMemsetAsync(r->d_words[d], 0, total * sizeof(uint64_t), up);
            if (up) {
                const hipError_t se = hipStreamSynchronize(up);
                if (he == hipSuccess) he = se;
                const hipError_t de = hipStreamDestroy(up);
                if (he == hipSuccess) he = de;
            }
        }
    }
    int rc = BSW_OK;
    if (he != hipSuccess) rc = fail(e, BSW_E_HIP, "%s: device allocation: %s", who, hipGetErrorString(he));
    (void)hipSetDevice(ctx->device0());
    if (!rc && r->up) {
        rc = pipeline_submit_job(ctx, up_piece, r.get(), r->up->npieces);
        if (rc) fail(e, rc, "%s: the pipeline could not be started", who);
    }
    if (rc) {
        up_release(ctx, r.get());
        if (r->up) ctx->uploads.fetch_sub(1);
        return ctx_fail(ctx, e, rc);
    }
    *out = r.release();
    return BSW_OK;
}

extern "C" int bsw_reads_upload_start(bsw_ctx *ctx, const uint8_t *const *reads, const int32_t *lens, size_t n_reads, bsw_reads **out)
{
    return reads_start_any("bsw_reads_upload_start", ctx, (const void *const *)reads, lens, n_reads, BSW_READS_CODES, out);
}

extern "C" int bsw_reads_upload_start_enc(bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int encoding, bsw_reads **out)
{
    return reads_start_any("bsw_reads_upload_start_enc", ctx, reads, lens, n_reads, encoding, out);
}

extern "C" int bsw_reads_test(bsw_ctx *ctx, const bsw_reads *rd)
{
    if (!ctx || !rd) return BSW_E_INVAL;
    reads_up *u = rd->up.get();
    if (!u) return 1;
    std::lock_guard<std::mutex> lk(u->mu);
    if (u->left) return 0;
    return u->rc ? u->rc : 1;
}

extern "C" int bsw_reads_wait(bsw_ctx *ctx, bsw_reads *rd)
{
    if (!ctx || !rd) return BSW_E_INVAL;
    reads_up *u = rd->up.get();
    if (!u) return BSW_OK;
    std::unique_lock<std::mutex> lk(u->mu);
    u->cv.wait(lk, [&]() { return u->left == 0; });      /* (every piece waits for the GPU under the watchdog) */
    if (u->rc) return ctx_fail(ctx, u->err, u->rc);
    return BSW_OK;
}

extern "C" int bsw_reads_image(bsw_ctx *ctx, const bsw_reads *rd, int k, uint64_t *words, size_t cap_words)
{
    if (!ctx || !rd) return BSW_E_INVAL;
    errs e;
    const size_t total = (size_t)rd->words + 2 * BSW_READS_SLACK;
    if (rd->owner != ctx) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_reads_image: the read block was uploaded through another context"));
    if (k < 0 || (size_t)k >= rd->d_words.size() || !words || cap_words < total)
        return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_reads_image: device %d of %zu, room for %zu of %zu words", k, rd->d_words.size(), cap_words, total));
    const int st = bsw_reads_test(ctx, rd);
    if (st != 1) return ctx_fail(ctx, e, fail(e, st ? st : BSW_E_BUSY, "bsw_reads_image: the block is not ready (%s)", st ? "its upload failed" : "its upload is in flight"));
    if (ctx->dead) return ctx_fail(ctx, e, fail(e, BSW_E_HIP, "bsw_reads_image: context is dead (an earlier wait for the GPU timed out)"));
    hipError_t he = hipSetDevice(ctx->devs[(size_t)k].device);
    if (he == hipSuccess) he = hipMemcpy(words, rd->d_words[(size_t)k], total * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipSetDevice(ctx->device0());
    if (he != hipSuccess) return ctx_fail(ctx, e, fail(e, BSW_E_HIP, "bsw_reads_image: %s", hipGetErrorString(he)));
    return BSW_OK;
}
