/*
 * bsw_reads.hip — the resident read store: bsw_reads_upload / bsw_reads_free / bsw_reads_info (part of the host side of
 * libbwasw_mi355.so; shared types: bsw_internal.h).
 *
 * A read block is packed once on the host into the device sequence format (4 bits per base, every read on a word boundary,
 * BSW_READS_SLACK zeroed words in front and behind) and copied to every device of the context, as bsw_ref_upload copies the pac.
 * The three *_reads_* submits live with their pointer forms (bsw_batch.hip, bsw_matesw.hip, bsw_cigar.hip) and read the block
 * as plain data; bsw_pack_kernel fetches the query words from it (bsw_reads_fetch.h).
 *
 * bsw_reads_upload is the SYNCHRONOUS form: the caller sits in it while one host thread packs and a pageable image is copied.
 * bsw_reads_upload_start (bsw_reads_async.hip) is the asynchronous one: it returns at once, the reads cross PCIe as they lie,
 * bsw_reads_pack_kernel packs them on every GPU, and tickets that name the block are ordered behind that on the device.  Both
 * make the same image, and bsw_reads_free / bsw_reads_info here serve both.  The _enc forms of both take the reads as FASTQ
 * letters or as 4-bit words too (BSW_READS_ASCII / BSW_READS_PACKED): the image is the one the codes those spell would give.
 *
 * These calls may run while tickets are in flight and from several threads: they use no state of the context but its device
 * list and its error text (under its lock), and the upload copies on a stream of its own per device.
 */
#include "bsw_internal.h"
#include "bsw_reads_pack.h"                      /* (bsw_rdpack_clamp_nibbles) */

/* positions are 32 bits: 16 * words + the longest read must stay below 2^32 */
#define READS_MAX_WORDS ((1ull << 28) - (1ull << 13))
#define READS_MAX_LEN 65535

static void reads_release_devices(bsw_ctx *ctx, bsw_reads *r)
{
    for (size_t d = 0; d < r->d_words.size(); ++d) {
        if (!r->d_words[d]) continue;
        (void)hipSetDevice(ctx->devs[d].device);
        (void)hipFree(r->d_words[d]);
        r->d_words[d] = nullptr;
    }
    if (r->up)                                       /* (after a failed upload too: what there is) */
        for (size_t d = 0; d < r->up->ev.size(); ++d) {
            (void)hipSetDevice(ctx->devs[d].device);
            for (hipEvent_t &ev : r->up->ev[d]) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
        }
    (void)hipSetDevice(ctx->device0());
}

/* the image of one read: words[0 .. nwords(len)) */
static void reads_pack_one(const void *read, int32_t len, int enc, std::vector<uint8_t> &codes, uint64_t *words)
{
    if (enc == BSW_READS_PACKED) {                   /* clamp and mask: nibbles above 4 become 4, those behind the last base zero */
        const uint64_t *src = (const uint64_t *)read;
        const size_t nw = nwords(len);
        for (size_t k = 0; k < nw; ++k) words[k] = bsw_rdpack_clamp_nibbles(src[k]);
        if (len & 15) words[nw - 1] &= (1ull << (4 * (len & 15))) - 1ull;
        return;
    }
    const uint8_t *b = (const uint8_t *)read;
    if (enc == BSW_READS_ASCII) {                    /* translate, then pack like codes */
        static const struct lut { uint8_t c[256]; lut() { memset(c, 4, sizeof(c)); c['A'] = c['a'] = 0; c['C'] = c['c'] = 1; c['G'] = c['g'] = 2; c['T'] = c['t'] = 3; } } L;
        codes.resize((size_t)len);
        for (int32_t j = 0; j < len; ++j) codes[(size_t)j] = L.c[b[j]];
        b = codes.data();
    }
    (void)bsw_pack_bases(b, len, words);
}

static int reads_upload_any(const char *who, bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int enc, bsw_reads **out)
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
    /* the device image: slack | reads | slack, packed here once for all devices */
    const size_t total = (size_t)words + 2 * BSW_READS_SLACK;
    std::vector<uint64_t> img;
    try { img.assign(total, 0ull); } catch (const std::bad_alloc &) { return ctx_fail(ctx, e, fail(e, BSW_E_NOMEM, "%s: %zu bytes of host memory", who, total * 8)); }
    std::vector<uint8_t> codes;
    for (size_t i = 0; i < n_reads; ++i)
        if (lens[i]) reads_pack_one(reads[i], lens[i], enc, codes, img.data() + BSW_READS_SLACK + r->rd[i].woff);
    r->d_words.assign(ctx->devs.size(), nullptr);
    for (size_t d = 0; d < ctx->devs.size(); ++d) {               /* every GPU of the context keeps its own copy */
        hipStream_t up = nullptr;
        hipError_t he = hipSetDevice(ctx->devs[d].device);
        if (he == hipSuccess) he = hipMalloc((void **)&r->d_words[d], total * sizeof(uint64_t));
        if (he == hipSuccess) he = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
        if (he == hipSuccess) he = hipMemcpyAsync(r->d_words[d], img.data(), total * sizeof(uint64_t), hipMemcpyHostToDevice, up);
        if (up) {
            const hipError_t se = hipStreamSynchronize(up);      /* (also behind a failed copy: img is ours until nothing reads it) */
            if (he == hipSuccess) he = se;
            const hipError_t de = hipStreamDestroy(up);
            if (he == hipSuccess) he = de;
        }
        if (he != hipSuccess) {
            reads_release_devices(ctx, r.get());                 /* a failed upload leaves no copy on any device */
            return ctx_fail(ctx, e, fail(e, BSW_E_HIP, "read block upload to device %d: %s", ctx->devs[d].device, hipGetErrorString(he)));
        }
    }
    (void)hipSetDevice(ctx->device0());
    *out = r.release();
    return BSW_OK;
}

extern "C" int bsw_reads_upload(bsw_ctx *ctx, const uint8_t *const *reads, const int32_t *lens, size_t n_reads, bsw_reads **out)
{
    return reads_upload_any("bsw_reads_upload", ctx, (const void *const *)reads, lens, n_reads, BSW_READS_CODES, out);
}

extern "C" int bsw_reads_upload_enc(bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int encoding, bsw_reads **out)
{
    return reads_upload_any("bsw_reads_upload_enc", ctx, reads, lens, n_reads, encoding, out);
}

extern "C" int bsw_reads_free(bsw_ctx *ctx, bsw_reads *rd)
{
    if (!rd) return BSW_OK;
    if (!ctx) return BSW_E_INVAL;
    errs e;
    if (rd->owner != ctx) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_reads_free: the read block was uploaded through another context"));
    if (rd->up) {                                    /* bsw_reads_upload_start: its pieces read and write the block until the last one has reported */
        std::lock_guard<std::mutex> lk(rd->up->mu);
        if (rd->up->left) return ctx_fail(ctx, e, fail(e, BSW_E_BUSY, "bsw_reads_free: the upload of the block is still in flight"));
    }
    int none = 0;
    if (!rd->users.compare_exchange_strong(none, -1))
        return ctx_fail(ctx, e, fail(e, BSW_E_BUSY, "bsw_reads_free: %d ticket(s) that use the block have not been collected", none));
    reads_release_devices(ctx, rd);
    delete rd;
    return BSW_OK;
}

extern "C" int bsw_reads_info(const bsw_reads *rd, uint64_t *n_reads, uint64_t *bases, uint64_t *device_bytes)
{
    if (!rd) return BSW_E_INVAL;
    if (n_reads) *n_reads = rd->rd.size();
    if (bases) *bases = rd->bases;
    if (device_bytes) *device_bytes = (rd->words + 2 * BSW_READS_SLACK) * sizeof(uint64_t);
    return BSW_OK;
}
