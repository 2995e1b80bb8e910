/* host_reads_enc.cpp — the upload encodings of a resident read block (bsw_reads_upload_enc / bsw_reads_upload_start_enc:
 * bsw_reads.hip, bsw_reads_async.hip) on the host-memory HIP stand-in, under ASan / UBSan or TSan (TEST INFRASTRUCTURE;
 * tests/test_reads_enc_double_cpu.py builds it with its row in tests/_host_double_build.py and runs it).
 *
 *   host_reads_enc parity      codes, letters and words; reads in one registered arena (direct) and in pageable memory (gathered);
 *                              one device and the same ordinal twice; 4 KiB pieces: every device's image of the _start_enc upload
 *                              equals the image of bsw_reads_upload_enc and the image of bsw_reads_upload of the codes the input
 *                              spells; on the gather path bsw_host_stats.h2d_bytes grows per device by raw bytes + 16 per read
 *   host_reads_enc refusals    an unknown encoding, a packed read off its 8-byte boundary, and the per-read checks under every
 *                              encoding: the codes of the existing calls, no allocation, no launch
 *   host_reads_enc faults      the first failure of each kind of HIP call of both uploads, under every encoding
 *
 * The launcher is launchers_reads_pack_enc.cpp: the word function restated per base, honouring every record's encoding. */
#include <algorithm>
#include <string>
#include "host_common.h"

namespace standin_rdpack {
uint64_t launches();
uint64_t reads();
uint64_t reads_of(int enc);
void reset();
}

static const int ENCS[3] = {BSW_READS_CODES, BSW_READS_ASCII, BSW_READS_PACKED};
static const char *ENC_NAME[3] = {"codes", "letters", "words"};

/* this program's own generator: its stream defines the blocks, which the splitmix rng_t of host_common.h would change */
struct xorshift_t {
    uint64_t s;
    explicit xorshift_t(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    uint32_t below(uint32_t n) { return next() % n; }
};

static uint8_t code_of_letter(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

/* a block under one encoding: the raw units of every read (with garbage behind a packed read's last base), the codes they spell, and
 * the reads once more inside ONE registered arena with small gaps */
struct enc_block {
    int enc = 0;
    std::vector<int32_t> len;
    std::vector<std::vector<uint64_t>> store;        /* a read's raw bytes, in 8-byte units (a packed read must start on one) */
    std::vector<std::vector<uint8_t>> codes;
    std::vector<const void *> ptr, ptr_arena;
    std::vector<const uint8_t *> code_ptr;
    uint8_t *arena = nullptr;
    uint64_t raw_bytes = 0;
    size_t rawb(size_t i) const { return enc == BSW_READS_PACKED ? 8 * (size_t)((len[i] + 15) >> 4) : (size_t)len[i]; }
    void make(int e, const std::vector<int32_t> &lens, uint64_t seed)
    {
        enc = e;
        len = lens;
        xorshift_t r(seed);
        static const char letters[] = "ACGTacgtNnRYKMUu-.*";
        size_t arena_len = 64;
        for (size_t i = 0; i < len.size(); ++i) {
            const int L = len[i];
            std::vector<uint8_t> c((size_t)L), raw(rawb(i) + 8, 0);
            for (int j = 0; j < L; ++j) {
                const uint32_t x = r.next();
                if (enc == BSW_READS_CODES) { const uint8_t b = (x & 31) ? (uint8_t)((x >> 8) % 5) : (uint8_t)(x >> 8); raw[(size_t)j] = b; c[(size_t)j] = b > 4 ? 4 : b; }
                else if (enc == BSW_READS_ASCII) { const uint8_t b = (x & 15) ? (uint8_t)letters[(x >> 8) % (sizeof(letters) - 1)] : (uint8_t)(x >> 8); raw[(size_t)j] = b; c[(size_t)j] = code_of_letter(b); }
                else { const uint8_t v = (x & 15) ? (uint8_t)((x >> 8) % 5) : (uint8_t)((x >> 8) & 15); raw[(size_t)(j >> 1)] |= (uint8_t)(v << (4 * (j & 1))); c[(size_t)j] = v > 4 ? 4 : v; }
            }
            if (enc == BSW_READS_PACKED)
                for (int j = L; j < 16 * ((L + 15) >> 4); ++j) raw[(size_t)(j >> 1)] |= (uint8_t)((5 + r.below(11)) << (4 * (j & 1)));      /* garbage behind the last base */
            std::vector<uint64_t> units((rawb(i) + 7) / 8);
            if (!units.empty()) memcpy(units.data(), raw.data(), rawb(i));
            store.push_back(units);
            codes.push_back(c);
            raw_bytes += rawb(i);
            arena_len += rawb(i) + 24;
        }
        arena = (uint8_t *)bsw_host_alloc(arena_len);
        CHECK(arena, "bsw_host_alloc");
        memset(arena, 0xA7, arena_len);
        size_t off = enc == BSW_READS_PACKED ? 8 : 5;
        for (size_t i = 0; i < len.size(); ++i) {
            ptr.push_back(len[i] ? store[i].data() : nullptr);
            code_ptr.push_back(len[i] ? codes[i].data() : nullptr);
            if (len[i]) memcpy(arena + off, store[i].data(), rawb(i));
            ptr_arena.push_back(len[i] ? arena + off : nullptr);
            off += rawb(i) + (enc == BSW_READS_PACKED ? 8 * (i % 3) : i % 4);      /* (packed: both halves of a 16-byte line) */
        }
    }
    ~enc_block() { if (arena) bsw_host_free(arena); }
};

static std::vector<int32_t> block_lens()
{
    std::vector<int32_t> l = {0};
    xorshift_t r(17);
    for (int rep = 0; rep < 3; ++rep) {
        for (int n : {1, 15, 16, 17, 31, 32, 33, 150, 250, 255, 256, 257, 513, 1000}) l.push_back(n);
        for (int k = 0; k < 12; ++k) l.push_back(1 + (int32_t)r.below(300));
        if (rep == 1) { l.push_back(0); l.push_back(0); }
    }
    for (int k = 0; k < 16; ++k) l.push_back(17);      /* back to back: every byte phase, both word parities */
    l.push_back(0);
    return l;
}

static std::vector<uint64_t> image(bsw_ctx *ctx, const bsw_reads *rd, int k)
{
    uint64_t db = 0;
    CHECK(bsw_reads_info(rd, nullptr, nullptr, &db) == BSW_OK, "bsw_reads_info");
    std::vector<uint64_t> w(db / 8 + 1, 0x5a5a5a5a5a5a5a5aull);
    const int rc = bsw_reads_image(ctx, rd, k, w.data(), db / 8);
    CHECK(rc == BSW_OK, "bsw_reads_image of device %d -> %d (%s)", k, rc, bsw_last_error(ctx));
    CHECK(w.back() == 0x5a5a5a5a5a5a5a5aull, "bsw_reads_image wrote behind the image");
    w.pop_back();
    return w;
}

static int parity_mode()
{
    const std::vector<int32_t> lens = block_lens();
    const size_t n = lens.size();
    size_t cases = 0;
    uint64_t pieces = 0;
    setenv("BSW_READS_UP_BYTES", "4096", 1);
    for (int G : {1, 2}) {
        for (int e = 0; e < 3; ++e) {
            fresh(1);
            {
                enc_block B;
                B.make(ENCS[e], lens, 100 + (uint64_t)e);
                const int same[2] = {0, 0};              /* the same ordinal twice: two copies on one device */
                for (int direct = 0; direct < 2; ++direct) {
                    standin::reset();
                    standin_rdpack::reset();
                    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, G, 256, 2, 20000, same);
                    const void *const *P = direct ? B.ptr_arena.data() : B.ptr.data();
                    bsw_reads *rd = nullptr;
                    CHECK(bsw_reads_upload(ctx, B.code_ptr.data(), lens.data(), n, &rd) == BSW_OK && rd, "bsw_reads_upload: %s", bsw_last_error(ctx));
                    const std::vector<uint64_t> want = image(ctx, rd, 0);
                    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free");
                    CHECK(bsw_reads_upload_enc(ctx, P, lens.data(), n, ENCS[e], &rd) == BSW_OK && rd, "bsw_reads_upload_enc: %s", bsw_last_error(ctx));
                    CHECK(bsw_reads_test(ctx, rd) == 1, "a block of bsw_reads_upload_enc is ready");
                    for (int k = 0; k < G; ++k) CHECK(image(ctx, rd, k) == want, "%s, %s: device %d's copy by bsw_reads_upload_enc differs from bsw_reads_upload of the codes", ENC_NAME[e], direct ? "direct" : "gather", k);
                    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free");
                    CHECK(standin_rdpack::launches() == 0, "a synchronous upload launched the pack kernel");
                    const uint64_t h0 = stats_of(ctx).h2d_bytes;
                    CHECK(bsw_reads_upload_start_enc(ctx, P, lens.data(), n, ENCS[e], &rd) == BSW_OK && rd, "bsw_reads_upload_start_enc: %s", bsw_last_error(ctx));
                    CHECK(bsw_inflight(ctx) == 0, "an upload counts as a submit");
                    CHECK(bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_test(ctx, rd) == 1, "bsw_reads_wait: %s", bsw_last_error(ctx));
                    for (int k = 0; k < G; ++k) {
                        const std::vector<uint64_t> got = image(ctx, rd, k);
                        CHECK(got.size() == want.size(), "image sizes");
                        for (size_t i = 0; i < got.size(); ++i)
                            CHECK(got[i] == want[i], "%s, %d copies, %s: word %zu of copy %d is %016llx, bsw_reads_upload of the codes makes %016llx", ENC_NAME[e], G, direct ? "direct" : "gather", i, k,
                                  (unsigned long long)got[i], (unsigned long long)want[i]);
                    }
                    const uint64_t grew = stats_of(ctx).h2d_bytes - h0;
                    if (!direct) CHECK(grew == (uint64_t)G * (B.raw_bytes + 16 * n), "%s gathered: h2d_bytes grew by %llu, %d x (%llu raw bytes + 16 x %zu reads) expected", ENC_NAME[e],
                                       (unsigned long long)grew, G, (unsigned long long)B.raw_bytes, n);
                    else CHECK(grew >= (uint64_t)G * (B.raw_bytes + 16 * n), "%s direct: h2d_bytes grew by %llu", ENC_NAME[e], (unsigned long long)grew);
                    const uint64_t per_dev = standin_rdpack::launches() / (uint64_t)G;
                    CHECK(standin_rdpack::launches() == per_dev * (uint64_t)G && per_dev >= 2, "%llu pack launches for %d copies of %llu raw bytes in 4 KiB pieces", (unsigned long long)standin_rdpack::launches(), G, (unsigned long long)B.raw_bytes);
                    CHECK(standin_rdpack::reads_of(ENCS[e]) == (uint64_t)G * n && standin_rdpack::reads() == (uint64_t)G * n, "records of another encoding reached the launcher");
                    pieces += standin_rdpack::launches();
                    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free: %s", bsw_last_error(ctx));
                    bsw_destroy(ctx);
                    CHECK(hipdbl::live_objects() == 1, "%zu HIP objects left alive", hipdbl::live_objects());      /* (the registered arena) */
                    ++cases;
                }
            }
            CHECK(hipdbl::live_objects() == 0, "parity: %zu HIP objects left", hipdbl::live_objects());
        }
    }
    printf("parity: %zu cases, %llu pieces\n", cases, (unsigned long long)pieces);
    return 0;
}

typedef int (*upload_fn)(bsw_ctx *, const void *const *, const int32_t *, size_t, int, bsw_reads **);

static int refusals_mode()
{
    fresh(1);
    size_t refused = 0;
    {
        alignas(16) static uint64_t words[64];
        const uint8_t *bytes = (const uint8_t *)words;
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2);
        bsw_reads *rd = nullptr;
        const void *p1[1] = {bytes};
        const int32_t l1[1] = {150};
        CHECK(bsw_reads_upload_start_enc(ctx, p1, l1, 1, BSW_READS_ASCII, &rd) == BSW_OK && bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK, "a first upload");
        const upload_fn fns[2] = {bsw_reads_upload_enc, bsw_reads_upload_start_enc};
        const char *names[2] = {"bsw_reads_upload_enc", "bsw_reads_upload_start_enc"};
        for (int f = 0; f < 2; ++f) {
            const size_t live = hipdbl::live_objects();
            const uint64_t launches = standin_rdpack::launches(), h2d = stats_of(ctx).h2d_bytes;
            hipdbl::reset_counters();
            auto refuse = [&](const void *const *P, const int32_t *L, size_t n, int enc, int want, const char *text) {
                bsw_reads *out = (bsw_reads *)16;
                const int rc = fns[f](ctx, P, L, n, enc, &out);
                CHECK(rc == want && !out, "%s (encoding %d): %d where %d is expected", names[f], enc, rc, want);
                CHECK(strstr(bsw_last_error(ctx), names[f]) && strstr(bsw_last_error(ctx), text), "%s: the text \"%s\" lacks \"%s\"", names[f], bsw_last_error(ctx), text);
                ++refused;
            };
            for (int enc : {3, -1, 1 << 20}) refuse(p1, l1, 1, enc, BSW_E_INVAL, "encoding");
            for (int shift : {1, 2, 4, 7, 12}) {
                const void *P[3] = {bytes, nullptr, bytes + shift};
                const int32_t L[3] = {150, 0, 40};
                refuse(P, L, 3, BSW_READS_PACKED, BSW_E_INVAL, "read 2");
            }
            for (int enc : ENCS) {
                const void *P[2] = {bytes, nullptr};
                const int32_t L[2] = {10, 5};
                refuse(P, L, 2, enc, BSW_E_INVAL, "read 1: NULL read");
                const void *Q[2] = {bytes, bytes};
                const int32_t M[2] = {10, -1};
                refuse(Q, M, 2, enc, BSW_E_INVAL, "read 1: negative length");
                const int32_t big[1] = {65536};
                refuse(Q, big, 1, enc, BSW_E_LIMIT, "read 0: more than 65535 bases");
                std::vector<const void *> many(66000, bytes);
                std::vector<int32_t> ml(66000, 65535);                      /* 66 000 x 4 096 words > 2^28 - 2^13: refused before any base is read */
                refuse(many.data(), ml.data(), many.size(), enc, BSW_E_LIMIT, "split it");
                bsw_reads *out = (bsw_reads *)16;
                CHECK(fns[f](ctx, nullptr, l1, 1, enc, &out) == BSW_E_INVAL, "NULL reads[]");
                CHECK(fns[f](ctx, p1, l1, 1, enc, nullptr) == BSW_E_INVAL, "NULL out");
            }
            CHECK(hipdbl::live_objects() == live, "%s: a refusal allocated something", names[f]);
            CHECK(hipdbl::calls("hipMalloc") == 0 && hipdbl::calls("hipMemcpyAsync") == 0 && hipdbl::calls("hipEventCreateWithFlags") == 0, "%s: a refusal called the runtime", names[f]);
            CHECK(standin_rdpack::launches() == launches && stats_of(ctx).h2d_bytes == h2d, "%s: a refusal queued something", names[f]);
            /* a read without a base need not keep the boundary, and the context goes on */
            const void *P[2] = {bytes + 8, bytes + 3};
            const int32_t L[2] = {100, 0};
            CHECK(fns[f](ctx, P, L, 2, BSW_READS_PACKED, &rd) == BSW_OK && rd && bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK, "%s after the refusals: %s", names[f], bsw_last_error(ctx));
        }
        CHECK(bsw_inflight(ctx) == 0, "bsw_inflight");
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "refusals: %zu HIP objects left", hipdbl::live_objects());
    printf("refusals: ok, %zu\n", refused);
    return 0;
}

static int faults_mode()
{
    const std::vector<int32_t> lens = block_lens();
    const size_t n = lens.size();
    size_t failed = 0;
    setenv("BSW_READS_UP_BYTES", "4096", 1);
    for (int e = 0; e < 3; ++e) {
        fresh(1);
        {
            enc_block B;
            B.make(ENCS[e], lens, 300 + (uint64_t)e);
            /* the asynchronous upload: the first call of each kind on a piece's way fails -> the upload fails, the block can be
             * freed, nothing is left; a failing reservation in the start itself makes no block */
            for (const char *who : {"launch_reads_pack", "hipMemcpyAsync", "hipMemsetAsync", "hipMalloc", "hipEventCreateWithFlags"}) {
                for (int direct = 0; direct < 2; ++direct) {
                    standin::reset();
                    standin_rdpack::reset();
                    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 128, 2, 4000);
                    hipdbl::reset_counters();
                    const bool in_start = !strcmp(who, "hipMalloc") || !strcmp(who, "hipEventCreateWithFlags");
                    hipdbl::fail_named(who, 1);
                    bsw_reads *rd = (bsw_reads *)16;
                    const int rs = bsw_reads_upload_start_enc(ctx, direct ? B.ptr_arena.data() : B.ptr.data(), lens.data(), n, ENCS[e], &rd);
                    if (in_start) {
                        CHECK(rs == BSW_E_HIP && !rd, "%s fails in the start (%s) and it answers %d", who, ENC_NAME[e], rs);
                        hipdbl::clear_failures();
                    } else {
                        CHECK(rs == BSW_OK && rd, "bsw_reads_upload_start_enc -> %d (%s)", rs, bsw_last_error(ctx));
                        const int rw = bsw_reads_wait(ctx, rd);
                        CHECK(hipdbl::fired(), "%s never failed (%s)", who, ENC_NAME[e]);
                        hipdbl::clear_failures();
                        CHECK(rw == BSW_E_HIP && bsw_reads_test(ctx, rd) == BSW_E_HIP, "%s fails (%s) and bsw_reads_wait -> %d", who, ENC_NAME[e], rw);
                        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free after a failed upload: %s", bsw_last_error(ctx));
                    }
                    ++failed;
                    /* the context goes on: the same upload, clean */
                    CHECK(bsw_reads_upload_start_enc(ctx, B.ptr.data(), lens.data(), n, ENCS[e], &rd) == BSW_OK && bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK,
                          "the clean rerun behind %s: %s", who, bsw_last_error(ctx));
                    bsw_destroy(ctx);
                    CHECK(hipdbl::live_objects() == 1, "%s (%s): %zu HIP objects left alive", who, ENC_NAME[e], hipdbl::live_objects());
                }
            }
            /* the synchronous upload */
            for (const char *who : {"hipMalloc", "hipStreamCreateWithFlags", "hipMemcpyAsync", "hipStreamSynchronize"}) {
                const int same[2] = {0, 0};
                for (uint64_t k = 1; k <= 2; ++k) {                       /* on the first and on the second copy */
                    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 128, 2, 4000, same);
                    hipdbl::reset_counters();
                    hipdbl::fail_named(who, k);
                    bsw_reads *rd = (bsw_reads *)16;
                    const int rs = bsw_reads_upload_enc(ctx, B.ptr.data(), lens.data(), n, ENCS[e], &rd);
                    CHECK(hipdbl::fired(), "%s never failed", who);
                    hipdbl::clear_failures();
                    CHECK(rs == BSW_E_HIP && !rd, "%s fails in bsw_reads_upload_enc (%s) and it answers %d", who, ENC_NAME[e], rs);
                    ++failed;
                    CHECK(bsw_reads_upload_enc(ctx, B.ptr.data(), lens.data(), n, ENCS[e], &rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK, "the clean rerun behind %s", who);
                    bsw_destroy(ctx);
                    CHECK(hipdbl::live_objects() == 1, "%s (%s, synchronous): %zu HIP objects left alive", who, ENC_NAME[e], hipdbl::live_objects());
                }
            }
        }
        CHECK(hipdbl::live_objects() == 0, "faults: %zu HIP objects left", hipdbl::live_objects());
    }
    printf("faults: ok, %zu\n", failed);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "parity") return parity_mode();
    if (mode == "refusals") return refusals_mode();
    if (mode == "faults") return faults_mode();
    fprintf(stderr, "usage: host_reads_enc parity | refusals | faults\n");
    return 2;
}
