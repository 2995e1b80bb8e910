// Stand-alone check of bsw_rdpack_word_enc (csrc/bsw_reads_pack.h: the word bsw_reads_pack_kernel computes per lane, for reads that
// lie as codes, as FASTQ letters or as 4-bit words) against per-base loops that restate the upload encodings' contract.  Built by
// tests/test_reads_pack_enc_model.py with -fsanitize=address,undefined: the raw buffer is allocated with exactly the documented
// slack behind its last byte, so a load that reached further would be reported.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../bwa-mem-sw_amd/csrc/bsw_reads_pack.h"

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static long g_words[3] = {0, 0, 0};
static bool g_seen_byte[256], g_seen_nibble[16];

// the contract, per base
static unsigned code_of_letter(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}
static unsigned code_of_code(uint8_t b) { return b > 4 ? 4u : b; }

static int compare(int enc, int pad, size_t i, int len, int k, uint64_t got, uint64_t want)
{
    ++g_words[enc];
    if (got == want) return 0;
    fprintf(stderr, "encoding %d pad %d read %zu len %d word %d: got %016llx want %016llx\n", enc, pad, i, len, k, (unsigned long long)got, (unsigned long long)want);
    return 1;
}

// byte encodings: reads of lens[] one behind the other from byte `pad` of a buffer that ends exactly BSW_RDPACK_RAW_SLACK bytes
// behind the last read; `fill`: 0 random bytes with letters and codes frequent, 1 byte i of the buffer is i & 255
static int check_bytes(int enc, const std::vector<int> &lens, int pad, int fill)
{
    size_t total = (size_t)pad;
    for (int l : lens) total += (size_t)l;
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, total + BSW_RDPACK_RAW_SLACK)) return 1;
    uint8_t *raw = (uint8_t *)mem;
    static const char letters[] = "ACGTacgtNn";
    for (size_t i = 0; i < total; ++i) {
        const uint32_t r = rnd();
        raw[i] = fill == 1 ? (uint8_t)(i & 255) : (r & 3) == 0 ? (uint8_t)(r >> 4) : enc == (int)BSW_RDPACK_ASCII ? (uint8_t)letters[(r >> 4) % 10] : (uint8_t)((r >> 4) % 5);
    }
    for (int j = 0; j < pad; ++j) raw[j] = (uint8_t)(0x80 | rnd());           // garbage in front of the first read ...
    memset(raw + total, 0xFF, BSW_RDPACK_RAW_SLACK);                          // ... and behind the last: the slack's content must not matter
    size_t off = (size_t)pad;
    int bad = 0;
    for (size_t i = 0; i < lens.size() && !bad; ++i) {
        const int len = lens[i], nw = (len + 15) >> 4;
        for (int k = 0; k <= nw && !bad; ++k) {          // k == nw: behind the read, 0 without a load
            uint64_t want = 0;
            for (int j = 16 * k; j < len && j < 16 * k + 16; ++j) {
                const uint8_t b = raw[off + (size_t)j];
                g_seen_byte[b] = true;
                want |= (uint64_t)(enc == (int)BSW_RDPACK_ASCII ? code_of_letter(b) : code_of_code(b)) << (4 * (j & 15));
            }
            bad |= compare(enc, pad, i, len, k, bsw_rdpack_word_enc(raw, (uint32_t)off, len, k, (uint32_t)enc), want);
            if (enc == (int)BSW_RDPACK_CODES && bsw_rdpack_word(raw, (uint32_t)off, len, k) != want) {
                fprintf(stderr, "bsw_rdpack_word differs from encoding 0: pad %d read %zu len %d word %d\n", pad, i, len, k);
                bad = 1;
            }
        }
        off += (size_t)len;
    }
    free(mem);
    return bad;
}

// the packed encoding: reads of lens[] bases, 8 * ceil(len / 16) bytes each, one behind the other from byte `pad` (0 or 8: the two
// halves of a 16-byte line); every nibble value occurs, and the nibbles behind a read's last base are never zero
static int check_packed(const std::vector<int> &lens, int pad)
{
    size_t total = (size_t)pad;
    for (int l : lens) total += 8 * (size_t)((l + 15) >> 4);
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, total + BSW_RDPACK_RAW_SLACK)) return 1;
    uint8_t *raw = (uint8_t *)mem;
    memset(raw, 0xEE, (size_t)pad);
    memset(raw + total, 0xFF, BSW_RDPACK_RAW_SLACK);
    std::vector<std::vector<uint8_t>> nib(lens.size());
    size_t off = (size_t)pad;
    for (size_t i = 0; i < lens.size(); ++i) {
        const int len = lens[i], nw = (len + 15) >> 4;
        nib[i].resize((size_t)nw * 16);
        for (int j = 0; j < nw * 16; ++j) {
            const uint32_t r = rnd();
            uint8_t v = (r & 3) == 0 ? (uint8_t)((r >> 4) & 15) : (uint8_t)((r >> 4) % 5);
            if (j >= len && v == 0) v = 9;                                     // garbage behind the last base
            nib[i][(size_t)j] = v;
        }
        for (int w = 0; w < nw; ++w) {
            uint64_t word = 0;
            for (int j = 0; j < 16; ++j) word |= (uint64_t)nib[i][(size_t)(16 * w + j)] << (4 * j);
            memcpy(raw + off + 8 * (size_t)w, &word, 8);
        }
        off += 8 * (size_t)nw;
    }
    off = (size_t)pad;
    int bad = 0;
    for (size_t i = 0; i < lens.size() && !bad; ++i) {
        const int len = lens[i], nw = (len + 15) >> 4;
        for (int k = 0; k <= nw && !bad; ++k) {
            uint64_t want = 0;
            for (int j = 16 * k; j < len && j < 16 * k + 16; ++j) {
                const uint8_t v = nib[i][(size_t)j];
                g_seen_nibble[v] = true;
                want |= (uint64_t)(v > 4 ? 4 : v) << (4 * (j & 15));
            }
            bad |= compare((int)BSW_RDPACK_PACKED, pad, i, len, k, bsw_rdpack_word_enc(raw, (uint32_t)off, len, k, BSW_RDPACK_PACKED), want);
        }
        off += 8 * (size_t)nw;
    }
    free(mem);
    return bad;
}

int main()
{
    int bad = 0;
    std::vector<int> lens;
    for (int l = 1; l <= 40; ++l) lens.push_back(l);
    lens.push_back(255);
    lens.push_back(256);
    lens.push_back(257);
    for (int enc : {(int)BSW_RDPACK_CODES, (int)BSW_RDPACK_ASCII}) {
        for (int phase = 0; phase < 16 && !bad; ++phase) {
            for (int len : lens) {
                bad |= check_bytes(enc, {len}, phase, 0);                  // the first AND the last read of its buffer
                bad |= check_bytes(enc, {23, len, 9}, phase, 0);           // between two others
                bad |= check_bytes(enc, {40, len}, phase, 0);              // the last of two: its upper load meets the slack
            }
            bad |= check_bytes(enc, {0, 20, 0, 33, 0}, phase, 0);          // zero-length reads first, in the middle and last
            bad |= check_bytes(enc, {256, 256}, phase, 1);                 // every byte value 0 .. 255
            bad |= check_bytes(enc, {255}, phase, 1);
        }
        for (int b = 0; b < 256; ++b)
            if (!g_seen_byte[b]) { fprintf(stderr, "encoding %d: byte value %d never occurred\n", enc, b); bad = 1; }
        memset(g_seen_byte, 0, sizeof(g_seen_byte));
    }
    for (int phase = 0; phase < 16 && !bad; phase += 8) {
        for (int len : lens) {
            bad |= check_packed({len}, phase);
            bad |= check_packed({23, len, 9}, phase);
            bad |= check_packed({40, len}, phase);
            bad |= check_packed({len, 17}, phase);                          // (an odd number of words in front moves the next read to the other half)
        }
        bad |= check_packed({0, 20, 0, 33, 0}, phase);
    }
    for (int v = 0; v < 16; ++v)
        if (!g_seen_nibble[v]) { fprintf(stderr, "nibble value %d never occurred\n", v); bad = 1; }
    if (bad) return 1;
    printf("ok %ld %ld %ld words\n", g_words[0], g_words[1], g_words[2]);
    return 0;
}
