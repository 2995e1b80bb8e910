// Stand-alone check of bsw_rdpack_word (csrc/bsw_reads_pack.h: the word bsw_reads_pack_kernel computes per lane) against a byte
// loop.  Built by tests/test_reads_pack_model.py with -fsanitize=address,undefined: the raw buffer is allocated with exactly the
// documented slack behind its last byte, so a load that reached further would be reported.  Test infrastructure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../bwa-mem-sw_amd/csrc/bsw_reads_pack.h"

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static long g_words = 0;

// reads of lens[] laid one behind the other from byte `pad` of a buffer that ends 16 bytes behind the last read
static int check_layout(const std::vector<int> &lens, int pad, int mode)
{
    size_t total = (size_t)pad;
    for (int l : lens) total += (size_t)l;
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, total + BSW_RDPACK_RAW_SLACK)) return 1;
    uint8_t *raw = (uint8_t *)mem;
    for (size_t i = 0; i < total; ++i) {
        const uint32_t r = rnd();
        raw[i] = mode == 0 ? (uint8_t)(r % 5) : mode == 1 ? (uint8_t)(i & 255) : (r & 7) ? (uint8_t)(r % 5) : (uint8_t)(r >> 4);
    }
    memset(raw + total, 0xFF, BSW_RDPACK_RAW_SLACK);      // the slack's content must not matter
    size_t off = (size_t)pad;
    int bad = 0;
    for (size_t i = 0; i < lens.size() && !bad; ++i) {
        const int len = lens[i], nw = (len + 15) >> 4;
        for (int k = 0; k <= nw && !bad; ++k) {          // k == nw: behind the read, 0 without a load
            uint64_t want = 0;
            for (int j = 16 * k; j < len && j < 16 * k + 16; ++j) {
                const uint8_t b = raw[off + (size_t)j];
                want |= (uint64_t)(b > 4 ? 4 : b) << (4 * (j & 15));
            }
            const uint64_t got = bsw_rdpack_word(raw, (uint32_t)off, len, k);
            ++g_words;
            if (got != want) {
                fprintf(stderr, "pad %d read %zu len %d word %d: got %016llx want %016llx\n", pad, i, len, k, (unsigned long long)got, (unsigned long long)want);
                bad = 1;
            }
        }
        off += (size_t)len;
    }
    free(mem);
    return bad;
}

int main()
{
    int bad = 0;
    std::vector<int> lens;
    for (int l = 0; l < 50; ++l) lens.push_back(l);
    lens.push_back(65535);
    for (int phase = 0; phase < 16 && !bad; ++phase) {
        for (int len : lens) {
            bad |= check_layout({len}, phase, 2);                  // the first AND the last read of its buffer (phase 0: at byte 0)
            bad |= check_layout({23, len, 9}, phase, 2);           // between two others
            bad |= check_layout({len, 40}, phase, 0);              // the first of two
            bad |= check_layout({40, len}, phase, 0);              // the last of two: its upper load meets the slack
        }
        bad |= check_layout({0, 20, 0, 33, 0}, phase, 2);          // zero-length reads first, in the middle and last
        bad |= check_layout({0}, phase, 2);
        bad |= check_layout({256, 256}, phase, 1);                 // every byte value 0 .. 255
        bad |= check_layout({255}, phase, 1);
    }
    if (bad) return 1;
    printf("ok %ld words\n", g_words);
    return 0;
}
