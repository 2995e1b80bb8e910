/* reads_fetch_model.cpp — bsw_reads_word() of csrc/bsw_reads_fetch.h, the very function bsw_pack_kernel inlines, compiled by
 * g++ for tests/test_reads_fetch_model.py (TEST INFRASTRUCTURE).  The store is built as bsw_reads_upload builds it — slack
 * words, every read on a word boundary, codes > 4 stored as 4 — by a plain nibble loop, not by the library. */
#include "../bwa-mem-sw_amd/csrc/bsw_reads_fetch.h"

#include <vector>

extern "C" {

int reads_model_slack(void) { return BSW_READS_SLACK; }

/* pack reads (back to back in `bases`, lens[n]) into img (slack + words + slack, zeroed by the caller); woff[n] receives the word
 * offsets; returns the words the reads take */
long reads_model_pack(const uint8_t *bases, const int *lens, int n, uint64_t *img, uint32_t *woff)
{
    uint64_t *store = img + BSW_READS_SLACK;
    long words = 0;
    for (int i = 0; i < n; ++i) {
        woff[i] = (uint32_t)words;
        for (int k = 0; k < lens[i]; ++k) {
            const uint64_t c = bases[k] > 4 ? 4 : bases[k];
            store[words + (k >> 4)] |= c << (4 * (k & 15));
        }
        bases += lens[i];
        words += (lens[i] + 15) >> 4;
    }
    return words;
}

/* out[0 .. (L + 15) / 16) = the words of the sequence of L bases at position s, forwards or backwards */
void reads_model_fetch(const uint64_t *img, uint32_t s, int backwards, int L, uint64_t *out)
{
    for (int k = 0; 16 * k < L; ++k) out[k] = bsw_reads_word(img + BSW_READS_SLACK, s, backwards, L, k);
}
}
