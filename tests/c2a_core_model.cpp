// c2a_core_model.cpp — bsw_c2a_core.h (the device replay's statement of mem_chain2aln's seed loop) under the host compiler with the
// CPU policy, against bsw_chain2aln_replay on the same arrays, byte for byte.  A stand-alone program; tests/test_c2a_device_cpu.py
// builds it with -fsanitize=address,undefined together with bsw_chain2aln.c and bsw_glue.c and runs it
//     c2a_core_model FILE...     every FILE a set written by tests/_c2a_device_gen.py dump()
//     c2a_core_model hand        the hand cases of tests/test_chain2aln_cpu.py restated as data
// A read with a chain above BSW_C2A_DEV_MAX_CHAIN is marked for the host as the chunk function does and must come out empty.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bwa-mem-sw_amd/csrc/bsw_c2a_core.h"

struct set_t {
    bsw_params p;
    bsw_c2a_opt o;
    std::vector<bsw_chain> chains;
    std::vector<bsw_cseed> seeds;
    std::vector<int32_t> lens;
    std::vector<char> results;
    size_t stride = sizeof(bsw_pair);
};

static int fails = 0;
static void check(bool ok, const char *what, const std::string &name)
{
    if (!ok) { ++fails; printf("FAIL %s: %s\n", name.c_str(), what); }
}

// the whole set as ONE chunk through c2a_cpu_launch; the host-route reads are filled in by the host routine, as the chunk function does
static void run_set(const set_t &s, const std::string &name)
{
    const size_t nc = s.chains.size(), ns = s.seeds.size(), nr = s.lens.size();
    std::vector<bsw_creg> want(ns + 1);
    std::vector<uint8_t> wext(ns + 1, 7), gext(ns + 1, 9);
    std::vector<uint64_t> wstart(nr + 1, 0);
    size_t wn = 0;
    const int fmt = s.stride == sizeof(bsw_pair) ? BSW_RESULT_PAIR : BSW_RESULT_FULL;
    const int rc = bsw_chain2aln_replay(&s.p, &s.o, s.chains.data(), nc, s.seeds.data(), ns, s.lens.data(), nr, s.results.data(), fmt, want.data(), &wn,
                                        wext.data(), wstart.data());
    check(rc == BSW_OK, "bsw_chain2aln_replay refused the set", name);
    if (rc || !nc) { printf("%s: %zu seeds, host only\n", name.c_str(), ns); return; }
    std::vector<c2a_dchain> dch(nc);
    std::vector<c2a_dread> drd;
    for (size_t k = 0; k < nc; ++k) {
        const bsw_chain &c = s.chains[k];
        dch[k] = c2a_dchain{(uint32_t)c.first_seed, c.n_seeds, s.lens[c.read], c.rid, c.frac_rep, c.read, (uint32_t)k, 0};
        if (!k || c.read != s.chains[k - 1].read) drd.push_back(c2a_dread{(uint32_t)k, 0, (uint32_t)c.first_seed, 0, 0, 0});
        drd.back().n_chains++;
        drd.back().n_seeds += (uint32_t)c.n_seeds;
        if (c.n_seeds > BSW_C2A_DEV_MAX_CHAIN) drd.back().host = 1;
    }
    std::vector<bsw_creg> stage(ns), out(ns);
    std::vector<uint32_t> counts(drd.size()), offs(drd.size() + 1);
    c2a_dev_args a;
    memset(&a, 0, sizeof(a));
    a.reads = drd.data(); a.n_reads = (uint32_t)drd.size(); a.chains = dch.data(); a.seeds = s.seeds.data(); a.seed_base = 0;
    a.results = s.results.data(); a.stride = (uint32_t)s.stride;
    a.par = c2a_dpar{s.p.mat[0], s.p.o_del, s.p.e_del, s.p.o_ins, s.p.e_ins, s.p.w, s.o.seedlen0_frac, s.o.ovl_len_frac};
    a.stage = stage.data(); a.out = out.data(); a.counts = counts.data(); a.offs = offs.data(); a.flags = gext.data();
    c2a_cpu_launch(&a);
    // the device's reads against the host's, read by read; a host-route read must be empty and its flags cleared
    size_t n_host = 0, at = 0;
    bool same = true;
    for (size_t r = 0; r < drd.size(); ++r) {
        const uint32_t read = dch[drd[r].chain0].read;
        const size_t w0 = (size_t)wstart[read], wcnt = (size_t)(wstart[read + 1] - wstart[read]);
        check(offs[r] == at, "offs[] is not the prefix sum of counts[]", name);
        if (drd[r].host) {
            ++n_host;
            check(counts[r] == 0, "a host-route read has device regions", name);
            for (uint32_t i = 0; i < drd[r].n_seeds; ++i) same &= gext[drd[r].seed0 + i] == 0;
        } else {
            if (counts[r] != wcnt) { same = false; printf("read %u: %u regions, want %zu\n", read, counts[r], wcnt); }
            else {
                same &= memcmp(out.data() + at, want.data() + w0, wcnt * sizeof(bsw_creg)) == 0;
                same &= memcmp(stage.data() + drd[r].seed0, want.data() + w0, wcnt * sizeof(bsw_creg)) == 0;
            }
            same &= memcmp(gext.data() + drd[r].seed0, wext.data() + drd[r].seed0, drd[r].n_seeds) == 0;
        }
        at += counts[r];
    }
    check(offs[drd.size()] == at, "offs[n_reads] is not the total", name);
    check(same, "regions or flags differ from bsw_chain2aln_replay's", name);
    printf("%s: %zu reads (%zu for the host), %zu seeds, %zu regions on the host, %zu on the device\n", name.c_str(), drd.size(), n_host, ns, wn, at);
}

static bool load(const char *path, set_t &s)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int64_t h[4];
    bool ok = fread(h, sizeof(h), 1, f) == 1 && fread(&s.p, sizeof(s.p), 1, f) == 1 && fread(&s.o, sizeof(s.o), 1, f) == 1;
    if (ok) {
        s.chains.resize((size_t)h[0]); s.seeds.resize((size_t)h[1]); s.lens.resize((size_t)h[2]); s.stride = (size_t)h[3];
        s.results.resize(s.seeds.size() * s.stride);
        ok = (!h[0] || fread(s.chains.data(), sizeof(bsw_chain), s.chains.size(), f) == s.chains.size()) &&
             (!h[1] || fread(s.seeds.data(), sizeof(bsw_cseed), s.seeds.size(), f) == s.seeds.size()) &&
             (!h[2] || fread(s.lens.data(), sizeof(int32_t), s.lens.size(), f) == s.lens.size()) &&
             (s.results.empty() || fread(s.results.data(), 1, s.results.size(), f) == s.results.size());
    }
    fclose(f);
    return ok;
}

// ---- hand cases: one read of 200 bases; seed 0 (score 100) is extended first into the region [qb0, qe0) x [rb0, re0) with band w0,
// then the probe seeds are visited.  `want` = the extended flags of seeds 1.. (seed 0 is always extended) ----
struct hseed { int64_t rbeg; int qbeg, len, score; int qb, qe_abs; int64_t rb, re; int w; };     // its record as absolute coordinates
struct hcase { const char *name; double f0, fo; int a, o, e, w; std::vector<hseed> seeds; std::vector<int> n_per_chain; std::vector<int> want; };

static void run_hand(const hcase &h)
{
    set_t s;
    memset(&s.p, 0, sizeof(s.p));                    // (the replay reads the match score, the gap penalties and w alone)
    for (int i = 0; i < 4; ++i) s.p.mat[i * 5 + i] = (int8_t)h.a;
    s.p.o_del = s.p.o_ins = h.o; s.p.e_del = s.p.e_ins = h.e; s.p.w = h.w;
    s.o.seedlen0_frac = h.f0; s.o.ovl_len_frac = h.fo;
    s.lens.assign(1, 200);
    size_t at = 0;
    for (int n : h.n_per_chain) {
        bsw_chain c;
        memset(&c, 0, sizeof(c));
        c.read = 0; c.n_seeds = n; c.first_seed = at; c.rid = 3; c.frac_rep = .25f;
        s.chains.push_back(c);
        at += (size_t)n;
    }
    std::vector<bsw_pair> rec;
    for (const hseed &x : h.seeds) {
        s.seeds.push_back(bsw_cseed{x.rbeg, x.qbeg, x.len, x.score, 0});
        rec.push_back(bsw_pair{(uint32_t)rec.size(), x.qb, x.qe_abs - (x.qbeg + x.len), (int32_t)(x.rb - x.rbeg), (int32_t)(x.re - (x.rbeg + x.len)), 50, 50, x.w});
    }
    s.results.resize(rec.size() * sizeof(bsw_pair));
    memcpy(s.results.data(), rec.data(), s.results.size());
    run_set(s, std::string("hand/") + h.name);
    // what the case is about: the host's own flags are the expected ones (so the data states the case it names)
    std::vector<bsw_creg> regs(s.seeds.size());
    std::vector<uint8_t> ext(s.seeds.size());
    size_t n = 0;
    bsw_chain2aln_replay(&s.p, &s.o, s.chains.data(), s.chains.size(), s.seeds.data(), s.seeds.size(), s.lens.data(), 1, s.results.data(), BSW_RESULT_PAIR, regs.data(), &n,
                         ext.data(), nullptr);
    bool ok = ext[0] == 1;
    for (size_t i = 0; i < h.want.size(); ++i) ok &= ext[i + 1] == h.want[i];
    check(ok, "the case does not state what its name says (flags of the host replay)", std::string("hand/") + h.name);
}

// seed 0: [50, 80) on the query at reference 1050 (diagonal 1000), region [40, 120) x [1040, 1120), band w0.  The probes of the
// explains cases sit in a chain of their own: in seed 0's chain a shifted diagonal would un-skip them.
static hseed big(int w0, int score = 100, int len = 30) { return hseed{1050, 50, len, score, 40, 120, 1040, 1120, w0}; }
static hseed probe(int qbeg, int64_t rbeg, int len, int score) { return hseed{rbeg, qbeg, len, score, qbeg, qbeg + len, rbeg, rbeg + len, 5}; }

static void hand_cases()
{
    const std::vector<hcase> cases = {
        // inside on all four sides: explained, skipped
        {"contained", .1, .95, 1, 6, 1, 100, {big(100), probe(60, 1060, 20, 20)}, {1, 1}, {0}},
        // one base out on each of the four containment sides: not explained
        {"out_query_left", .1, .95, 1, 6, 1, 100, {big(100), probe(39, 1041, 20, 20)}, {1, 1}, {1}},
        {"out_query_right", .1, .95, 1, 6, 1, 100, {big(100), probe(101, 1099, 20, 20)}, {1, 1}, {1}},
        {"out_ref_left", .1, .95, 1, 6, 1, 100, {big(100), probe(41, 1039, 20, 20)}, {1, 1}, {1}},
        {"out_ref_right", .1, .95, 1, 6, 1, 100, {big(100), probe(99, 1101, 20, 20)}, {1, 1}, {1}},
        // seedlen0: len - seedlen0 > .1 * 200 = 20 means "may give a better alignment"; 50 - 30 = 20 is NOT greater (equality), 51 - 30 is
        {"seedlen0_equal", .1, .95, 1, 6, 1, 100, {big(100), probe(45, 1045, 50, 20)}, {1, 1}, {0}},
        {"seedlen0_above", .1, .95, 1, 6, 1, 100, {big(100), probe(45, 1045, 51, 20)}, {1, 1}, {1}},
        {"seedlen0_off", -1., .95, 1, 6, 1, 100, {big(100), probe(45, 1045, 51, 20)}, {1, 1}, {0}},
        // ahead: the seed starts at the region's corner with a shifted diagonal — ahead there is no room (cal_max_gap(0) = 1, |0 - 3| >= 1)
        // but behind it the band takes it; and a seed in the far corner that only the AHEAD side takes
        {"behind_takes_it", .1, .95, 1, 6, 1, 100, {big(100), probe(40, 1043, 20, 20)}, {1, 1}, {0}},
        {"ahead_takes_it", .1, .95, 1, 6, 1, 100, {big(100), probe(100, 1097, 20, 20)}, {1, 1}, {0}},
        // the band bounded by the region's w: diagonal shift 4 under w0 = 5 is inside, under w0 = 4 is not (4 < 4 fails on both sides)
        {"band_w_inside", .1, .95, 1, 6, 1, 100, {big(5), probe(60, 1064, 20, 20)}, {1, 1}, {0}},
        {"band_w_outside", .1, .95, 1, 6, 1, 100, {big(4), probe(60, 1064, 20, 20)}, {1, 1}, {1}},
        // ... or by cal_max_gap: o = 30, e = 5: ahead min(qd, rd) = 20 -> (20 - 30) / 5 + 1 -> 1; behind min(40, 36) = 36 -> (int)2.2 = 2: a shift of 4 is outside,
        // with o = 6, e = 1 it is inside (the first row of this group)
        {"band_gap_outside", .1, .95, 1, 30, 5, 100, {big(100), probe(60, 1064, 20, 20)}, {1, 1}, {1}},
        // ... and by 2 * w of the scoring: w = 2 -> 4: a shift of 4 is outside, a shift of 3 inside
        {"band_2w_outside", .1, .95, 1, 6, 1, 2, {big(100), probe(60, 1064, 20, 20)}, {1, 1}, {1}},
        {"band_2w_inside", .1, .95, 1, 6, 1, 2, {big(100), probe(60, 1063, 20, 20)}, {1, 1}, {0}},
        // un-skip: a chain of its own behind chain 0.  t = [60, 100) len 40 on another diagonal is extended (its reference end leaves the
        // region); s = [70, 110) len 40 on the region's diagonal is explained; the overlap on the query is 30 >= 40 >> 2: un-skipped
        {"unskip", .1, .95, 1, 6, 1, 100, {big(100), probe(60, 1085, 40, 90), probe(70, 1070, 40, 40)}, {1, 2}, {1, 1}},
        // ... the overlap at exactly len >> 2 = 10, and one below
        {"unskip_overlap_equal", .1, .95, 1, 6, 1, 100, {big(100), probe(40, 1065, 40, 90), probe(70, 1070, 40, 40)}, {1, 2}, {1, 1}},
        {"unskip_overlap_below", .1, .95, 1, 6, 1, 100, {big(100), probe(40, 1065, 39, 90), probe(70, 1070, 40, 40)}, {1, 2}, {1, 0}},
        // ... t.len against .95 * s.len with s.len = 40, a multiple of 20: 38 = .95 * 40 is not below it, 37 is
        {"unskip_len_equal", .1, .95, 1, 6, 1, 100, {big(100), probe(75, 1100, 38, 90), probe(70, 1070, 40, 40)}, {1, 2}, {1, 1}},
        {"unskip_len_below", .1, .95, 1, 6, 1, 100, {big(100), probe(75, 1100, 37, 90), probe(70, 1070, 40, 40)}, {1, 2}, {1, 0}},
        // ... a t on the SAME diagonal un-skips nothing
        {"unskip_same_diagonal", .1, .95, 1, 6, 1, 100, {big(100), probe(75, 1075, 40, 90), probe(70, 1070, 40, 40)}, {1, 2}, {0, 0}},
        // score ties: the larger index is visited first — of two equal seeds that explain each other only through the first region made,
        // index 2 is extended and index 1 is then explained by it
        {"score_tie", .1, .95, 1, 6, 1, 100, {hseed{5000, 10, 20, 5, 10, 30, 5000, 5020, 5}, hseed{1050, 50, 30, 50, 40, 120, 1040, 1120, 100}, hseed{1050, 50, 30, 50, 40, 120, 1040, 1120, 100}},
         {3}, {0, 1}},
        // score 0 at index 0: bwa reads its srt[] entry as skipped; it is visited last and extended like any other seed
        {"score0_index0", .1, .95, 1, 6, 1, 100, {hseed{5000, 10, 20, 0, 10, 30, 5000, 5020, 5}, probe(60, 1060, 20, 20), probe(120, 3000, 30, 0)}, {3}, {1, 1}},
    };
    for (const hcase &h : cases) run_hand(h);
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: c2a_core_model hand | FILE...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "hand")) { hand_cases(); continue; }
        set_t s;
        if (!load(argv[i], s)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        run_set(s, argv[i]);
    }
    printf("%s\n", fails ? "FAILED" : "all equal");
    return fails ? 1 : 0;
}
