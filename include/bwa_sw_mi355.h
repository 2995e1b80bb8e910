/*
 * bwa_sw_mi355.h — C ABI of libbwasw_mi355.so
 *
 * MI355X (gfx950) implementation of BWA-MEM's banded affine-gap Smith-Waterman
 * seed-extension path: ksw_extend / ksw_extend2 as driven by mem_chain2aln
 * (left extension, right extension, MAX_BAND_TRY band doubling, clip-vs-extend
 * decision).  Every entry point below computes on the GPU through hand-written
 * HIP kernels; there is NO CPU fallback in this library.  If no gfx950 device
 * (or no usable HIP runtime) is present the calls fail with BSW_E_NODEVICE.
 *
 * What each entry point replaces in the reference (peterpengwei/bwa-mem-sw,
 * FPGA RTL; citations are into that tree):
 *
 *   ksw_extend2 / ksw_extend   the software ABI the accelerator stands in for
 *                              (bwa ksw.h; hardware statement of it:
 *                              sw_pe_array_sw_extend.v:96-123 ports,
 *                              :1639-1705 FSM)
 *   bsw_params                 batch-global words G0/G1
 *                              (sw_pe_array_proc_element.v:816-819, :916-917)
 *   bsw_task                   8-word task header H0..H7 + packed bases
 *                              (sw_pe_array_task_parse.v:1884-1951,
 *                               sw_pe_array_proc_element.v:807-933, :1638-1683)
 *   bsw_result                 5-word result record R0..R4
 *                              (sw_pe_array_proc_element.v:1662-1665, :1190-1199)
 *   bsw_create/.../bsw_wait    CSR + DSM handshake and the TBB/RBB round trip
 *                              (batch_manager.v:208-221, :358-739; tbb.v; rbb.v)
 *   bsw_refbatch_*             the exact 256 KiB task batch / 16 KiB result
 *                              batch wire format (bwa_mem_sw.v:163-170)
 *   bsw_cigar_ref_batch        bwa_gen_cigar2 (+ mem_reg2aln's retries) against the
 *                              device-resident reference: score, CIGAR, NM, MD
 *                              (bwa host software, not the RTL)
 *   bsw_matesw_ref_batch       mem_matesw's ksw_align2 against the device-resident
 *                              reference (bwa host software, not the RTL)
 *   bsw_patch_ref_batch        mem_patch_reg (mem_sort_dedup_patch, bwa >= 0.7.10) against the
 *                              device-resident reference: the score of bwa_gen_cigar2 without a
 *                              CIGAR, and the tests around it (bwa host software, not the RTL)
 *   bsw_chain2aln_*_start,     mem_chain2aln's driver around ksw_extend2 (bwa 0.7.12 - 0.7.17, as recalled): which seeds of a chain
 *   bsw_chain2aln_finish       are extended, in which order, and the regions with seedcov / seedlen0 / rid / frac_rep; every seed
 *                              is extended as one job of the pipeline, bwa's loop is replayed on the host (bwa host software)
 *   bsw_sdp_*_start,           mem_sort_dedup_patch (bwa 0.7.12 - 0.7.17, as recalled): the sort, the redundancy test, the merges through
 *   bsw_sdp_finish             mem_patch_reg and the removal of duplicates, as a job around the patch tickets; both sorts stable
 *   bsw_rescue_*_start,        mem_sam_pe's mate-rescue loop with mem_matesw inside it (bwa 0.7.12 - 0.7.17, as recalled): the anchors,
 *   bsw_rescue_finish          skip[], the contig clamp, the insertion and the sort-and-dedup pass, as a job around the rescue tickets
 *   bsw_cigar_ref_submit_t /   the three calls above as tickets of the streaming pipeline:
 *   bsw_matesw_ref_submit_t /  every device of the context, beside extension submits
 *   bsw_patch_ref_submit_t
 *   bsw_reads_upload,          a read block resident on every device; the three stages as tickets that name a
 *   bsw_*_reads_submit_t       read by its index (only coordinates cross PCIe)
 *
 * Base codes: 0..3 = A,C,G,T; 4 = N; one base per byte, exactly as bwa passes
 * them to ksw_extend.  Left-extension query/target must already be reversed by
 * the caller (as mem_chain2aln does before calling ksw_extend2).
 */
#ifndef BWA_SW_MI355_H
#define BWA_SW_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (never abort; the reference signals no errors at all) ---- */
#define BSW_OK            0
#define BSW_E_NODEVICE   (-1)  /* no gfx950 GPU / HIP runtime unusable            */
#define BSW_E_INVAL      (-2)  /* NULL pointer, bad params (e_ins<=0, h0<=0, ...) */
#define BSW_E_LIMIT      (-3)  /* task outside device limits (see BSW_MAX_*)      */
#define BSW_E_HIP        (-4)  /* a HIP runtime call failed                       */
#define BSW_E_NOMEM      (-5)
#define BSW_E_BUSY       (-6)  /* BSW_MAX_INFLIGHT submits in flight already, or a synchronous call while one is */

/* ---- device limits ------------------------------------------------------- */
#define BSW_MAX_QLEN   8191    /* query side length per extension (ksw_extend2 and the batch API; up to 1 023 in registers,
                                  beyond that the eh[] row lives in LDS: bsw_long_kernel.hip)                          */
#define BSW_GLOBAL_MAX_QLEN 8191 /* ksw_global2 / bsw_global_batch (up to 1 023 in registers, beyond that the eh[]
                                    row lives in an LDS ring the size of the band: bsw_global_long_kernel.hip)       */
#define BSW_MAX_TLEN   65535   /* target side length per extension                */
#define BSW_MAX_SCORE  (1 << 20) /* h0 + qlen*max(mat) must stay below this       */

/* recurrence variant:
 *   H   = the RTL's cell (h += s with no zero test, gaps open from h: sw_pe_array_sw_extend.v:1797-1798,1863,1866) with
 *         modern bwa's column 0 (only while beg == 0) and next-row trimming (first / last entry with h|e != 0); the default;
 *   M   = bwa >= 0.7.9 throughout ("M? M+q : 0");
 *   RTL = the reference: H's cell, column 0 on every row (:1795-1796,1835,849; int32, no 8-bit wrap) and the next row
 *         trimmed to the run of non-zero h around the row maximum's column, e ignored (:1767-1769,1779,1790,1872). */
#define BSW_VARIANT_H    0
#define BSW_VARIANT_M    1
#define BSW_VARIANT_RTL  2

typedef struct bsw_params {
    int8_t  mat[25];        /* 5x5 scoring matrix, row = target base (K6)        */
    int8_t  _pad[3];
    int32_t o_del, e_del;   /* G0 [7:0], [15:8]                                  */
    int32_t o_ins, e_ins;   /* G0 [23:16], [31:24]                               */
    int32_t w;              /* G1 [23:16]  opt->w                                */
    int32_t pen_clip5;      /* G1 [7:0]    also end_bonus of the left extension  */
    int32_t pen_clip3;      /* G1 [15:8]   also end_bonus of the right extension */
    int32_t zdrop;          /* not in the RTL (quirk Q3); bwa default 100        */
    int32_t max_band_try;   /* MAX_BAND_TRY, 2 in bwa and in the RTL (:1963)     */
    int32_t variant;        /* BSW_VARIANT_H (default), _M or _RTL               */
} bsw_params;

/* One seed = left + right extension (what one RTL processing element handles). */
typedef struct bsw_task {
    const uint8_t *lquery;  /* reversed query[0..qbeg)          (H0 qlen0)       */
    const uint8_t *ltarget; /* reversed reference left of seed  (H0 tlen0)       */
    const uint8_t *rquery;  /* query[qbeg+len..l_query)         (H1 qlen1)       */
    const uint8_t *rtarget; /* reference right of the seed      (H1 tlen1)       */
    int32_t  lqlen, ltlen, rqlen, rtlen;
    int32_t  h0;            /* s->len * a                       (H4)             */
    int32_t  init_score;    /* a->score before the left ext; bwa: -1 (H3 low)    */
    int32_t  qbeg;          /* s->qbeg                          (H3 high)        */
    uint32_t tag;           /* opaque, echoed back              (H7 -> R0)       */
    /* Host-supplied band limits min(max_ins, max_del) per side — the RTL's header words H5 / H6
     * (sw_pe_array_proc_element.v:925,933; applied at sw_pe_array_sw_extend.v:1881,1890).
     * 0 = let the library compute them with bwa's formula from the scoring parameters. */
    int32_t  wlim_l, wlim_r;
} bsw_task;

/* Raw outputs of the last ksw_extend2 pass of one side (K9) + bookkeeping. */
typedef struct bsw_ext {
    int32_t  score, qle, tle, gtle, gscore, max_off;
    int32_t  aw;            /* band width of the last pass, unclamped w<<k (P3)  */
    uint32_t cells;         /* DP cells evaluated over all passes of this side   */
} bsw_ext;

typedef struct bsw_result {
    uint32_t tag;           /* R0                                                */
    int32_t  qb, qe;        /* R1: qb absolute in the query; qe relative to the
                                   seed's query end                              */
    int32_t  rb, re;        /* R2: relative to the seed's reference begin / end
                                   (rb = -tle or -gtle)                          */
    int32_t  score, truesc; /* R3                                                */
    int32_t  w;             /* R4: max(aw_left, aw_right)                        */
    bsw_ext  left, right;   /* not in the RTL record; for parity checking        */
} bsw_result;

/* The pair-level record alone: exactly the information of the RTL's 5-word result record R0..R4
 * (sw_pe_array_proc_element.v:1662-1665,1190-1199) — the first 32 bytes of bsw_result.  A context created with
 * bsw_config.result_format = BSW_RESULT_PAIR hands THESE back from bsw_submit / bsw_submit_packed / bsw_submit_ref
 * (the `out` argument then addresses bsw_pair[n], cast to bsw_result *): a third of the bytes over PCIe and out of
 * the finalize kernel; the per-side bsw_ext records stay in device scratch. */
typedef struct bsw_pair {
    uint32_t tag;
    int32_t  qb, qe, rb, re, score, truesc, w;
} bsw_pair;

/* One plain ksw_extend2 call (no band retry), for batched single extensions. */
typedef struct bsw_ext_task {
    const uint8_t *query, *target;
    int32_t qlen, tlen;
    int32_t w, end_bonus, h0;
} bsw_ext_task;

#define BSW_MAX_DEVICES 16
typedef struct bsw_config {
    int32_t device;         /* HIP device ordinal (used when n_devices == 0)      */
    int32_t kernel;         /* BSW_KERNEL_*                                      */
    int32_t streams;        /* staging slots per device = streams = pipeline threads of bsw_submit (1..8, def 4) */
    int32_t pack_threads;   /* helper threads of the slots (def 8): a chunk's host pass (validate, lay out, count) runs on
                               1 + pack_threads / streams threads side by side, and so does the gather of sequences that
                               are NOT in registered memory into pinned staging */
    size_t  chunk_tasks;    /* tasks per H2D/launch chunk in bsw_submit; 0 (def) = sized per submit by the seeds' work:
                               128 Ki seeds of 131-base sides, more of shorter ones (two chunks in flight fill the GPU) */
    /* One context can drive several GPUs, as the reference's batch manager drives its 4 PE arrays
     * round-robin (batch_manager.v:343-348,418; bwa_mem_sw.v:162): chunk k of a bsw_submit goes to
     * devices[k mod n_devices].  n_devices == 0 means the single `device` above.  The same ordinal
     * may appear more than once (more slots on that GPU). */
    int32_t n_devices;
    int32_t devices[BSW_MAX_DEVICES];
    int32_t timeout_ms;     /* watchdog on every wait for the GPU; 0 (def) = BSW_TIMEOUT_MS from the environment, else 120000
                               (bsw_effective_timeout_ms); on expiry the call fails with BSW_E_HIP and the context is dead
                               (every later call fails fast)  */
    int32_t result_format;  /* BSW_RESULT_FULL (def): bsw_result[n]; BSW_RESULT_PAIR: bsw_pair[n] from the bsw_submit* calls */
    int32_t pin_threads;    /* 0 / 1 (def): the slot and gather threads of a device run on the CPUs of that GPU's NUMA node
                               (/sys/bus/pci/devices/<bdf>/local_cpulist, intersected with the process affinity) and their
                               pinned staging is allocated and first touched from there — one manager next to its arrays
                               (batch_manager.v:745-773); -1: threads and staging are left where the OS puts them */
} bsw_config;               /* 104 bytes in ABI 5 (pin_threads took the tail padding of ABI 4) */

/* ABI of this header.  bsw_config has no size field of its own: bsw_create() reads sizeof(bsw_config) of THIS header, so a
 * caller built against an older, shorter struct must use bsw_create_sized() with ITS sizeof (fields beyond it take their
 * defaults) — or check bsw_abi_version() == BSW_ABI_VERSION at start-up.  History: 3 = 96-byte config; 4 = result_format
 * (104 bytes); 5 = pin_threads in the former padding, bsw_create_sized, bsw_chain_timeouts; 6 = tickets (bsw_submit*_t,
 * bsw_wait_ticket, bsw_test: BSW_MAX_INFLIGHT submits per context where 5 answered BSW_E_BUSY to the second), bsw_host_stats,
 * bsw_upload_raw / bsw_run_staged, bsw_default_config writes timeout_ms = 0 (bsw_effective_timeout_ms). */
#define BSW_ABI_VERSION 6

#define BSW_RESULT_FULL  0
#define BSW_RESULT_PAIR  1

#define BSW_KERNEL_AUTO  0  /* per-bin choice (batch manager)                    */
#define BSW_KERNEL_WAVE  1  /* one wavefront per task, row-synchronous           */
#define BSW_KERNEL_LANE  2  /* one lane per task, inter-task SIMD                */

typedef struct bsw_ctx bsw_ctx;
typedef struct bsw_dev_batch bsw_dev_batch;

/* ---- drop-in scalar ABI (bwa ksw.h).  Thread-safe: concurrent callers (bwa mem -t N worker threads)
 * are coalesced into one device batch per round trip (leader/follower; no per-call allocation).
 * Contract at the edges: h0 <= 0 or qlen <= 0 (outside bwa's assert(h0 > 0) domain) returns
 * max(h0,0) with qle = tle = gtle = 0, gscore = -1, max_off = 0 without touching the GPU; on a device
 * failure the call prints the reason to stderr, writes the same neutral outputs and returns -1. ---- */
int ksw_extend2(int qlen, const uint8_t *query, int tlen, const uint8_t *target,
                int m, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                int w, int end_bonus, int zdrop, int h0,
                int *qle, int *tle, int *gtle, int *gscore, int *max_off);
int ksw_extend(int qlen, const uint8_t *query, int tlen, const uint8_t *target,
               int m, const int8_t *mat, int gapo, int gape,
               int w, int end_bonus, int zdrop, int h0,
               int *qle, int *tle, int *gtle, int *gscore, int *max_off);
/* recurrence variant used by ksw_extend/ksw_extend2 (process-wide, default H) */
void bsw_set_default_variant(int variant);
/* calls served / device round trips made by the scalar ABI so far (their ratio = mean coalescing factor) */
void bsw_scalar_stats(uint64_t *calls, uint64_t *trips);

/* ---- BSW_VARIANT_RTL on the packed two-seeds-per-lane kernels (opt-in) ----
 * Process-wide and atomic; applies to the launches enqueued afterwards.  Initially 1 when the environment variable
 * BSW_RTL_PACKED is "1", else 0.  With the switch on, the lane-list sides of variant RTL whose class is the 72- or the
 * 136-column 8-bit class, under scoring parameters in the packed range (a bwa-style matrix, a + b < 256, o + e < 256 per gap
 * kind), run on bsw_lane2_rtl_kernel instead of the one-seed-per-lane kernel, through every entry
 * point that builds lane lists; results are the same bytes.  The 232-column and the 16-bit class, parameters outside that
 * range, and variants H and M are not affected. */
void bsw_set_rtl_packed(int on);
int  bsw_rtl_packed(void);
/* launches of the packed RTL kernel so far, per instantiation: [0] 72 columns shared gap penalties (o_del == o_ins and
 * e_del == e_ins), [1] 72 separate, [2] 136 shared, [3] 136 separate.  Writes min(cap, 4) counters, returns 4. */
int  bsw_rtl_packed_stats(uint64_t *launches, int cap);

/* ---- ksw_align2 for queries of 1 025 to BSW_ALIGN_LONG_MAX_QLEN bases (opt-in) ----
 * Process-wide and atomic; applies to the calls that enter the library afterwards (a call or a submit reads the switch once, in
 * the caller's thread: a ticket submitted under mode 1 completes under mode 1 whatever the switch says by then).  Initially the
 * value of the environment variable BSW_ALIGN_LONG when that is "1" or "2", else 0.
 *   0  a query beyond BSW_ALIGN_MAX_QLEN is refused: BSW_E_LIMIT from the batch calls, score -1 from ksw_align2 / ksw_align.
 *   1  ksw_align2, ksw_align, bsw_align_batch, bsw_matesw_ref_batch, bsw_matesw_ref_submit_t and bsw_matesw_reads_submit_t accept
 *      queries (mates) up to BSW_ALIGN_LONG_MAX_QLEN bases; those beyond BSW_ALIGN_MAX_QLEN run on bsw_align_long_kernel
 *      (the rows of H, E and Hmax in LDS), shorter ones on bsw_align_kernel as before.  Results are the
 *      same bit-exact ksw_u8 / ksw_i16 values.  Beyond BSW_ALIGN_LONG_MAX_QLEN: BSW_E_LIMIT still.
 *   2  as 1, and every alignment runs on bsw_align_long_kernel, the short ones too (tests, rate comparisons).
 * Any other value sets 0. */
#define BSW_ALIGN_LONG_MAX_QLEN 8191
void bsw_set_align_long(int mode);
int  bsw_align_long(void);
/* launches of bsw_align_long_kernel so far, per class: (8-bit mode, slen bound 16, 32, ... 512), then (16-bit mode, slen bound
 * 32, 64, ... 1 024); slen = ceil(qlen / 16) resp. ceil(qlen / 8).  Writes min(cap, classes) counters, returns the number of
 * classes (12). */
int  bsw_align_long_stats(uint64_t *launches, int cap);

/* ---- batch API ------------------------------------------------------------ */
void     bsw_default_params(bsw_params *p);          /* bwa defaults a=1,b=4,o=6,e=1,w=100,clip=5,zdrop=100 */
void     bsw_default_config(bsw_config *c);
int      bsw_device_count(void);                     /* gfx950 devices visible; <=0 if none */
int      bsw_create(const bsw_config *cfg, bsw_ctx **out);
int      bsw_create_sized(const bsw_config *cfg, size_t cfg_size, bsw_ctx **out);   /* cfg_size = the CALLER's sizeof(bsw_config) */
/* Where device k of the context (index into bsw_config.devices[]) sits: PCI address ("0000:c1:00.0"), NUMA node (-1: the
 * kernel does not say) and how many CPUs next to it the context's slot threads are pinned to (0: not pinned). */
int      bsw_device_placement(const bsw_ctx *ctx, int k, char *bdf, size_t bdf_cap, int *numa_node, int *n_cpus);
int      bsw_abi_version(void);                      /* BSW_ABI_VERSION the library was built with */
/* The watchdog (ms) a context created from cfg would run with: cfg->timeout_ms when > 0, else the environment variable
 * BSW_TIMEOUT_MS when it holds a positive number, else 120000.  bsw_default_config writes 0.  Host only. */
int      bsw_effective_timeout_ms(const bsw_config *cfg);
/* How many of the launch chain's waiting waves gave up at their 20 ms deadline so far (the chain's flag is a
 * scheduling hint, a follower released early is still correct).  Non-zero where kernels are run one at a time
 * (rocprofv3 --pmc, HIP_LAUNCH_BLOCKING, AMD_SERIALIZE_KERNEL); 0 in normal operation.  Synchronises the context. */
int      bsw_chain_timeouts(bsw_ctx *ctx, uint64_t *n);
void     bsw_destroy(bsw_ctx *ctx);
const char *bsw_last_error(const bsw_ctx *ctx);      /* text of the last failure  */

/* ---- host memory the GPU can DMA directly.  Sequences and result arrays that live in memory obtained
 * from bsw_host_alloc (or registered with bsw_host_register) cross PCIe with NO host copy: bsw_submit
 * DMAs the byte-per-base arena of a chunk as it is and packs / bins it on the GPU.  Anything else is first
 * gathered into pinned staging by `pack_threads` host threads (correct, but host-bound).  Process-wide. ---- */
void    *bsw_host_alloc(size_t bytes);
void     bsw_host_free(void *p);
int      bsw_host_register(void *p, size_t bytes);
int      bsw_host_unregister(void *p);

/* Asynchronous: validates lengths, DMAs the raw sequences to the device in chunks (chunk k ->
 * device k mod n_devices), packs + bins them there, launches, copies results back into out[] in
 * TASK ORDER.  out[], tasks[] and the task sequences must stay valid until the submit has been waited for.
 * Up to BSW_MAX_INFLIGHT submits may be in flight per context (the reference's manager keeps four task batches
 * going: batch_manager.v:343-348 request bits, :434-435 busy bitmap); their chunks run through the context's slots in
 * submit order, so the tail of one overlaps the head of the next.  One more than that answers BSW_E_BUSY.
 * bsw_wait waits for ALL of them and returns the first failure in submit order.
 *
 * THREADS.  bsw_submit*_t (and the forms without a ticket), bsw_cigar_ref_submit_t, bsw_matesw_ref_submit_t, bsw_patch_ref_submit_t, the four
 * *_reads_* submits (bsw_patch_reads_submit_t among them), bsw_reads_upload, bsw_reads_upload_enc, bsw_reads_upload_start, bsw_reads_upload_start_enc, bsw_reads_test,
 * bsw_reads_wait, bsw_reads_free, bsw_sdp_ref_start, bsw_sdp_reads_start, bsw_sdp_test, bsw_sdp_finish, bsw_sdp_job_stats,
 * bsw_rescue_ref_start, bsw_rescue_reads_start, bsw_rescue_test, bsw_rescue_finish, bsw_rescue_job_stats, bsw_rescue_job_out_capacity (one job from one thread at a time),
 * bsw_wait_ticket, bsw_test, bsw_wait and bsw_inflight may be called on ONE context from several threads at once, the first submit included;
 * every other call that takes the context (bsw_destroy, the synchronous and resident calls, bsw_ref_upload / bsw_ref_free,
 * bsw_host_stats, bsw_reads_image) needs it to itself.  bsw_set_align_long, bsw_align_long and bsw_align_long_stats take no
 * context and may be called from any thread at any time; a change applies to the calls that enter the library afterwards.
 *   - bsw_reads_upload and bsw_reads_free may run while tickets are in flight (block k+1 is uploaded while block k is on the GPU):
 *     the upload copies on a stream of its own per device and returns when the copies are complete; a block is handed to a
 *     submit only after its upload has returned, and freed only by one thread.
 *   - bsw_reads_upload_start returns at once and its block may be handed to a submit at once, from any thread; bsw_reads_test and
 *     bsw_reads_wait may be called on one block from several threads.
 *   - A ticket belongs to whoever collects it first.  bsw_wait collects every submit in flight when it is called, other threads'
 *     too; a thread blocked in bsw_wait_ticket on a ticket that bsw_wait (or a second bsw_wait_ticket) collects meanwhile returns
 *     BSW_E_INVAL once that submit is complete: its results are in out[], its error code went to the collector.
 *     bsw_test answers < 0 for a collected ticket.
 *   - BSW_E_BUSY from a submit (BSW_MAX_INFLIGHT in flight) changes nothing: collect a ticket and submit again.
 *   - bsw_last_error is one text per context: with several threads it describes the last failure of ANY of them, and the
 *     pointer is good until the next failing call; read it only while no other thread is inside a call on the context. */
#define BSW_MAX_INFLIGHT 4
typedef uint64_t bsw_ticket;            /* names one submit; never 0 */
int      bsw_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out);
int      bsw_wait(bsw_ctx *ctx);
/* the same submit, handing back its ticket (ticket may be NULL) */
int      bsw_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out, bsw_ticket *ticket);
/* wait for ONE submit and collect it: its error code, BSW_E_INVAL for a ticket that is not in flight */
int      bsw_wait_ticket(bsw_ctx *ctx, bsw_ticket ticket);
/* the host's status poll (the busy nibble at DSM + 0x40, batch_manager.v:844-854): 1 = complete (out[] is filled; collect the
 * submit and its error code with bsw_wait_ticket / bsw_wait), 0 = in flight, < 0 = no such ticket.  Never blocks. */
int      bsw_test(bsw_ctx *ctx, bsw_ticket ticket);
int      bsw_inflight(bsw_ctx *ctx);    /* submits not collected by a wait yet */
/* What the host side of the streaming path has cost so far: CPU time of the context's slot threads (validate, lay out,
 * count, start DMAs, poll) and of the gather helpers (sequences outside registered memory), and the volume moved.  out_size
 * = the caller's sizeof(bsw_stats). */
typedef struct bsw_stats {
    uint64_t slot_cpu_ns, helper_cpu_ns;    /* CLOCK_THREAD_CPUTIME_ID, summed over threads */
    uint64_t seeds, chunks, submits;
    uint64_t h2d_bytes, d2h_bytes;
    uint64_t slot_threads;
} bsw_stats;
int      bsw_host_stats(bsw_ctx *ctx, bsw_stats *out, size_t out_size);
/* The same for callers that keep sequences 4-BIT PACKED: the bsw_task pointers then address uint64 words, 16 bases
 * each (base k in bits [4k, 4k+3]; codes 0-3 = ACGT, 4-7 = N), every sequence starting on an 8-byte boundary; the
 * lengths stay in bases; the unused nibbles behind a sequence's last base may hold anything.  This is the device's own layout and the encoding the reference ships over its link (8 bases
 * per 32-bit word, first base in the top nibble there: sw_pe_array_proc_element.v:1638,1677-1683).  Words in registered
 * memory are DMA'd straight into the sequence buffer — no pack kernel, ~0.6x the PCIe bytes per seed of bsw_submit.
 * bsw_pack_bases() packs one byte-per-base sequence; bsw_pack_tasks() a whole task array. */
int      bsw_submit_packed(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out);
int      bsw_submit_packed_t(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out, bsw_ticket *ticket);
/* tasks[0..n) (byte per base) -> out[0..n) with the sequences packed into `arena` (8-byte aligned, `cap` bytes);
 * returns the bytes used or <0 (BSW_E_NOMEM: arena too small).  bsw_pack_tasks_bound() = a sufficient `cap`. */
int64_t  bsw_pack_tasks(const bsw_task *tasks, size_t n, uint64_t *arena, size_t cap, bsw_task *out);
size_t   bsw_pack_tasks_bound(const bsw_task *tasks, size_t n);
/* Batched plain ksw_extend2 (one pass each, w/end_bonus/h0 per task); synchronous. */
int      bsw_extend_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_ext_task *tasks, size_t n, bsw_ext *out);

/* ---- banded global alignment with CIGAR: bwa's ksw_global2 / ksw_global (ksw.c), the
 * Smith-Waterman user after seed extension inside mem_reg2aln (bwa_gen_cigar2).  Not in the reference RTL — it
 * belongs to the host software named at reference README.md:7-18.  CIGAR encoding is BAM's: len << 4 | op,
 * op 0 = M, 1 = I, 2 = D.  Queries up to BSW_GLOBAL_MAX_QLEN = 8 191 bases (bwa's routine has no limit; the read-sized
 * path keeps the row in registers, queries of 1 024 bases and more run with the row in LDS), targets and bands up to
 * BSW_MAX_TLEN. ---- */
typedef struct bsw_gtask {
    const uint8_t *query, *target;   /* codes 0..4, one per byte */
    int32_t qlen, tlen, w;           /* w = band half-width */
    int32_t _pad;
} bsw_gtask;
typedef struct bsw_gresult {
    int32_t score;                   /* eh[qlen].h of the last row, exactly as bwa returns it */
    int32_t n_cigar;                 /* CIGAR operations written; < 0: -n operations did not fit max_cigar */
} bsw_gresult;
/* Batched ksw_global2 on the GPU.  cigars (may be NULL: scores only) receives max_cigar words per task. */
int      bsw_global_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_gtask *tasks, size_t n, int max_cigar,
                          bsw_gresult *res, uint32_t *cigars);
/* drop-in scalar ABI (bwa ksw.h): *cigar is malloc'ed, the caller frees it; n_cigar / cigar may be NULL */
int ksw_global2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                int o_del, int e_del, int o_ins, int e_ins, int w, int *n_cigar, uint32_t **cigar);
int ksw_global(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
               int gapo, int gape, int w, int *n_cigar, uint32_t **cigar);

/* ---- bwa_gen_cigar2 against a DEVICE-RESIDENT reference (bwa.c; mem_reg2aln's band-widening loop around it, bwamem.c):
 * reads plus reference intervals go in, score, CIGAR, NM and MD come back.  The target [rb, re) is fetched on the GPU from
 * the reference of bsw_ref_upload (reverse strand: the read and the target are both reversed, as bwa does, so indels sit
 * leftmost and the CIGAR / MD are in that reversed frame), the band follows bwa's formula, ksw_global2 runs on the GPU and
 * NM / MD are computed there from the CIGAR.  Only the reads cross PCIe.  The whole batch runs on the context's first device
 * (bsw_cigar_ref_submit_t below: the same work as a ticket, over every device of the context).
 * Retry (mem_reg2aln):  w2 = w; last = -(1 << 30);
 *     do { w2 = min(w2, w_cap); bwa_gen_cigar2(w_ = w2); if (score == last || w2 == w_cap) break; last = score; w2 <<= 1; }
 *     while (++i < max_tries && score < min_score);
 * the outputs are those of the final try. ---- */
struct bsw_ref;                /* (bsw_ref_upload, below) */
typedef struct bsw_ctask {
    const uint8_t *query;    /* read bases [qb, qe) in read order, codes 0..4 (bwa passes &query[qb])                */
    int32_t  l_query;        /* qe - qb, <= BSW_GLOBAL_MAX_QLEN                                                     */
    int32_t  w;              /* w_ of the first try (0..BSW_MAX_TLEN)                                               */
    int64_t  rb, re;         /* reference interval in bwa coordinates [0, 2*l_pac); re - rb <= BSW_MAX_TLEN          */
    int32_t  w_cap;          /* retries never exceed this band (0: = w, i.e. no widening)                          */
    int32_t  min_score;      /* retry while score < min_score (truesc - a in bwa); INT32_MIN: never                 */
    int32_t  max_tries;      /* 1..3 (0 = 1 = plain bwa_gen_cigar2)                                                 */
    int32_t  _pad;
} bsw_ctask;                 /* 48 bytes */
typedef struct bsw_cresult {
    int32_t score;           /* global score of the final try (0 when status != 0)                                  */
    int32_t n_cigar;         /* ops written; < 0: -n ops did not fit max_cigar (as bsw_global_batch)                 */
    int32_t nm;              /* edit distance as bwa computes it; -1 when there is no CIGAR (status, CIGAR overflow)  */
    int32_t md_len;          /* MD bytes written without the NUL; < 0: -(bytes needed, NUL included) did not fit max_md
                                (the slot then holds ""); 0 with nm == -1.  md == NULL: the MD's length, nothing written */
    int32_t w;               /* w_ of the final try                                                                 */
    int32_t tries;           /* bwa_gen_cigar2 calls made, 1..max_tries                                             */
    int32_t status;          /* 0; 1: bwa returns no alignment (l_query == 0, rb >= re, the interval bridges l_pac or
                                leaves [0, 2*l_pac)) — such a task does not fail the batch                          */
    int32_t _pad;
} bsw_cresult;               /* 32 bytes */
/* Batched bwa_gen_cigar2 (+ retries) on the GPU.  max_cigar >= 1 words per task of CIGAR room on the device and in cigars
 * (may be NULL: not returned); md (may be NULL) receives a NUL-terminated MD string in a slot of max_md bytes per task.
 * The first malformed task rejects the batch: negative length or band, NULL query, max_tries outside 0..3 -> BSW_E_INVAL;
 * l_query > BSW_GLOBAL_MAX_QLEN, re - rb > BSW_MAX_TLEN, w or w_cap > BSW_MAX_TLEN -> BSW_E_LIMIT. */
int      bsw_cigar_ref_batch(bsw_ctx *ctx, const bsw_params *p, const struct bsw_ref *ref, const bsw_ctask *tasks, size_t n,
                             int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res);
/* The same as a TICKET of the context's pipeline (bsw_submit_t above: one ticket space, BSW_MAX_INFLIGHT submits of any mix,
 * collected by bsw_wait_ticket / bsw_wait, polled by bsw_test, counted by bsw_inflight; ticket may be NULL; n == 0 completes at
 * once).  The argument and task checks of bsw_cigar_ref_batch run in the caller's thread before anything is queued, with the
 * same codes and texts, and no ticket is made when they fail; BSW_E_BUSY changes nothing.  The submit is cut into chunks by
 * work, chunk k runs on device k mod n_devices of the context against that device's copy of the reference, on the slot threads
 * and streams the extension submits use, in submit order with them: it is accepted while extension submits are in flight and
 * the other way round.  res, cigars and md receive, byte for byte, what bsw_cigar_ref_batch writes for the same tasks, in task
 * order.  tasks[], the reads they point to, res, cigars and md stay valid until the ticket is collected.  A chunk that fails
 * makes the others of its ticket give up; the wait returns the failure, nothing of the ticket is still queued then (this holds for
 * every submit: a slot whose own wait for a chunk fails waits once more before it reports, so res and the other arrays may be freed as
 * soon as bsw_wait_ticket has returned the failure — unless the context is dead, below), and other tickets are left alone.  May be called on one context from several threads (THREADS above).
 * A watchdog expiry is different: the wait answers BSW_E_HIP, the context is dead, and what the hung device still holds in its
 * queues may read the reads and `ref` whenever it wakes.  Call bsw_destroy (it leaves the runtime alone on a dead context), do
 * NOT call bsw_ref_free on that reference and do not free or unregister the reads of the failed tickets: that memory is
 * abandoned with the device, as the context's own buffers are; a new context needs a new bsw_ref_upload.
 * The work a chunk holds is a constant of the library; the environment variables BSW_F4_CIGAR_WORK /
 * BSW_F4_MATESW_WORK replace it for tests and measurements only. */
int      bsw_cigar_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const struct bsw_ref *ref, const bsw_ctask *tasks, size_t n,
                                int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res, bsw_ticket *ticket);
/* mem_reg2aln's infer_bw: the band a global alignment of l1 x l2 bases needs to reach `score` (a = match, q / r = gap
 * open / extend of one kind; bwa takes the larger of the deletion and the insertion answers) */
int      bsw_infer_bw(int l1, int l2, int score, int a, int q, int r);

/* ---- local alignment with start / second-best search (second half: bwa ksw.h ksw_align2, the
 * Smith-Waterman of mate rescue, mem_matesw; like ksw_global2 it lives in the reference's host software, the
 * bwa-0.7.8 tree named at /root/reference/README.md:7-18, not in the RTL) ---------------------------------
 * Results are those of bwa's striped SSE2 code (ksw_u8 when KSW_XBYTE is set, else ksw_i16), bit for bit: score
 * (255 = the 8-bit run saturated, call again without KSW_XBYTE), te/qe (end on target / query, inclusive),
 * score2/te2 (best end at least ceil(score/max) rows away, needs KSW_XSUBO | threshold), tb/qb (start, needs
 * KSW_XSTART; -1 when the start pass did not run or disagrees).  xtra = flags | 16-bit threshold, as in bwa.
 * The matrix is mat[target code * 5 + query code] and need not be symmetric; codes above 4 count as 4; 16-bit scores saturate at
 * 32 767.  Two things ksw_u8 has no byte for are rejected, per task, by bsw_align_batch, bsw_matesw_ref_batch and its ticket forms
 * and (as the call's failure, score -1) by ksw_align2 / ksw_align; the same task without KSW_XBYTE runs:
 *   - KSW_XBYTE with a matrix whose smallest entry is above 0 -> BSW_E_INVAL.  ksw_qinit's shift 256 - min wraps there and the
 *     SSE2 code adds a wrapped profile byte; a smallest entry of 0 (shift 0) is the last one that works;
 *   - KSW_XBYTE with o_del + e_del > 255 or o_ins + e_ins > 255 -> BSW_E_LIMIT.  bwa keeps these sums in 8-bit lanes
 *     (_mm_set1_epi8), so 256 would act as 0 there; 255 is accepted. */
#define KSW_XBYTE  0x10000
#define KSW_XSTOP  0x20000
#define KSW_XSUBO  0x40000
#define KSW_XSTART 0x80000
#define BSW_ALIGN_MAX_QLEN 1024
typedef struct bsw_kswr {            /* = bwa's kswr_t */
    int32_t score, te, qe, score2, te2, tb, qb;
} bsw_kswr;
typedef struct bsw_atask {
    const uint8_t *query, *target;   /* codes 0..4, one per byte */
    int32_t qlen, tlen;              /* qlen <= BSW_ALIGN_MAX_QLEN; <= BSW_ALIGN_LONG_MAX_QLEN under bsw_set_align_long(1 / 2) */
    int32_t xtra;
    int32_t _pad;
} bsw_atask;
/* Batched ksw_align2 on the GPU (m = 5; p supplies mat and the four gap penalties). */
int      bsw_align_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_atask *tasks, size_t n, bsw_kswr *out);
/* drop-in scalar ABI (bwa ksw.h).  qry (bwa's query-profile cache) is not used: pass NULL, or a pointer whose target
 * stays NULL. */
#ifndef __AC_KSW_H
typedef struct { int score; int te, qe; int score2, te2; int tb, qb; } kswr_t;
#endif
kswr_t ksw_align2(int qlen, uint8_t *query, int tlen, uint8_t *target, int m, const int8_t *mat,
                  int o_del, int e_del, int o_ins, int e_ins, int xtra, void **qry);
kswr_t ksw_align(int qlen, uint8_t *query, int tlen, uint8_t *target, int m, const int8_t *mat,
                 int gapo, int gape, int xtra, void **qry);

/* ---- mate rescue against a DEVICE-RESIDENT reference (bwa's mem_matesw, bwamem_pair.c): one ksw_align2 per window,
 * the window [rb, re) fetched on the GPU from the reference of bsw_ref_upload (bns_get_seq semantics, both strands), the
 * mate complemented and reversed on the GPU when is_rev.  Only the mates cross PCIe.  The whole batch runs on the context's
 * first device (bsw_matesw_ref_submit_t below: the same work as a ticket, over every device of the context).  mem_matesw's bookkeeping (which orientations to try, its order dependency) is bsw_rescue_* further down, a job around
 * these tickets; a host that keeps it to itself has bsw_infer_dir and bsw_matesw_windows below, INTEGRATION.md "Mate rescue".  Kept (status 0) exactly when bwa keeps the
 * region: aln.score >= min_score && aln.qb >= 0. ---- */
typedef struct bsw_mtask {
    const uint8_t *mate;     /* the mate in READ order, codes 0..4 (bwa's ms)                                       */
    int32_t  l_ms;           /* 0..BSW_ALIGN_MAX_QLEN, 0..BSW_ALIGN_LONG_MAX_QLEN under bsw_set_align_long(1 / 2) (0: status 1,
                                nothing run)                                                                          */
    int32_t  is_rev;         /* 0 / 1: align the reverse complement of the mate (mem_matesw: r>>1 != (r&1))          */
    int64_t  rb, re;         /* the window in bwa coordinates [0, 2*l_pac), as the caller would fetch it; re - rb <=
                                BSW_MAX_TLEN                                                                          */
    int32_t  xtra;           /* ksw_align2 flags | threshold, as mem_matesw builds them                              */
    int32_t  min_score;      /* keep the region when score >= min_score && qb >= 0 (bwa: opt->min_seed_len)          */
} bsw_mtask;                 /* 40 bytes */
typedef struct bsw_mresult {
    bsw_kswr aln;            /* ksw_align2's outputs in the window's frame (query = the mate as aligned, reverse-
                                complemented when is_rev), bit for bit; status 1: {0, -1, -1, -1, -1, -1, -1}          */
    int32_t  status;         /* 0 kept; 1 not run (l_ms == 0, rb >= re, the window bridges l_pac or leaves
                                [0, 2*l_pac)) -- such a task does not fail the batch; 2 run, not kept                */
    int64_t  rb, re;         /* mem_matesw's b.rb / b.re (bwa coordinates); status 0 only, else 0                      */
    int32_t  qb, qe;         /* b.qb / b.qe in the mate's read order; status 0 only, else 0                           */
    int32_t  score, csub;    /* b.score = aln.score, b.csub = aln.score2; status 0 only, else 0                        */
    int32_t  seedcov;        /* min(re - rb, qe - qb) >> 1; status 0 only, else 0                                     */
    int32_t  _pad;
} bsw_mresult;               /* 72 bytes */
/* Batched mem_matesw Smith-Waterman on the GPU (m = 5; p supplies mat and the four gap penalties).  The first malformed task
 * rejects the batch: negative l_ms, NULL mate, is_rev other than 0 / 1, an unknown xtra flag -> BSW_E_INVAL;
 * l_ms > BSW_ALIGN_MAX_QLEN (BSW_ALIGN_LONG_MAX_QLEN under bsw_set_align_long(1 / 2)) or re - rb > BSW_MAX_TLEN -> BSW_E_LIMIT;
 * KSW_XBYTE with a matrix minimum above 0 -> BSW_E_INVAL, with a gap open + extend above 255 -> BSW_E_LIMIT (at KSW_XBYTE above). */
int      bsw_matesw_ref_batch(bsw_ctx *ctx, const bsw_params *p, const struct bsw_ref *ref, const bsw_mtask *tasks, size_t n,
                              bsw_mresult *res);
/* The same as a TICKET of the context's pipeline: the contract of bsw_cigar_ref_submit_t above, with the checks and the results
 * of bsw_matesw_ref_batch.  tasks[], the mates they point to and res stay valid until the ticket is collected.  mem_matesw's
 * replay of the anchor order (INTEGRATION.md "Mate rescue") runs on res after the ticket is collected. */
int      bsw_matesw_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const struct bsw_ref *ref, const bsw_mtask *tasks, size_t n,
                                 bsw_mresult *res, bsw_ticket *ticket);
/* mem_infer_dir: the orientation (0..3) of a pair whose leftmost positions are b1 (anchor) and b2 (mate), and in *dist the
 * distance between them on the anchor's strand */
int      bsw_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist);
/* mem_matesw's windows for the four orientations r of an anchor at anchor_rb and a mate of l_ms bases, from the insert size
 * bounds low[r] / high[r] of bwa's mem_pestat_t: rb[r], re[r] clamped to [0, 2*l_pac) (the window may come out empty),
 * is_rev[r] = r>>1 != (r&1), skip[r] = failed[r] != 0.  The contig clamp of newer bwa's bns_fetch_seq and its rid check are not
 * made here (bsw_rescue_* makes them).  Returns BSW_OK, or BSW_E_INVAL for NULL arrays, l_pac < 1 or l_ms < 0. */
int      bsw_matesw_windows(int64_t anchor_rb, int l_ms, int64_t l_pac, const int32_t low[4], const int32_t high[4],
                            const int32_t failed[4], int64_t rb[4], int64_t re[4], int32_t is_rev[4], int32_t skip[4]);

/* ---- device-resident batches (inputs in HBM before the timed region) ------- */
int      bsw_upload(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_dev_batch **out);
int      bsw_upload_packed(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_dev_batch **out);   /* 4-bit packed sequences, as bsw_submit_packed */
int      bsw_run(bsw_ctx *ctx, bsw_dev_batch *b);          /* enqueue kernels only        */
/* bsw_upload that also KEEPS the byte-per-base sequences (as they crossed PCIe) in HBM, and bsw_run_staged = the whole device
 * side of one chunk of bsw_submit on such a batch: pack (bytes -> 16 bases per uint64) + bin (counting sort into the launch
 * lists) + the DP kernels — the batch manager's work from "task batch landed" to "result batch ready" (tbb.v:110-123,
 * sw_pe_array_task_parse.v:1600-1648, rbb.v:219-224), inputs resident in HBM.  bsw_run on such a batch still runs the DP
 * kernels alone.  bsw_run_history2 splits every run since the last call into total / pack + bin milliseconds (HIP events on
 * the library's stream). */
int      bsw_upload_raw(bsw_ctx *ctx, const bsw_params *p, const bsw_task *tasks, size_t n, bsw_dev_batch **out);
int      bsw_run_staged(bsw_ctx *ctx, bsw_dev_batch *b);
int      bsw_run_history2(bsw_ctx *ctx, float *total_ms, float *staging_ms /* may be NULL */, int cap);
int      bsw_sync(bsw_ctx *ctx);                            /* hipStreamSynchronize        */
int      bsw_download(bsw_ctx *ctx, bsw_dev_batch *b, bsw_result *out); /* task order      */
int      bsw_batch_info(const bsw_dev_batch *b, uint64_t *n_tasks, uint64_t *in_bytes, uint64_t *out_bytes, uint64_t *n_launches);
/* the launch order the device-side binning produced for a resident batch (same layout as bsw_plan_batch, up to the redo
 * list: seg[25] <= 4*n words are written; order[] of bsw_plan_order_capacity(n) words always holds them; seg[BSW_PLAN_SEGS+1]);
 * for tests and tools */
int      bsw_batch_order(bsw_ctx *ctx, const bsw_dev_batch *b, uint32_t *order, uint32_t *seg);
/* time of the kernels of the last bsw_run, measured with hipEvents on the
 * library's own stream; valid after bsw_sync.                                  */
int      bsw_last_run_ms(bsw_ctx *ctx, float *ms);
/* kernel time (ms) of every bsw_run since the previous call, oldest first; returns the
 * count written (<= cap) and resets the history.  Synchronises on the recorded events.   */
int      bsw_run_history(bsw_ctx *ctx, float *ms, int cap);
void     bsw_free_batch(bsw_ctx *ctx, bsw_dev_batch *b);

/* ---- batch plan (host only, no GPU needed): how the batch manager cuts tasks[0..n) into launches.
 * The device sorts the seeds (bsw_stage_kernel.hip); the host only counts them per class, with the same
 * class functions, to size the launches.  order[] (capacity bsw_plan_order_capacity(n) words = 5*n+32, may be NULL: behind the
 * redo space a chunk that does not fill the machine keeps a list of its lane seeds with an N in a query, n more words that
 * seg[] does not describe; an array of 4*n+16 words, the size this header used to give, is overrun by such a plan) receives a launch order
 * built on the host with the device's rules (lane sides: queries with an N first, each part longest first, left
 * sides of one length by h0 bucket — 8 buckets over the chunk's h0 range; inside one bin the device's order is arbitrary);
 * seg[] receives BSW_PLAN_SEGS+1 offsets into order[]:
 * segments 0..7 = wave-per-task classes (64,128,192,256,512,1024,2048,8192 columns), 8 = all lane seeds,
 * 9..16 = lane left sides per lane class, 17..24 = lane right sides per lane class, 25 = redo list space.
 * kernel = BSW_KERNEL_*.  Returns the number of sequence words the batch needs, or <0. ---- */
#define BSW_PLAN_SEGS 26
int64_t  bsw_plan_batch(const bsw_params *p, const bsw_task *tasks, size_t n, int kernel, int pack_threads,
                        uint32_t *order, uint32_t *seg /*[BSW_PLAN_SEGS+1]*/);
/* words of order[] that bsw_plan_batch / bsw_batch_order may write for a batch of n tasks */
size_t   bsw_plan_order_capacity(size_t n);

/* ---- reference wire format (bwa_mem_sw.v:163-170) ----------- */
#define BSW_REFBATCH_IN_WORDS   65536   /* 256 KiB task batch (tbb.v:59)         */
#define BSW_REFBATCH_OUT_WORDS  4096    /* 16 KiB result batch (rbb.v:59)        */
#define BSW_REFBATCH_MAX_TASKS  819     /* floor(4096/5) five-word records       */
/* Encode up to n tasks; returns the number of tasks that fit (>=0) or <0.
 * Tasks whose fields exceed the RTL's port widths (quirk Q1) stop the batch.   */
int      bsw_refbatch_encode(const bsw_params *p, const bsw_task *tasks, size_t n, uint32_t *words /*[65536]*/);
/* Decode a task batch; sequences are unpacked into seqbuf (byte per base).     */
int      bsw_refbatch_decode(const uint32_t *words, bsw_params *p, bsw_task *tasks, size_t max_tasks,
                             uint8_t *seqbuf, size_t seqbuf_len);
int      bsw_refbatch_encode_results(const bsw_result *res, size_t n, uint32_t *words /*[4096]*/);
int      bsw_refbatch_decode_results(const uint32_t *words, size_t n, bsw_result *res);
/* Run one 256 KiB task batch end to end on the GPU and fill the 16 KiB result
 * batch — what one RTL PE array does between task_start and TestCmp.           */
int      bsw_refbatch_run(bsw_ctx *ctx, const uint32_t *in_words, uint32_t *out_words, int variant, int zdrop);
/* Queue a task batch (asynchronous; the reference keeps 4 in flight, batch_manager.v:418,745-773; here up to
 * BSW_REFBATCH_MAX_INFLIGHT).  in_words / out_words must stay valid until bsw_refbatch_wait, which runs
 * everything queued as ONE device batch (the nibble streams are unpacked on the GPU), fills every out_words
 * in TASK ORDER (the RTL emits completion order and relies on the tag, sw_pe_array_fill_resulBuf.v:377-429)
 * and returns the number of batches completed or <0.  All batches of one wait share variant / zdrop.
 * The header's H5/H6 (max_ins/max_del) are honoured as the band limits, as in the RTL. */
#define BSW_REFBATCH_MAX_INFLIGHT 256
int      bsw_refbatch_submit(bsw_ctx *ctx, const uint32_t *in_words, uint32_t *out_words);
int      bsw_refbatch_wait(bsw_ctx *ctx, int variant, int zdrop);

/* ---- mem_chain2aln caller glue: what bwamem.c does either side of ksw_extend2.
 * Reference coordinates are bwa's: [0, l_pac) forward strand, [l_pac, 2*l_pac) reverse complement. ---- */
typedef struct bsw_seed {           /* mem_seed_t */
    int64_t rbeg;
    int32_t qbeg, len;
} bsw_seed;
typedef struct bsw_alnreg {         /* the fields of mem_alnreg_t this path produces */
    int64_t rb, re;
    int32_t qb, qe;
    int32_t score, truesc, w;
} bsw_alnreg;
/* cal_max_gap(opt, qlen): longest gap a qlen-base flank can pay for, capped at 2w */
int      bsw_cal_max_gap(const bsw_params *p, int qlen);
/* the chain's reference window [rmax[0], rmax[1]) as mem_chain2aln computes it from all seeds of a chain */
int      bsw_chain_window(const bsw_params *p, const bsw_seed *seeds, int n_seeds, int l_query, int64_t l_pac, int64_t rmax[2]);
/* bytes of scratch bsw_seed_to_task needs for the reversed left query + left target */
size_t   bsw_seed_scratch_bytes(const bsw_seed *s, int64_t rmax0);
/* one seed -> one task.  rseq = reference bases of [rmax0, rmax1) (bns_get_seq), query = the read (codes 0..4).
 * The left query/target are written reversed into scratch; right ones point into query / rseq. */
int      bsw_seed_to_task(const bsw_params *p, const bsw_seed *s, int l_query, const uint8_t *query,
                          int64_t rmax0, int64_t rmax1, const uint8_t *rseq,
                          uint8_t *scratch, size_t scratch_len, uint32_t tag, bsw_task *t);
/* result record -> alignment region in read / reference coordinates */
int      bsw_result_to_alnreg(const bsw_seed *s, const bsw_result *r, bsw_alnreg *a);
/* bns_get_seq: bases of [beg, end) from a 2-bit packed reference (4 bases per byte, first base in the top bits);
 * returns the number of bases written, 0 if the range bridges the forward/reverse boundary */
int64_t  bsw_pac_get_seq(int64_t l_pac, const uint8_t *pac, int64_t beg, int64_t end, uint8_t *dst);

/* ---- seeds against a DEVICE-RESIDENT reference: the 2-bit pac is uploaded once, the
 * extension targets are fetched on the GPU (bns_get_seq semantics, both strands, left side reversed),
 * so only the reads travel over PCIe. ---- */
typedef struct bsw_ref bsw_ref;
typedef struct bsw_ref_task {
    const uint8_t *query;   /* the whole read, codes 0..4                                  */
    int32_t  l_query;
    int32_t  init_score;    /* -1 in bwa                                                    */
    bsw_seed seed;          /* rbeg in [0, 2*l_pac), qbeg, len                              */
    int64_t  rmax0, rmax1;  /* reference window of the chain (bsw_chain_window)             */
    uint32_t tag;
    uint32_t _pad;
} bsw_ref_task;
int      bsw_ref_upload(bsw_ctx *ctx, const uint8_t *pac, int64_t l_pac, bsw_ref **out);
void     bsw_ref_free(bsw_ctx *ctx, bsw_ref *ref);
/* device-resident batch whose targets come from `ref`; then bsw_run / bsw_download as usual */
int      bsw_upload_ref(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ref_task *tasks, size_t n, bsw_dev_batch **out);
/* streaming form (like bsw_submit; finish with bsw_wait): chunk k -> device k mod n_devices, every device holding
 * its own copy of the reference (bsw_ref_upload puts one on each GPU of the context).  Only the reads cross PCIe
 * (~1/2.5 of the bytes of bsw_submit at 150 bp); reads in bsw_host_alloc / registered memory are DMA'd as they are. */
int      bsw_submit_ref(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ref_task *tasks, size_t n, bsw_result *out);
int      bsw_submit_ref_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ref_task *tasks, size_t n, bsw_result *out, bsw_ticket *ticket);
/* convenience: upload_ref + run + download + free (synchronous) */
int      bsw_extend_ref(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ref_task *tasks, size_t n, bsw_result *out);

/* ---- RESIDENT READ BLOCKS: the reads of a block are uploaded once and the three Smith-Waterman stages name a read by its
 * index, so that only coordinates cross PCIe: seed extension (bsw_submit_reads_t), mate rescue (bsw_matesw_reads_submit_t) and
 * CIGAR generation (bsw_cigar_reads_submit_t) against the resident reference AND the resident reads.  The pointer forms send the
 * same read up to three times (whole, as a mate per rescue task, as &query[qb] slices) and look at every sequence pointer of a
 * chunk on the host (span, registration, gather); these forms send 76 - 112 bytes of records per task whatever the read length.
 * bsw_pack_kernel takes the query words out of the 4-bit store (a funnel shift over two words, backwards for the left flank and
 * the reverse-strand CIGAR read); every kernel behind it reads the same `seq` as before.
 * A block goes up in one of two ways: bsw_reads_upload packs it on the caller's thread and returns when every device has its
 * copy; bsw_reads_upload_start returns at once, sends the reads across as they lie and packs them on the GPU, and the tickets
 * that name the block wait for it ON THE DEVICE.  Both make the same image. ---- */
typedef struct bsw_reads bsw_reads;
/* reads[i]: lens[i] bases, codes 0..4 (larger codes stored as 4), any host memory.  A 4-bit packed copy (the device sequence
 * format, every read on a word boundary, zeroed slack words in front and behind) is placed on every device of the context, as
 * bsw_ref_upload does for the reference.  Synchronous: the copies are complete and reads[] may be freed when it returns; it
 * copies on a stream of its own per device, so it neither waits for nor holds up tickets in flight.
 * BSW_E_INVAL: lens[i] < 0, a NULL read of non-zero length; BSW_E_LIMIT: lens[i] > 65 535, or a block whose base positions do
 * not fit 32 bits (more than 2^28 - 2^13 packed words = ~4.29 G bases of word-aligned reads).  A failed upload leaves no copy on
 * any device.  n_reads == 0 is a valid, empty block. */
int      bsw_reads_upload(bsw_ctx *ctx, const uint8_t *const *reads, const int32_t *lens, size_t n_reads, bsw_reads **out);
/* The ASYNCHRONOUS upload.  The argument and per-read checks of bsw_reads_upload run in the caller's thread, with the same codes;
 * the {offset, length} table is built and the device copies are reserved; the transfer is queued on every device and the call
 * returns.  When a check or a reservation fails no block is made, nothing is queued and no device keeps anything.
 *   - *out may be handed to bsw_submit_reads_t, bsw_matesw_reads_submit_t and bsw_cigar_reads_submit_t AT ONCE: their checks need
 *     only the table, and on every device the first kernel of each of their chunks that reads the block runs after that device's
 *     copy is complete (ordered on the GPU; the host does not wait for the copy).
 *   - reads[] and lens[] may be freed when the call returns; the BASES they point to stay valid and unchanged until the block is
 *     ready (bsw_reads_test == 1 / bsw_reads_wait returned).  Bases in registered memory (bsw_host_alloc / bsw_host_register) are
 *     DMA'd as they lie; anything else is gathered into pinned staging by the context's slot threads.
 *   - An upload is not a submit: no ticket, no place among BSW_MAX_INFLIGHT, not counted by bsw_inflight, not collected by
 *     bsw_wait.  At most 2 uploads per context are in flight (block k+1 goes up while block k's tickets and upload are still
 *     about); one more answers BSW_E_BUSY and changes nothing.  A block without a base (n_reads == 0 included) is ready at once.
 *   - A failed upload (bsw_reads_wait / bsw_reads_test say so) fails every chunk that names the block with BSW_E_HIP before it
 *     launches anything that reads the block; other tickets are left alone.  bsw_reads_free then frees what there is.
 *   - bsw_reads_free answers BSW_E_BUSY while the upload is in flight; bsw_destroy waits for it, as it does for tickets. */
int      bsw_reads_upload_start(bsw_ctx *ctx, const uint8_t *const *reads, const int32_t *lens, size_t n_reads, bsw_reads **out);
/* UPLOAD ENCODINGS.  A host holds its reads as codes only after a conversion pass; the _enc forms of the two uploads take them
 * as they lie at two other moments.  lens[] stays in BASES whatever the encoding, and the block is THE SAME IMAGE: reads that
 * spell the same bases give, word for word, the device copy bsw_reads_upload makes of their codes, slack words included, so
 * nothing behind the upload changes.  The two calls above are the _enc calls with BSW_READS_CODES; everything said there — the
 * threading rules, at most 2 uploads in flight, tickets ordered behind the upload on the device, bsw_reads_test / _wait / _image /
 * _free / _info, the failure rules, 65 535 bases per read and 2^28 - 2^13 words per block — holds for them word for word.
 *   BSW_READS_ASCII   FASTQ letters, as a reader thread hands a block over: A a -> 0, C c -> 1, G g -> 2, T t -> 3, EVERY other
 *                     byte value -> 4 (N n, IUPAC letters, '-', U, and the bytes 0..4 themselves).  No byte is an error.
 *   BSW_READS_PACKED  the device's own format, as bsw_pack_bases writes it: reads[i] addresses ceil(lens[i] / 16) uint64 words,
 *                     all of them readable.  Nibbles 0..3 are stored as they are, 4..15 as 4; the nibbles behind a read's last
 *                     base may hold anything and come out zero.  A read of non-zero length whose pointer is not 8-byte aligned
 *                     is refused: BSW_E_INVAL, the text names the read, no block is made.
 *   any other value   BSW_E_INVAL; nothing is allocated or queued.
 * A read's RAW bytes are lens[i] for the byte encodings and 8 * ceil(lens[i] / 16) for the packed one: that is what crosses
 * PCIe per read and device (plus a 16-byte record on the asynchronous path), what bsw_host_stats.h2d_bytes grows by, and what
 * the asynchronous upload cuts its pieces by.  Letters are translated, and words clamped and masked, by the GPU kernel that
 * packs the codes form (bsw_reads_upload_start_enc) or on the caller's thread (bsw_reads_upload_enc). */
#define BSW_READS_CODES   0   /* one byte per base, codes 0..4, larger stored as 4: the form of the two calls above */
#define BSW_READS_ASCII   1   /* one byte per base, FASTQ letters */
#define BSW_READS_PACKED  2   /* reads[i] addresses uint64 words, 16 bases each, base k in bits [4k, 4k+3] */
int      bsw_reads_upload_enc(bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int encoding, bsw_reads **out);
int      bsw_reads_upload_start_enc(bsw_ctx *ctx, const void *const *reads, const int32_t *lens, size_t n_reads, int encoding, bsw_reads **out);
/* 1: the block is ready, 0: its upload is in flight, < 0: the upload's failure.  Never blocks. */
int      bsw_reads_test(bsw_ctx *ctx, const bsw_reads *rd);
/* blocks until the upload is over (the watchdog of every wait applies) and returns its error code; may be called again */
int      bsw_reads_wait(bsw_ctx *ctx, bsw_reads *rd);
/* tests and tools: device k's copy of a READY block, slack words included (bsw_reads_info's device_bytes / 8 words), into
 * words[0 .. cap_words).  Synchronous; BSW_E_BUSY while the upload is in flight, BSW_E_INVAL for too small a buffer. */
int      bsw_reads_image(bsw_ctx *ctx, const bsw_reads *rd, int k, uint64_t *words, size_t cap_words);
/* BSW_E_BUSY while a ticket that has not been collected uses rd, or while its upload is in flight (nothing is freed then); BSW_E_INVAL for a block of another
 * context.  rd == NULL is BSW_OK. */
int      bsw_reads_free(bsw_ctx *ctx, bsw_reads *rd);
/* reads, bases, and the bytes ONE device copy holds (slack included); any pointer may be NULL */
int      bsw_reads_info(const bsw_reads *rd, uint64_t *n_reads, uint64_t *bases, uint64_t *device_bytes);

typedef struct bsw_rd_task {         /* bsw_ref_task with query = reads[read], l_query = lens[read] */
    uint32_t read;
    int32_t  init_score;
    bsw_seed seed;
    int64_t  rmax0, rmax1;
    uint32_t tag, _pad;
} bsw_rd_task;                       /* 48 bytes */
typedef struct bsw_rd_mtask {        /* bsw_mtask with mate = reads[read], l_ms = lens[read] */
    uint32_t read;
    int32_t  is_rev;
    int64_t  rb, re;
    int32_t  xtra, min_score;
} bsw_rd_mtask;                      /* 32 bytes */
typedef struct bsw_rd_ctask {        /* bsw_ctask with query = reads[read] + qb, l_query = qe - qb */
    uint32_t read;
    int32_t  qb, qe, w;
    int64_t  rb, re;
    int32_t  w_cap, min_score, max_tries, _pad;
} bsw_rd_ctask;                      /* 48 bytes */
/* Tickets of the context's pipeline under the contract of bsw_cigar_ref_submit_t (one ticket space, BSW_MAX_INFLIGHT, chunk k on
 * device k mod n_devices against that device's copies of the reference and of the reads).  Results are, byte for byte, those of
 * bsw_submit_ref_t (BSW_RESULT_PAIR included) / bsw_matesw_ref_submit_t / bsw_cigar_ref_submit_t for the same read bytes.
 * ALL checks run in the caller's thread before anything is queued, and no ticket is made when one fails: the pointer form's
 * checks with its codes and texts (for extension also those the pointer form reports from the wait), read >= n_reads ->
 * BSW_E_INVAL, a CIGAR task with qb < 0, qe < qb or qe > lens[read] -> BSW_E_INVAL, a block uploaded through another context ->
 * BSW_E_INVAL.  tasks[] and the result arrays stay valid, and rd stays allocated, until the ticket is collected. */
int      bsw_submit_reads_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd, const bsw_rd_task *tasks,
                            size_t n, bsw_result *out, bsw_ticket *ticket);
int      bsw_matesw_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd,
                                   const bsw_rd_mtask *tasks, size_t n, bsw_mresult *res, bsw_ticket *ticket);
int      bsw_cigar_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd,
                                  const bsw_rd_ctask *tasks, size_t n, int max_cigar, uint32_t *cigars, int max_md, char *md,
                                  bsw_cresult *res, bsw_ticket *ticket);

/* ---- mem_chain2aln itself (bwamem.c of bwa 0.7.12 - 0.7.17, restated AS RECALLED: bwa's source is not in this tree):
 * the loop that DRIVES the seed extension.  Per read bwa keeps one growing list av of regions, shared by the read's chains.  It
 * visits a chain's seeds by score (srt[i] = (uint64)score << 32 | i sorted ascending, walked from the top: highest score first,
 * the larger index first among equal scores), SKIPS a seed that an earlier region of the read explains — the seed lies inside
 * the region on both axes, is not more than 0.1 * l_query longer than the seed the region grew from, and sits within
 * min(cal_max_gap, region.w) of the region's diagonal ahead of or behind it — UN-SKIPS it when a seed of the same chain that was
 * visited earlier and not skipped, at least 0.95 times as long, overlaps it on the query by len >> 2 or more on another
 * diagonal, and stamps every region with seedcov, seedlen0, rid and frac_rep.  A region per seed is NOT bwa's output.
 * The extension of a seed does not depend on av, only the decision to run it does: bsw_chain2aln_plan makes a task of EVERY
 * seed, the existing extension path runs them, and bsw_chain2aln_replay walks bwa's loop with the results at hand.  The
 * result of a skipped seed is never read; regs[] is bwa's av, in bwa's push order.  What the speculation costs: README.
 * The skip mark is the VALUE 0 in srt[], as in bwa, so (score 0, index 0) reads as skipped; with scores >= 0 that entry is
 * visited last and nothing reads it afterwards, so the quirk is kept and has no effect.  Negative scores are refused.
 * A host of the bwa-0.7.8 era passes score = len and seedlen0_frac < 0. ---- */
typedef struct bsw_cseed {           /* mem_seed_t with its score */
    int64_t rbeg;
    int32_t qbeg, len, score, _pad;
} bsw_cseed;                         /* 24 bytes */
typedef struct bsw_chain {           /* mem_chain_t: seeds[first_seed, first_seed + n_seeds) */
    uint32_t read;                   /* the chains are sorted by read (a read's chains contiguous), in bwa's order inside a read (after mem_chain_flt) */
    int32_t  n_seeds;
    uint64_t first_seed;             /* chain k's seeds follow chain k-1's: seeds[] is the chains' seeds laid end to end */
    int64_t  rlo, rhi;               /* the chain's contig in [0, 2*l_pac) coordinates (forward: [offset, offset + len), reverse: mirrored); the
                                        window is clamped into it as bns_fetch_seq does.  rhi <= rlo: no clamp */
    int32_t  rid;                    /* copied into the regions */
    float    frac_rep;
} bsw_chain;                         /* 40 bytes */
typedef struct bsw_creg {            /* the fields of mem_alnreg_t that mem_chain2aln writes */
    int64_t  rb, re;
    int32_t  qb, qe, score, truesc, w;
    int32_t  seedcov;                /* sum of len over ALL seeds of the chain inside the region on both axes, skipped ones too */
    int32_t  seedlen0;               /* length of the seed the region grew from */
    int32_t  rid;
    float    frac_rep;
    uint32_t read, chain, seed;      /* where it came from: indices into lens[] / chains[] / seeds[] */
} bsw_creg;                          /* 64 bytes */
typedef struct bsw_c2a_opt {
    double seedlen0_frac;            /* .1: a region does not explain a seed with len - seedlen0 > seedlen0_frac * l_query; < 0: test off (bwa 0.7.8) */
    double ovl_len_frac;             /* .95: only a seed t with t.len >= ovl_len_frac * s.len can un-skip s */
} bsw_c2a_opt;
typedef struct bsw_c2a_stats {
    uint64_t seeds_gpu;              /* seeds extended on the GPU: all of them */
    uint64_t seeds_bwa;              /* seeds bwa would have extended = regions pushed (0 before the replay) */
    uint64_t regs;
    uint64_t chains, reads;
} bsw_c2a_stats;
void     bsw_c2a_default_opt(bsw_c2a_opt *o);
/* Pure host.  One task per seed, in seed order: tag = the seed's index in seeds[], init_score = -1, the window of its chain
 * (bsw_chain_window, then the chain's contig clamp).  rd_tasks[n_seeds] and ref_tasks[n_seeds] may each be NULL; ref_tasks needs
 * reads[n_reads] (the pointers it stores).  lens[read] = l_query.  err (may be NULL) receives the text of a failure.
 * BSW_E_INVAL: a seed outside its read or outside [0, 2*l_pac), a negative score, a chain without seeds or of a read >= n_reads,
 * chains not sorted by read (the chains of a read not contiguous), seeds[] not the chains' seeds end to end, a seed outside its
 * chain's clamped window; BSW_E_LIMIT: a window side (reference bases left or right of a seed) beyond BSW_MAX_TLEN. */
int      bsw_chain2aln_plan(const bsw_params *p, int64_t l_pac, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                            const int32_t *lens, size_t n_reads, const uint8_t *const *reads, bsw_rd_task *rd_tasks, bsw_ref_task *ref_tasks,
                            char *err, size_t err_cap);
/* Pure host, one thread.  results[i] = the record of seed i (the plan's task order): bsw_result[] for BSW_RESULT_FULL, bsw_pair[] for
 * BSW_RESULT_PAIR (the pair record holds everything the replay reads).  opt == NULL: the defaults.  Writes regs[0 .. *n_regs)
 * (capacity n_seeds): the reads in order, a read's regions contiguous and in bwa's push order; extended[n_seeds] (may be NULL): 1
 * where bwa runs the extension; reg_start[n_reads + 1] (may be NULL): read r's regions are regs[reg_start[r], reg_start[r + 1]). */
int      bsw_chain2aln_replay(const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds,
                              size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs,
                              size_t *n_regs, uint8_t *extended, uint64_t *reg_start);
/* The two as ONE JOB of the ticket pipeline, in place of the extension ticket: start = plan, the task and result arrays in
 * DMA-able memory (bsw_host_alloc), bsw_submit_ref_t / bsw_submit_reads_t; finish = bsw_wait_ticket, replay, free.  The job is one
 * of the context's BSW_MAX_INFLIGHT submits (one more answers BSW_E_BUSY and leaves no job), runs over every device of the
 * context and reads the context's result_format.  A failed start leaves *job NULL and queues nothing; its code is the plan's or
 * the submit's (a flank beyond BSW_MAX_QLEN: the submit's BSW_E_LIMIT), the text is in bsw_last_error.  chains[], seeds[], lens[]
 * and the reads (the block) stay valid AND UNCHANGED until finish (they are checked once, by start's plan).  A start beside
 * BSW_MAX_INFLIGHT submits is refused before anything is allocated or planned.  n_seeds == 0 makes a job without a ticket that is complete at once.
 * finish replays on the caller's thread and up to bsw_config.pack_threads - 1 helpers (reads are independent: the block's reads are
 * split into parts of at least 1 024 seeds); bsw_chain2aln_replay itself runs on the calling thread alone.
 * bsw_chain2aln_test: 1 complete, 0 in flight, < 0 an error; never blocks.  bsw_chain2aln_finish returns the ticket's failure or the
 * replay's and frees the job WHATEVER it returns (job == NULL: BSW_E_INVAL); the arrays are bsw_chain2aln_replay's, stats (may be
 * NULL) receives the counts.  bsw_chain2aln_stats: the same counts of a job that has not been finished (seeds_bwa and regs are
 * 0 then: they are the replay's).  The calls may come from several threads, one job from one thread at a time. */
typedef struct bsw_c2a_job bsw_c2a_job;
int      bsw_chain2aln_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                                 const int32_t *lens, size_t n_reads, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                                 bsw_c2a_job **job);
int      bsw_chain2aln_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                                   const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds, bsw_c2a_job **job);
int      bsw_chain2aln_test(bsw_c2a_job *job);
int      bsw_chain2aln_finish(bsw_c2a_job *job, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start, bsw_c2a_stats *stats);
int      bsw_chain2aln_stats(const bsw_c2a_job *job, bsw_c2a_stats *stats);

/* ---- the replay on the GPU (opt-in; off unless asked for).  bsw_chain2aln_replay's loop as a kernel, one 16-lane row per read: the
 * kernel lives in a COMPANION library, libbwasw_c2a.so next to this one, which links against this library and hands it a launcher
 * when it is loaded; every entry point is here.  regs, n_regs, extended and reg_start are byte for byte bsw_chain2aln_replay's.
 *   bsw_c2a_device_load(path)   dlopen the companion (NULL: libbwasw_c2a.so in this library's own directory).  BSW_OK (also when a
 *                               launcher is registered already), or BSW_E_INVAL when the file or its registration is missing: the
 *                               text is bsw_c2a_device_error()'s (process-wide; the call has no context; a diagnostic that is
 *                               NOT thread-safe: read it from the thread that made the failing call, with no other load or switch call beside it).
 *   bsw_c2a_device_register     what the companion's constructor calls: INTERNAL to the pair of libraries.
 *   bsw_set_c2a_device(on) / bsw_c2a_device()   a process-wide switch, initially BSW_C2A_DEVICE=1 (which implies one
 *                               bsw_c2a_device_load(NULL) attempt on first use).  Turning it on without a registered launcher is
 *                               refused with BSW_E_INVAL and leaves it off.  A chain2aln job reads it ONCE, at start, in the caller's thread.
 *   bsw_chain2aln_replay_batch  synchronous, on the context's own lane (BSW_E_BUSY while any ticket is uncollected).  It needs a
 *                               registered launcher (BSW_E_INVAL) but not the switch.  The arrays are checked first, with
 *                               bsw_chain2aln_replay's codes; results may be pageable, registered memory is DMA'd where it lies.
 *   bsw_chain2aln_replay_submit_t   the same as a ticket: one ticket space and BSW_MAX_INFLIGHT with every other submit, chunk k on
 *                               device k mod n; every array (the outputs and stats included) stays the ticket's until it is
 *                               collected.  A failed ticket leaves *n_regs 0.
 * Chunks are ranges of chains cut between two reads, sized in seeds (BSW_C2A_DEV_CHUNK overrides the size: tests, measurements); a
 * read with a chain of more than 512 seeds (BSW_C2A_DEV_MAX_CHAIN) is replayed by the host routine on the thread that runs its
 * chunk and merged into place.  Per chunk the chain records, the seeds and the result records go up (32 or 96 bytes per seed
 * AGAIN: DESIGN.md §9) and 4 bytes per read, 64 per region and, when extended is asked for, 1 per seed come back.
 * With the switch on, a chain2aln job replays through such a ticket: bsw_chain2aln_test never blocks — once the extension ticket is
 * complete it collects it and submits the replay ticket (BSW_E_BUSY there is not test's error: it answers 0 and tries again on the
 * next call) and answers 1 when the replay ticket is complete.  bsw_chain2aln_finish does the same blocking; BSW_E_BUSY from it
 * means the BSW_MAX_INFLIGHT places are taken by other tickets: THE JOB STAYS INTACT and the caller calls again (bsw_sdp_finish's
 * contract); every other answer frees the job as before.  While either ticket is in flight the job is one submit, never two. ---- */
typedef struct bsw_c2a_dev_stats {
    uint64_t reads_gpu;              /* reads with a chain that the kernel replayed */
    uint64_t reads_host;             /* reads with a chain above BSW_C2A_DEV_MAX_CHAIN seeds: replayed on the host */
    uint64_t chunks;
    uint64_t h2d_bytes, d2h_bytes;
} bsw_c2a_dev_stats;
int      bsw_c2a_device_register(const void *ops);
int      bsw_c2a_device_load(const char *path);
const char *bsw_c2a_device_error(void);
int      bsw_set_c2a_device(int on);
int      bsw_c2a_device(void);
int      bsw_chain2aln_replay_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                                    const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results,
                                    int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start,
                                    bsw_c2a_dev_stats *stats);
int      bsw_chain2aln_replay_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                                       const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results,
                                       int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start,
                                       bsw_c2a_dev_stats *stats, bsw_ticket *ticket);

/* ---- mem_patch_reg (bwamem.c of bwa >= 0.7.10, restated AS RECALLED: bwa's source is not in this tree) against the resident
 * reference: may two regions a, b of one read be joined into one?  Pre-tests on the host (strand, colinearity, the band and
 * ratio limits), bwa_gen_cigar2 with n_cigar = 0, cigar = 0 — the SCORE of the banded global alignment of read[a.qb, b.qe)
 * against the reference [a.rb, b.re), band w_ through bwa_gen_cigar2's formula, both reversed on the reverse strand, the no-gap
 * shortcut when the spans agree and w_ == 0 — and the 0.90 test of that score against the two regions' scores.  No backtrack
 * matrix, no CIGAR, no NM / MD: 8 bytes per alignment come back.  mem_sort_dedup_patch's bookkeeping (a merged region changes
 * later pairs) is bsw_sdp_* below, a job around these tickets: INTEGRATION.md "Region patching". ---- */
typedef struct bsw_preg {            /* the fields of mem_alnreg_t that mem_patch_reg reads */
    int64_t  rb, re;
    int32_t  qb, qe, score, w;
} bsw_preg;                          /* 32 bytes */
typedef struct bsw_ptask {
    const uint8_t *query;            /* the WHOLE read, codes 0..4 */
    int32_t  l_query, _pad;
    bsw_preg a, b;                   /* a.rb <= b.rb, as bwa asserts */
} bsw_ptask;                         /* 80 bytes */
typedef struct bsw_rd_ptask {        /* bsw_ptask with query = reads[read], l_query = lens[read] */
    uint32_t read;
    int32_t  _pad;
    bsw_preg a, b;
} bsw_rd_ptask;                      /* 72 bytes */
typedef struct bsw_presult {
    int32_t score;                   /* mem_patch_reg's return value: > 0 exactly when bwa merges, else 0 */
    int32_t w;                       /* *_w (the band handed to bwa_gen_cigar2) whenever the alignment ran, else 0 */
    int32_t gscore;                  /* bwa_gen_cigar2's score whenever the alignment ran (status 0 or 2), else 0 */
    int32_t status;                  /* 0 merged; 1 not run (a pre-test returned 0, or bwa_gen_cigar2 has no alignment: the interval
                                        bridges l_pac or leaves [0, 2*l_pac)); 2 run, and the return value is 0 (ratio below 0.90f) */
} bsw_presult;                       /* 16 bytes */
/* Batched mem_patch_reg on the context's first device; opt->w is p->w.  The first malformed task rejects the call: NULL read of
 * non-zero length, a region with rb >= re or without 0 <= qb < qe <= l_query, a.rb > b.rb, a.w / b.w / p->w < 0,
 * a.score + b.score <= 0 -> BSW_E_INVAL; a task that PASSES the pre-tests with b.qe - a.qb > BSW_GLOBAL_MAX_QLEN or
 * b.re - a.rb > BSW_MAX_TLEN -> BSW_E_LIMIT (one that fails a pre-test is never limit-checked and never reaches the GPU). */
int      bsw_patch_ref_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, size_t n, bsw_presult *res);
/* The same as a TICKET of the context's pipeline: the contract of bsw_cigar_ref_submit_t, word for word (one ticket space,
 * BSW_MAX_INFLIGHT, the checks above in the caller's thread and no ticket when one fails, chunk k on device k mod n_devices,
 * BSW_E_BUSY changes nothing, n == 0 completes at once), with the results of bsw_patch_ref_batch byte for byte.  tasks[], the
 * reads and res stay valid until the ticket is collected; the reads form (read >= n_reads, a block of another context ->
 * BSW_E_INVAL; the regions are checked against lens[read]) holds its block until then: bsw_reads_free answers BSW_E_BUSY.
 * BSW_F4_PATCH_WORK replaces the work of a chunk (banded cells) for tests and measurements only. */
int      bsw_patch_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, size_t n, bsw_presult *res,
                                bsw_ticket *ticket);
int      bsw_patch_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd, const bsw_rd_ptask *tasks,
                                  size_t n, bsw_presult *res, bsw_ticket *ticket);
/* Host only, no GPU: the two halves around the alignment, for a caller's replay of mem_sort_dedup_patch and for tests.
 * bsw_patch_pretest: 1 when bwa reaches bwa_gen_cigar2, with *w (may be NULL) the band it hands over; 0 when bwa returns 0 before.
 * bsw_patch_decide: mem_patch_reg's return value for bwa_gen_cigar2's score gscore (gscore, or 0 below the 0.90f ratio). */
int      bsw_patch_pretest(const bsw_params *p, int64_t l_pac, const bsw_preg *a, const bsw_preg *b, int *w);
int      bsw_patch_decide(const bsw_preg *a, const bsw_preg *b, int gscore);

/* ---- mem_sort_dedup_patch (bwamem.c of bwa 0.7.12 - 0.7.17, restated AS RECALLED: bwa's source is not in this tree):
 * the first thing bwa does with a read's regions av, and the loop AROUND mem_patch_reg.  Per read with n > 1 regions: sort by re,
 * n_comp = 1, then for i = 1 .. n-1 (p = a[i]) descend j = i-1, i-2, ... (q = a[j]) WHILE p.rid == q.rid and
 * p.rb < q.re + max_chain_gap — the condition ends the descent, and it is evaluated again with the smaller p.rb a merge leaves —
 * skipping a q that was excluded (qe == qb).  A pair that overlaps by more than mask_level_redun of the shorter region on BOTH
 * axes (binary32 products and comparisons, as bwa's float option makes them) is redundant: the lower score is excluded (p: the
 * descent breaks; q otherwise, ties included).  Otherwise, when q.rb < p.rb and mem_patch_reg(q, p) > 0, q is merged into p:
 * p.n_comp += q.n_comp + 1, seedcov / sub / csub the maxima, p.qb = q.qb, p.rb = q.rb, score = truesc = the return value,
 * p.w = the band, q excluded.  Then the excluded regions are dropped, the rest sorted by score descending, rb, qb ascending, and
 * of a run with equal (score, rb, qb) only the first is kept.  A read with n <= 1 is returned untouched (n_comp included).
 * TIES.  bwa's two sorts are ks_introsort, which is not stable; here both are STABLE (equal keys keep their previous order).  A
 * host that wants bwa's own order among equal re passes opt.presorted = 1 and what its ks_introsort left.  Of a full
 * (score, rb, qb) tie the survivor may differ from bwa's in the fields outside the key (re, qe, w, seedcov, src, ...).
 * The loop is sequential and needs alignment scores in the middle, so it is a resumable replay: the engine below (pure host,
 * no context) asks for the mem_patch_reg pairs it needs as bsw_rd_ptask records, the patch tickets score them on the GPU, and a
 * merge that a later pair depends on costs one more (small) round.  The engine never aligns anything itself.
 * mem_sam_pe's second call after mate rescue (bns / pac / query NULL: mem_patch_reg returns 0 at once) is opt.patch = 0: no
 * task, no GPU; sub / csub then carry values. ---- */
typedef struct bsw_sreg {            /* the fields of mem_alnreg_t that mem_sort_dedup_patch reads or writes */
    int64_t  rb, re;
    int32_t  qb, qe, score, truesc, w, seedcov, sub, csub, rid, n_comp;
    uint32_t read;
    uint32_t src;                    /* output: the index in the caller's regs[] of the region this one WAS (the surviving p of its
                                        merges): bwa's struct copy carries p's other fields (seedlen0, frac_rep, ...) along.  Input: ignored */
} bsw_sreg;                          /* 64 bytes */
typedef struct bsw_sdp_opt {
    float   mask_level_redun;        /* .95f */
    int32_t max_chain_gap;           /* 10000 */
    int32_t patch;                   /* 1; 0: mem_patch_reg returns 0 (the call after mate rescue) */
    int32_t presorted;               /* 0; 1: regs[] is sorted by re inside every read already, keep its order among equal re */
} bsw_sdp_opt;                       /* 16 bytes */
typedef struct bsw_sdp_stats {
    uint64_t reads, regs_in, regs_out;
    uint64_t merges;
    uint64_t kills_p, kills_q;       /* regions excluded by the redundancy test: p (with the break), q */
    uint64_t dups;                   /* removed behind the second sort: equal (score, rb, qb) */
    uint64_t rounds;                 /* submits the block needed = the most any of its reads needed */
    uint64_t tasks_first, tasks;     /* mem_patch_reg pairs sent in round 1 / in all rounds */
    uint64_t alns_bwa;               /* mem_patch_reg calls that reach bwa_gen_cigar2 in bwa's sequential order */
} bsw_sdp_stats;                     /* 88 bytes */
void     bsw_sdp_default_opt(bsw_sdp_opt *o);
/* regs[i] of bsw_chain2aln_finish as a bsw_sreg: sub = csub = 0, n_comp = 0, src = i.  BSW_E_INVAL for a NULL array with n > 0. */
int      bsw_sdp_from_cregs(const bsw_creg *cregs, size_t n, bsw_sreg *sregs);
/* The engine.  regs[n_regs] sorted by read with reg_start[n_reads + 1] (read r's regions are regs[reg_start[r], reg_start[r + 1]):
 * what bsw_chain2aln_finish writes), lens[read] = l_query, p->w = opt->w of mem_patch_reg; opt == NULL: the defaults.  Everything
 * is checked ONCE, by open, which names the first offender in err (may be NULL).  BSW_E_INVAL: a region with rb >= re, without
 * 0 <= qb < qe <= lens[read] (qe == qb would read as "excluded"), w < 0, score <= 0, read not the one reg_start puts it in,
 * reg_start not ascending from 0 to n_regs, presorted with a descending re; BSW_E_LIMIT: more than 2^32 - 1 regions.  The arrays
 * are copied: the engine does not read them after open.
 * bsw_sdp_needs advances every unfinished read as far as the scores it holds allow and returns the pairs it now needs (a = q,
 * b = p; owned by the engine, valid until the next call); *n == 0: every read is finished.  The first call speculates: every
 * pair (i, j) of the sorted UNMODIFIED regions down to which the descent's condition holds, that is not redundant, has
 * q.rb < p.rb and passes bsw_patch_pretest.  A later call asks, per stalled read, for the pair it stalled on and for every
 * further j' below it under the same four conditions on the current states, excluded regions skipped.  bsw_sdp_feed takes the
 * results of exactly those tasks in that order (BSW_E_INVAL for another n).  A held result is used only when all twelve values
 * of (a, b) equal the task's it was computed for; status 1 counts as 0.  One round for a block without merges, one more per
 * merge that a later pair depends on; every round resolves at least one pair of every stalled read, so it ends.
 * bsw_sdp_collect (once *n == 0 was returned, BSW_E_INVAL before): out[] (capacity n_regs), the reads in order, bwa's order inside
 * a read; out_start[n_reads + 1] and stats may be NULL.  One engine belongs to one thread at a time; needs runs on the calling
 * thread alone (what it costs: README). */
typedef struct bsw_sdp_eng bsw_sdp_eng;
int      bsw_sdp_open(const bsw_params *p, const bsw_sdp_opt *opt, int64_t l_pac, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start,
                      const int32_t *lens, size_t n_reads, bsw_sdp_eng **eng, char *err, size_t err_cap);
int      bsw_sdp_needs(bsw_sdp_eng *eng, const bsw_rd_ptask **tasks, size_t *n);
int      bsw_sdp_feed(bsw_sdp_eng *eng, const bsw_presult *res, size_t n);
int      bsw_sdp_collect(bsw_sdp_eng *eng, bsw_sreg *out, size_t *n_out, uint64_t *out_start, bsw_sdp_stats *stats);
void     bsw_sdp_close(bsw_sdp_eng *eng);
/* The engine as ONE JOB around the patch tickets: start = open, the first needs, the tasks and results in DMA-able memory
 * (bsw_host_alloc), bsw_patch_ref_submit_t (query = reads[read]) / bsw_patch_reads_submit_t.  While a round is in flight the job
 * is one of the context's BSW_MAX_INFLIGHT submits and runs over every device of the context.  A failed start leaves *job NULL
 * and queues nothing (a start with something to submit beside BSW_MAX_INFLIGHT submits: BSW_E_BUSY before anything is allocated);
 * the text is in bsw_last_error.  With nothing to submit (patch = 0, no pair) the job is complete at once and holds no ticket.
 * regs[], reg_start[], lens[] and the reads (the block) stay valid and unchanged until finish.
 * bsw_sdp_test never waits for the GPU: when the round's ticket is complete it collects it, feeds the engine, takes the next
 * needs and submits them; 1 = the engine has finished, 0 = not yet (also when the follow-up submit answered BSW_E_BUSY: the next
 * call tries again), < 0 = the job has failed, and finish reports it.  bsw_sdp_finish does the same with bsw_wait_ticket until the
 * engine has finished, writes bsw_sdp_collect's arrays and frees the job WHATEVER it returns (job == NULL: BSW_E_INVAL) — with one
 * exception: when a follow-up round's submit answers BSW_E_BUSY (other threads hold the four places), finish returns BSW_E_BUSY
 * with the job intact and a later finish or test continues there; waiting inside the library could deadlock a caller that
 * itself holds the uncollected tickets.  bsw_sdp_job_stats: the counts so far of a job not yet finished.
 * A pair that passes the pre-tests but exceeds BSW_GLOBAL_MAX_QLEN / BSW_MAX_TLEN fails the job with the patch submit's
 * BSW_E_LIMIT; with the pre-tests' limits on w that needs a read beyond 8 191 bases.  The calls may come from several threads,
 * one job from one thread at a time. */
typedef struct bsw_sdp_job bsw_sdp_job;
int      bsw_sdp_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_sdp_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                           const int32_t *lens, size_t n_reads, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, bsw_sdp_job **job);
int      bsw_sdp_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_sdp_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                             const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, bsw_sdp_job **job);
int      bsw_sdp_test(bsw_sdp_job *job);
int      bsw_sdp_finish(bsw_sdp_job *job, bsw_sreg *out, size_t *n_out, uint64_t *out_start, bsw_sdp_stats *stats);
int      bsw_sdp_job_stats(const bsw_sdp_job *job, bsw_sdp_stats *stats);

/* ---- the mate-rescue loop of mem_sam_pe with mem_matesw inside it (bwamem_pair.c of bwa 0.7.12 - 0.7.17, restated AS RECALLED:
 * bwa's source is not in this tree), as a job around the rescue tickets above.
 * BLOCK AND PAIRS.  Reads 2k and 2k+1 of the block are mates; n_reads is even.  INPUT: the regions of every read as
 * bsw_sreg regs[n_regs] with reg_start[n_reads + 1] — what bsw_sdp_finish writes: bwa's order inside a read, score descending.
 * DIRECTIONS.  For a pair and i in {0, 1}: the anchors come from read i, ma is a private copy of read !i's regions, the mate ms
 * is read !i.  Direction i reads only the INITIAL regions of read i (bwa copies b[0] and b[1] before the first rescue) and
 * mutates only a[!i]: the two directions of a pair are independent replays.
 * ANCHORS.  Every j with regs[j].score >= regs[first of the read].score - pen_unpaired (a filter over all j, not a break), in
 * input order, the first max_matesw of them.  A read without regions has no anchor.
 * mem_matesw(anchor a, ma).  skip[r] = failed[r] != 0; for every region m of the current ma: r = bsw_infer_dir(l_pac, a.rb, m.rb,
 * &dist), and low[r] <= dist <= high[r] sets skip[r] = 1; all four set: return 0.  skip[] is computed once per anchor, before
 * its orientations.  Then for r = 0..3, not skipped: the window of bsw_matesw_windows; if rb < re the contig step below; the
 * orientation RUNS when the contig step passed, re - rb >= min_seed_len after the clamp and the task's result is not status == 1.
 * If it runs, ++n; if it runs with status == 0, b is built (rid = a.rid; rb / re / qb / qe / score / csub / seedcov from the
 * bsw_mresult; truesc = w = sub = n_comp = 0) and inserted into ma in front of the first region with score < b.score, or at the
 * end.  Then, inside the r loop, for every orientation that was not skipped, whether or not it ran: when n > 0,
 * ma = mem_sort_dedup_patch with patch = 0 (mask_level_redun, max_chain_gap of the options) — bsw_sdp's own per-read pass with
 * patch = 0, its two STABLE sorts on the order ma has at that moment; the TIES caveat of bsw_sdp_* above holds here verbatim: bwa's
 * two sorts are ks_introsort, which is not stable, and of a full (score, rb, qb) tie the survivor may differ from bwa's in the
 * fields outside the key (re, qe, w, seedcov, src, ...).  So ma shrinks as well as grows.
 * CONTIG STEP (bns_fetch_seq).  mid = (rb + re) >> 1; fwd = mid >= l_pac ? 2*l_pac - 1 - mid : mid; rid' = the contig whose
 * [offset, offset + len) holds fwd; the contig's interval on mid's strand is [offset, offset + len) when mid < l_pac and
 * [2*l_pac - offset - len, 2*l_pac - offset) otherwise; rb is clamped up and re down to it; the step passes when rid' == a.rid.
 * With n_contigs == 0 (a bwa-0.7.8 host) there is no clamp and no rid test: only the ticket's own status == 1 (a window that
 * bridges l_pac) then keeps an orientation from running.
 * TASK FIELDS.  xtra = KSW_XSUBO | KSW_XSTART | (l_ms * a < 250 ? KSW_XBYTE : 0) | (min_seed_len * a); min_score = min_seed_len.
 * EXACTNESS AND ROUNDS.  A task's result depends only on (anchor, r, mate, contigs), never on ma: a held result is never stale,
 * only WHETHER it is needed changes.  Round 1 asks for every (anchor, r) not skipped on the INITIAL ma whose clamped window
 * passes the contig and length tests.  The replay uses a result only when bwa's loop reaches that (anchor, r).  A rescued region
 * can make an initial region redundant and kill it; when that region was the only one that put a later anchor's orientation
 * inside [low, high], the loop reaches an (anchor, r) it has no result for and the direction stalls.  The next needs asks for
 * that (anchor, r), the rest of this anchor's orientations not in skip[], and for every later anchor every orientation not
 * skipped under the CURRENT ma and not already held.  Every round resolves at least the stalling task and no (anchor, r) is
 * ever asked twice, so it ends after at most 4 x anchors tasks per direction.
 * OUTPUT.  Per read its final ma (out[], out_start[n_reads + 1]); for a read that no rescue touched, its input regions unchanged.
 * src = the input index for an input region, BSW_RESCUE_NEW | the input index of the anchor for a rescued one (more than
 * 2^31 - 1 regions: BSW_E_LIMIT).  n_sw[n_reads / 2] (may be NULL) = bwa's n per pair, summed over both directions. ---- */
#define BSW_RESCUE_NEW 0x80000000u
typedef struct bsw_contig {          /* bntann1_t: the contig covers [offset, offset + len) of the forward strand */
    int64_t offset, len;
} bsw_contig;                        /* 16 bytes */
typedef struct bsw_rescue_opt {
    int32_t low[4], high[4], failed[4];   /* mem_pestat_t per orientation */
    int32_t pen_unpaired;            /* 17 */
    int32_t max_matesw;              /* 50 */
    int32_t min_seed_len;            /* 19 */
    int32_t a;                       /* 1: the match score (xtra's KSW_XBYTE test and threshold) */
    float   mask_level_redun;        /* .95f */
    int32_t max_chain_gap;           /* 10000 */
} bsw_rescue_opt;                    /* 72 bytes */
typedef struct bsw_rescue_stats {
    uint64_t pairs, anchors;
    uint64_t rounds;                 /* submits the block needed */
    uint64_t tasks_first, tasks;     /* windows sent in round 1 / in all rounds */
    uint64_t alns_bwa;               /* orientations that run in bwa's sequential order (the sum of n_sw[]) */
    uint64_t pushed;                 /* rescued regions inserted into some ma (before the pass that may remove them again) */
    uint64_t regs_in, regs_out;
    uint64_t late;                   /* tasks first asked after round 1: what a host that speculates once would have dropped */
} bsw_rescue_stats;                  /* 80 bytes */
/* Everything but the twelve pes values; ALL FOUR orientations are marked failed, so that a forgotten pes rescues nothing
 * rather than something wrong. */
void     bsw_rescue_default_opt(bsw_rescue_opt *o);
/* The engine (pure host, no context), under the contracts of the bsw_sdp_* engine: the arrays are copied at open, everything
 * is checked ONCE, by open, which names the first offender in err (may be NULL); p supplies nothing but is kept for the job;
 * lens[read] = the read's length (l_ms of a task whose mate it is).  BSW_E_INVAL: what bsw_sdp_open refuses in a region or in
 * reg_start; an odd n_reads; contigs that do not tile [0, l_pac) in ascending order; a rid outside the table when there is
 * one; low[r] > high[r] for an orientation that has not failed; negative pen_unpaired, max_matesw or min_seed_len; a < 1;
 * min_seed_len * a beyond 65535 (xtra's threshold is 16 bits).  BSW_E_LIMIT: more than 2^31 - 1 regions.
 * bsw_rescue_needs returns the tasks it now needs (owned by the engine, valid until the next call; read = the mate); *n == 0:
 * every direction is finished.  bsw_rescue_feed takes the results of exactly those tasks in that order (BSW_E_INVAL for another
 * n).  bsw_rescue_collect (once *n == 0 was returned, BSW_E_INVAL before): out[] needs room for bsw_rescue_out_capacity(eng) =
 * n_regs + 4 x anchors regions; out_start, n_sw and stats may be NULL.  One engine belongs to one thread at a time. */
typedef struct bsw_rescue_eng bsw_rescue_eng;
int      bsw_rescue_open(const bsw_params *p, const bsw_rescue_opt *opt, int64_t l_pac, const bsw_contig *contigs, size_t n_contigs,
                         const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, const int32_t *lens, size_t n_reads,
                         bsw_rescue_eng **eng, char *err, size_t err_cap);
int      bsw_rescue_needs(bsw_rescue_eng *eng, const bsw_rd_mtask **tasks, size_t *n);
int      bsw_rescue_feed(bsw_rescue_eng *eng, const bsw_mresult *res, size_t n);
int      bsw_rescue_collect(bsw_rescue_eng *eng, bsw_sreg *out, size_t *n_out, uint64_t *out_start, int32_t *n_sw, bsw_rescue_stats *stats);
size_t   bsw_rescue_out_capacity(const bsw_rescue_eng *eng);     /* 0 for NULL */
void     bsw_rescue_close(bsw_rescue_eng *eng);
/* The engine as ONE JOB around the rescue tickets, under the contract of bsw_sdp_*_start / _test / _finish / _job_stats above word
 * for word: start = open, the first needs, the tasks and results in DMA-able memory (bsw_host_alloc), bsw_matesw_ref_submit_t
 * (bsw_rd_mtask turned into bsw_mtask with mate = reads[read], l_ms = lens[read]) / bsw_matesw_reads_submit_t.  A round is one
 * of the context's BSW_MAX_INFLIGHT submits and runs over every device of the context.  A failed start leaves *job NULL and
 * queues nothing (beside BSW_MAX_INFLIGHT submits: BSW_E_BUSY before anything is allocated); with nothing to submit the job is
 * complete at once and holds no ticket.  regs[], reg_start[], lens[], contigs[] and the reads (the block) stay valid and
 * unchanged until finish.  bsw_rescue_test never waits: 1 = finished, 0 = not yet (also when the follow-up submit answered
 * BSW_E_BUSY), < 0 = the job has failed, and finish reports it.  bsw_rescue_finish waits until the engine has finished, writes
 * collect's arrays (out_cap regions of room: bsw_rescue_job_out_capacity is always enough, fewer than the job's final count is
 * BSW_E_INVAL) and frees the job WHATEVER it returns (job == NULL: BSW_E_INVAL), except that a follow-up round that finds no place
 * answers BSW_E_BUSY with the job intact.  The limits are the rescue submit's own and fail the job with its text: a mate
 * beyond BSW_ALIGN_MAX_QLEN bases without bsw_set_align_long, a window beyond BSW_MAX_TLEN.  The calls may come from several
 * threads, one job from one thread at a time. */
typedef struct bsw_rescue_job bsw_rescue_job;
int      bsw_rescue_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_rescue_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                              const int32_t *lens, size_t n_reads, const bsw_contig *contigs, size_t n_contigs, const bsw_sreg *regs,
                              size_t n_regs, const uint64_t *reg_start, bsw_rescue_job **job);
int      bsw_rescue_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_rescue_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                                const bsw_contig *contigs, size_t n_contigs, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start,
                                bsw_rescue_job **job);
int      bsw_rescue_test(bsw_rescue_job *job);
int      bsw_rescue_finish(bsw_rescue_job *job, bsw_sreg *out, size_t out_cap, size_t *n_out, uint64_t *out_start, int32_t *n_sw,
                           bsw_rescue_stats *stats);
int      bsw_rescue_job_stats(const bsw_rescue_job *job, bsw_rescue_stats *stats);
size_t   bsw_rescue_job_out_capacity(const bsw_rescue_job *job); /* 0 for NULL */

/* ---- device sequence format: 4 bits per base, 16 bases per uint64, base k of a word in bits [4k,4k+3];
 * codes > 4 are stored as 4 (N).  words must hold (len+15)/16 entries.  Returns 1 if an N was seen. ---- */
int      bsw_pack_bases(const uint8_t *bases, int len, uint64_t *words);

/* ---- synthetic workload generator (no genome in the image) --- */
typedef struct bsw_synth_spec {
    uint64_t seed;
    int32_t  read_len;      /* 150 or 250                                        */
    int32_t  seed_len_min, seed_len_max; /* seed length ~ U[min,max]             */
    int32_t  seed_at_start; /* 1: seed = read[0:seed_len) (right extension only) */
    double   sub_rate, indel_rate;       /* per-base                             */
    double   n_rate;        /* fraction of bases turned into N                    */
    double   junk_frac;     /* fraction of tasks whose flanks are unrelated       */
    int32_t  a;             /* match score (for h0 = seed_len*a)                  */
    int32_t  w;             /* band, caps tlen = qlen + min(max_gap, 2w)          */
    int32_t  o, e;          /* gap penalties for cal_max_gap                      */
} bsw_synth_spec;
/* Fills tasks[0..n) and the arena; returns bytes of arena used or <0.          */
int64_t  bsw_synth_generate(const bsw_synth_spec *s, size_t n, bsw_task *tasks, uint8_t *arena, size_t arena_len);
size_t   bsw_synth_arena_bound(const bsw_synth_spec *s, size_t n);
/* Synthetic GENOME + reads for the device-resident-reference path: fills pac ((l_pac+3)/4 bytes, bwa's .pac layout)
 * with i.i.d. bases and tasks[0..n) with forward-strand reads of read_len bases (arena: n*read_len bytes), each with
 * one exact seed and flanks derived from the genome at the spec's error rates; rmax = bsw_chain_window of the seed. */
int64_t  bsw_synth_ref_generate(const bsw_synth_spec *s, const bsw_params *p, int64_t l_pac, uint8_t *pac, size_t n,
                                bsw_ref_task *tasks, uint8_t *arena, size_t arena_len);

#ifdef __cplusplus
}
#endif
#endif /* BWA_SW_MI355_H */
