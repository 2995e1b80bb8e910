"""Host-side mirror of the reference's operator interface, over the C ABI (ctypes).

Names follow the reference's domain: a *task batch* of seeds goes in, a *result batch*
comes out (batch_manager.v / tbb.v / rbb.v); PARAMS = global words G0/G1, TASK = header
H0..H7, RESULT = record R0..R4 (sw_pe_array_proc_element.v:807-933, :1662-1665).
numpy structured dtypes below are byte-for-byte the C structs of include/bwa_sw_mi355.h.
"""
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("BSW_LIB_PATH") or os.path.join(_HERE, "libbwasw_mi355.so")   # BSW_LIB_PATH: an experimental build (tools only)

PARAMS = np.dtype([("mat", "i1", (25,)), ("_pad", "i1", (3,)), ("o_del", "<i4"), ("e_del", "<i4"),
                   ("o_ins", "<i4"), ("e_ins", "<i4"), ("w", "<i4"), ("pen_clip5", "<i4"),
                   ("pen_clip3", "<i4"), ("zdrop", "<i4"), ("max_band_try", "<i4"), ("variant", "<i4")])
TASK = np.dtype([("lquery", "<u8"), ("ltarget", "<u8"), ("rquery", "<u8"), ("rtarget", "<u8"),
                 ("lqlen", "<i4"), ("ltlen", "<i4"), ("rqlen", "<i4"), ("rtlen", "<i4"),
                 ("h0", "<i4"), ("init_score", "<i4"), ("qbeg", "<i4"), ("tag", "<u4"),
                 ("wlim_l", "<i4"), ("wlim_r", "<i4")])
EXT = np.dtype([("score", "<i4"), ("qle", "<i4"), ("tle", "<i4"), ("gtle", "<i4"), ("gscore", "<i4"),
                ("max_off", "<i4"), ("aw", "<i4"), ("cells", "<u4")])
RESULT = np.dtype([("tag", "<u4"), ("qb", "<i4"), ("qe", "<i4"), ("rb", "<i4"), ("re", "<i4"),
                   ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4"), ("left", EXT), ("right", EXT)])
EXT_TASK = np.dtype([("query", "<u8"), ("target", "<u8"), ("qlen", "<i4"), ("tlen", "<i4"),
                     ("w", "<i4"), ("end_bonus", "<i4"), ("h0", "<i4"), ("_pad", "<i4")])
SYNTH = np.dtype([("seed", "<u8"), ("read_len", "<i4"), ("seed_len_min", "<i4"), ("seed_len_max", "<i4"),
                  ("seed_at_start", "<i4"), ("sub_rate", "<f8"), ("indel_rate", "<f8"), ("n_rate", "<f8"),
                  ("junk_frac", "<f8"), ("a", "<i4"), ("w", "<i4"), ("o", "<i4"), ("e", "<i4")])
SEED = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])
ALNREG = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("truesc", "<i4"),
                   ("w", "<i4"), ("_pad", "<i4")])
GTASK = np.dtype([("query", "<u8"), ("target", "<u8"), ("qlen", "<i4"), ("tlen", "<i4"), ("w", "<i4"), ("_pad", "<i4")])
GRESULT = np.dtype([("score", "<i4"), ("n_cigar", "<i4")])
CTASK = np.dtype([("query", "<u8"), ("l_query", "<i4"), ("w", "<i4"), ("rb", "<i8"), ("re", "<i8"), ("w_cap", "<i4"),
                  ("min_score", "<i4"), ("max_tries", "<i4"), ("_pad", "<i4")])
CRESULT = np.dtype([("score", "<i4"), ("n_cigar", "<i4"), ("nm", "<i4"), ("md_len", "<i4"), ("w", "<i4"), ("tries", "<i4"),
                    ("status", "<i4"), ("_pad", "<i4")])
ATASK = np.dtype([("query", "<u8"), ("target", "<u8"), ("qlen", "<i4"), ("tlen", "<i4"), ("xtra", "<i4"), ("_pad", "<i4")])
KSWR = np.dtype([("score", "<i4"), ("te", "<i4"), ("qe", "<i4"), ("score2", "<i4"), ("te2", "<i4"), ("tb", "<i4"), ("qb", "<i4")])
KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
MTASK = np.dtype([("mate", "<u8"), ("l_ms", "<i4"), ("is_rev", "<i4"), ("rb", "<i8"), ("re", "<i8"), ("xtra", "<i4"),
                  ("min_score", "<i4")])
MRESULT = np.dtype([("aln", KSWR), ("status", "<i4"), ("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"),
                    ("score", "<i4"), ("csub", "<i4"), ("seedcov", "<i4"), ("_pad", "<i4")], align=True)
REF_TASK = np.dtype([("query", "<u8"), ("l_query", "<i4"), ("init_score", "<i4"), ("seed", SEED),
                     ("rmax0", "<i8"), ("rmax1", "<i8"), ("tag", "<u4"), ("_pad", "<u4")])
# resident read blocks (bsw_reads_upload): the three stages' tasks name a read by its index
RD_TASK = np.dtype([("read", "<u4"), ("init_score", "<i4"), ("seed", SEED), ("rmax0", "<i8"), ("rmax1", "<i8"),
                    ("tag", "<u4"), ("_pad", "<u4")])
RD_MTASK = np.dtype([("read", "<u4"), ("is_rev", "<i4"), ("rb", "<i8"), ("re", "<i8"), ("xtra", "<i4"), ("min_score", "<i4")])
RD_CTASK = np.dtype([("read", "<u4"), ("qb", "<i4"), ("qe", "<i4"), ("w", "<i4"), ("rb", "<i8"), ("re", "<i8"),
                     ("w_cap", "<i4"), ("min_score", "<i4"), ("max_tries", "<i4"), ("_pad", "<i4")])
assert RD_TASK.itemsize == 48 and RD_MTASK.itemsize == 32 and RD_CTASK.itemsize == 48
# mem_patch_reg (bsw_patch_ref_batch): the fields it reads of two regions of one read
PREG = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("w", "<i4")])
PTASK = np.dtype([("query", "<u8"), ("l_query", "<i4"), ("_pad", "<i4"), ("a", PREG), ("b", PREG)])
RD_PTASK = np.dtype([("read", "<u4"), ("_pad", "<i4"), ("a", PREG), ("b", PREG)])
PRESULT = np.dtype([("score", "<i4"), ("w", "<i4"), ("gscore", "<i4"), ("status", "<i4")])
assert PREG.itemsize == 32 and PTASK.itemsize == 80 and RD_PTASK.itemsize == 72 and PRESULT.itemsize == 16
# mem_chain2aln (bsw_chain2aln_*): a chain's seeds with their scores, the chains of a read block, the regions bwa pushes
CSEED = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"), ("_pad", "<i4")])
CHAIN = np.dtype([("read", "<u4"), ("n_seeds", "<i4"), ("first_seed", "<u8"), ("rlo", "<i8"), ("rhi", "<i8"), ("rid", "<i4"),
                  ("frac_rep", "<f4")])
CREG = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4"),
                 ("seedcov", "<i4"), ("seedlen0", "<i4"), ("rid", "<i4"), ("frac_rep", "<f4"), ("read", "<u4"), ("chain", "<u4"),
                 ("seed", "<u4")])
C2A_OPT = np.dtype([("seedlen0_frac", "<f8"), ("ovl_len_frac", "<f8")])
C2A_STATS = np.dtype([("seeds_gpu", "<u8"), ("seeds_bwa", "<u8"), ("regs", "<u8"), ("chains", "<u8"), ("reads", "<u8")])
C2A_DEV_STATS = np.dtype([("reads_gpu", "<u8"), ("reads_host", "<u8"), ("chunks", "<u8"), ("h2d_bytes", "<u8"), ("d2h_bytes", "<u8")])
C2A_DEV_MAX_CHAIN = 512        # BSW_C2A_DEV_MAX_CHAIN: a read with a longer chain is replayed on the host
assert CSEED.itemsize == 24 and CHAIN.itemsize == 40 and CREG.itemsize == 64 and C2A_OPT.itemsize == 16 and C2A_STATS.itemsize == 40
# mem_sort_dedup_patch (bsw_sdp_*): the fields of a region it reads or writes, its options and its counts
SREG = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4"),
                 ("seedcov", "<i4"), ("sub", "<i4"), ("csub", "<i4"), ("rid", "<i4"), ("n_comp", "<i4"), ("read", "<u4"), ("src", "<u4")])
SDP_OPT = np.dtype([("mask_level_redun", "<f4"), ("max_chain_gap", "<i4"), ("patch", "<i4"), ("presorted", "<i4")])
SDP_STATS = np.dtype([(k, "<u8") for k in ("reads", "regs_in", "regs_out", "merges", "kills_p", "kills_q", "dups", "rounds", "tasks_first",
                                           "tasks", "alns_bwa")])
assert SREG.itemsize == 64 and SDP_OPT.itemsize == 16 and SDP_STATS.itemsize == 88
# the mate-rescue loop of mem_sam_pe (bsw_rescue_*): the contig table, its options (mem_pestat_t and the mem_opt_t fields it reads), its counts
CONTIG = np.dtype([("offset", "<i8"), ("len", "<i8")])
RESCUE_OPT = np.dtype([("low", "<i4", (4,)), ("high", "<i4", (4,)), ("failed", "<i4", (4,)), ("pen_unpaired", "<i4"), ("max_matesw", "<i4"),
                       ("min_seed_len", "<i4"), ("a", "<i4"), ("mask_level_redun", "<f4"), ("max_chain_gap", "<i4")])
RESCUE_STATS = np.dtype([(k, "<u8") for k in ("pairs", "anchors", "rounds", "tasks_first", "tasks", "alns_bwa", "pushed", "regs_in", "regs_out",
                                              "late")])
RESCUE_NEW = 0x80000000
assert CONTIG.itemsize == 16 and RESCUE_OPT.itemsize == 72 and RESCUE_STATS.itemsize == 80
# how the reads of a block are encoded at its upload (BSW_READS_*): codes 0..4, FASTQ letters, 4-bit words
READS_CODES, READS_ASCII, READS_PACKED = 0, 1, 2
MAX_DEVICES = 16
CONFIG = np.dtype([("device", "<i4"), ("kernel", "<i4"), ("streams", "<i4"), ("pack_threads", "<i4"),
                   ("chunk_tasks", "<u8"), ("n_devices", "<i4"), ("devices", "<i4", (MAX_DEVICES,)),
                   ("timeout_ms", "<i4"), ("result_format", "<i4"), ("pin_threads", "<i4")])
STATS = np.dtype([("slot_cpu_ns", "<u8"), ("helper_cpu_ns", "<u8"), ("seeds", "<u8"), ("chunks", "<u8"), ("submits", "<u8"),
                  ("h2d_bytes", "<u8"), ("d2h_bytes", "<u8"), ("slot_threads", "<u8")])
MAX_INFLIGHT = 4
PAIR = np.dtype([("tag", "<u4"), ("qb", "<i4"), ("qe", "<i4"), ("rb", "<i4"), ("re", "<i4"),
                 ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4")])       # the RTL's 5-word record: the first 32 bytes of RESULT
RESULT_FULL, RESULT_PAIR = 0, 1
assert PARAMS.itemsize == 68 and TASK.itemsize == 72 and EXT.itemsize == 32 and RESULT.itemsize == 96
assert ATASK.itemsize == 32 and KSWR.itemsize == 28
assert CTASK.itemsize == 48 and CRESULT.itemsize == 32
assert MTASK.itemsize == 40 and MRESULT.itemsize == 72
assert EXT_TASK.itemsize == 40 and SYNTH.itemsize == 72 and CONFIG.itemsize == 104 and PAIR.itemsize == 32 and REF_TASK.itemsize == 56

REFBATCH_IN_WORDS, REFBATCH_OUT_WORDS, REFBATCH_MAX_TASKS = 65536, 4096, 819
KERNEL_AUTO, KERNEL_WAVE, KERNEL_LANE = 0, 1, 2
LANE_AUTO_MIN = 40000          # seeds of the 150 bp single bin (131-base sides) from which BSW_KERNEL_AUTO uses the lane bins: LANE_WORK_MIN = 5 M query bases per launched side (bsw_internal.h)
LANE_WORK_MIN, GROUP_WORK_MIN = 5_000_000, 1_500_000   # per launched side: lane kernels / the group kernel (bsw_lane2g_kernel) from this many query bases
VARIANT_H, VARIANT_M, VARIANT_RTL = 0, 1, 2

ERRORS = {0: "BSW_OK", -1: "BSW_E_NODEVICE", -2: "BSW_E_INVAL", -3: "BSW_E_LIMIT", -4: "BSW_E_HIP",
          -5: "BSW_E_NOMEM", -6: "BSW_E_BUSY"}


class BswError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d) %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code


def lib_path():
    return _LIB


def build_library(force=False):
    """Compile csrc/ for gfx950 into libbwasw_mi355.so (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(_LIB):
        subprocess.check_call(["make", "-j6", "-C", os.path.join(_HERE, "csrc")], stdout=subprocess.DEVNULL)
    return _LIB


_lib = None


def lib():
    """The C-ABI library.  Raises if it is missing: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise RuntimeError("libbwasw_mi355.so is not built (run __graft_entry__.build()); "
                               "this package has no CPU/PyTorch fallback")
        L = C.CDLL(_LIB)
        vp, sz = C.c_void_p, C.c_size_t
        sig = {
            "bsw_default_params": (None, [vp]), "bsw_default_config": (None, [vp]),
            "bsw_device_count": (C.c_int, []),
            "bsw_create": (C.c_int, [vp, C.POINTER(vp)]), "bsw_destroy": (None, [vp]),
            "bsw_create_sized": (C.c_int, [vp, sz, C.POINTER(vp)]), "bsw_abi_version": (C.c_int, []),
            "bsw_chain_timeouts": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
            "bsw_device_placement": (C.c_int, [vp, C.c_int, C.c_char_p, sz, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
            "bsw_last_error": (C.c_char_p, [vp]),
            "bsw_submit": (C.c_int, [vp, vp, vp, sz, vp]), "bsw_wait": (C.c_int, [vp]),
            "bsw_submit_packed": (C.c_int, [vp, vp, vp, sz, vp]),
            "bsw_submit_t": (C.c_int, [vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_submit_packed_t": (C.c_int, [vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_submit_ref_t": (C.c_int, [vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_wait_ticket": (C.c_int, [vp, C.c_uint64]), "bsw_test": (C.c_int, [vp, C.c_uint64]),
            "bsw_inflight": (C.c_int, [vp]), "bsw_host_stats": (C.c_int, [vp, vp, sz]),
            "bsw_upload_packed": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp)]),
            "bsw_pack_tasks": (C.c_int64, [vp, sz, vp, sz, vp]), "bsw_pack_tasks_bound": (sz, [vp, sz]),
            "bsw_extend_batch": (C.c_int, [vp, vp, vp, sz, vp]),
            "bsw_upload": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp)]),
            "bsw_run": (C.c_int, [vp, vp]), "bsw_sync": (C.c_int, [vp]),
            "bsw_upload_raw": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp)]), "bsw_run_staged": (C.c_int, [vp, vp]),
            "bsw_run_history2": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
            "bsw_effective_timeout_ms": (C.c_int, [vp]),
            "bsw_download": (C.c_int, [vp, vp, vp]),
            "bsw_batch_info": (C.c_int, [vp] + [C.POINTER(C.c_uint64)] * 4),
            "bsw_last_run_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
            "bsw_free_batch": (None, [vp, vp]),
            "bsw_run_history": (C.c_int, [vp, C.POINTER(C.c_float), C.c_int]),
            "bsw_refbatch_encode": (C.c_int, [vp, vp, sz, vp]),
            "bsw_refbatch_decode": (C.c_int, [vp, vp, vp, sz, vp, sz]),
            "bsw_refbatch_encode_results": (C.c_int, [vp, sz, vp]),
            "bsw_refbatch_decode_results": (C.c_int, [vp, sz, vp]),
            "bsw_refbatch_run": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
            "bsw_refbatch_submit": (C.c_int, [vp, vp, vp]),
            "bsw_refbatch_wait": (C.c_int, [vp, C.c_int, C.c_int]),
            "bsw_host_alloc": (vp, [sz]), "bsw_host_free": (None, [vp]),
            "bsw_host_register": (C.c_int, [vp, sz]), "bsw_host_unregister": (C.c_int, [vp]),
            "bsw_batch_order": (C.c_int, [vp, vp, vp, vp]),
            "bsw_scalar_stats": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
            "bsw_set_rtl_packed": (None, [C.c_int]),
            "bsw_rtl_packed": (C.c_int, []),
            "bsw_rtl_packed_stats": (C.c_int, [C.c_void_p, C.c_int]),
            "bsw_set_align_long": (None, [C.c_int]),
            "bsw_align_long": (C.c_int, []),
            "bsw_align_long_stats": (C.c_int, [C.c_void_p, C.c_int]),
            "bsw_global_batch": (C.c_int, [vp, vp, vp, sz, C.c_int, vp, vp]),
            "bsw_align_batch": (C.c_int, [vp, vp, vp, sz, vp]),
            "bsw_cigar_ref_batch": (C.c_int, [vp, vp, vp, vp, sz, C.c_int, vp, C.c_int, vp, vp]),
            "bsw_cigar_ref_submit_t": (C.c_int, [vp, vp, vp, vp, sz, C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_uint64)]),
            "bsw_matesw_ref_submit_t": (C.c_int, [vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_reads_upload": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp)]),
            "bsw_reads_upload_start": (C.c_int, [vp, vp, vp, sz, C.POINTER(vp)]),
            "bsw_reads_upload_enc": (C.c_int, [vp, vp, vp, sz, C.c_int, C.POINTER(vp)]),
            "bsw_reads_upload_start_enc": (C.c_int, [vp, vp, vp, sz, C.c_int, C.POINTER(vp)]),
            "bsw_reads_test": (C.c_int, [vp, vp]),
            "bsw_reads_wait": (C.c_int, [vp, vp]),
            "bsw_reads_image": (C.c_int, [vp, vp, C.c_int, vp, sz]),
            "bsw_reads_free": (C.c_int, [vp, vp]),
            "bsw_reads_info": (C.c_int, [vp] + [C.POINTER(C.c_uint64)] * 3),
            "bsw_submit_reads_t": (C.c_int, [vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_matesw_reads_submit_t": (C.c_int, [vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_cigar_reads_submit_t": (C.c_int, [vp, vp, vp, vp, vp, sz, C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_uint64)]),
            "bsw_patch_ref_batch": (C.c_int, [vp, vp, vp, vp, sz, vp]),
            "bsw_patch_ref_submit_t": (C.c_int, [vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_patch_reads_submit_t": (C.c_int, [vp, vp, vp, vp, vp, sz, vp, C.POINTER(C.c_uint64)]),
            "bsw_patch_pretest": (C.c_int, [vp, C.c_int64, vp, vp, C.POINTER(C.c_int)]),
            "bsw_patch_decide": (C.c_int, [vp, vp, C.c_int]),
            "bsw_c2a_default_opt": (None, [vp]),
            "bsw_chain2aln_plan": (C.c_int, [vp, C.c_int64, vp, sz, vp, sz, vp, sz, vp, vp, vp, C.c_char_p, sz]),
            "bsw_chain2aln_replay": (C.c_int, [vp, vp, vp, sz, vp, sz, vp, sz, vp, C.c_int, vp, C.POINTER(sz), vp, vp]),
            "bsw_chain2aln_ref_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, sz, C.POINTER(vp)]),
            "bsw_chain2aln_reads_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, sz, C.POINTER(vp)]),
            "bsw_chain2aln_test": (C.c_int, [vp]),
            "bsw_chain2aln_finish": (C.c_int, [vp, vp, C.POINTER(sz), vp, vp, vp]),
            "bsw_chain2aln_stats": (C.c_int, [vp, vp]),
            "bsw_c2a_device_register": (C.c_int, [vp]),
            "bsw_c2a_device_load": (C.c_int, [C.c_char_p]),
            "bsw_c2a_device_error": (C.c_char_p, []),
            "bsw_set_c2a_device": (C.c_int, [C.c_int]),
            "bsw_c2a_device": (C.c_int, []),
            "bsw_chain2aln_replay_batch": (C.c_int, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, C.c_int, vp, C.POINTER(sz), vp, vp, vp]),
            "bsw_chain2aln_replay_submit_t": (C.c_int, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, C.c_int, vp, C.POINTER(sz), vp, vp, vp,
                                                        C.POINTER(C.c_uint64)]),
            "bsw_sdp_default_opt": (None, [vp]),
            "bsw_sdp_from_cregs": (C.c_int, [vp, sz, vp]),
            "bsw_sdp_open": (C.c_int, [vp, vp, C.c_int64, vp, sz, vp, vp, sz, C.POINTER(vp), C.c_char_p, sz]),
            "bsw_sdp_needs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz)]),
            "bsw_sdp_feed": (C.c_int, [vp, vp, sz]),
            "bsw_sdp_collect": (C.c_int, [vp, vp, C.POINTER(sz), vp, vp]),
            "bsw_sdp_close": (None, [vp]),
            "bsw_sdp_ref_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, C.POINTER(vp)]),
            "bsw_sdp_reads_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, C.POINTER(vp)]),
            "bsw_sdp_test": (C.c_int, [vp]),
            "bsw_sdp_finish": (C.c_int, [vp, vp, C.POINTER(sz), vp, vp]),
            "bsw_sdp_job_stats": (C.c_int, [vp, vp]),
            "bsw_rescue_default_opt": (None, [vp]),
            "bsw_rescue_open": (C.c_int, [vp, vp, C.c_int64, vp, sz, vp, sz, vp, vp, sz, C.POINTER(vp), C.c_char_p, sz]),
            "bsw_rescue_needs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz)]),
            "bsw_rescue_feed": (C.c_int, [vp, vp, sz]),
            "bsw_rescue_collect": (C.c_int, [vp, vp, C.POINTER(sz), vp, vp, vp]),
            "bsw_rescue_out_capacity": (sz, [vp]),
            "bsw_rescue_close": (None, [vp]),
            "bsw_rescue_ref_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, C.POINTER(vp)]),
            "bsw_rescue_reads_start": (C.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, C.POINTER(vp)]),
            "bsw_rescue_test": (C.c_int, [vp]),
            "bsw_rescue_finish": (C.c_int, [vp, vp, sz, C.POINTER(sz), vp, vp, vp]),
            "bsw_rescue_job_stats": (C.c_int, [vp, vp]),
            "bsw_rescue_job_out_capacity": (sz, [vp]),
            "bsw_infer_bw": (C.c_int, [C.c_int] * 6),
            "bsw_matesw_ref_batch": (C.c_int, [vp, vp, vp, vp, sz, vp]),
            "bsw_infer_dir": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
            "bsw_matesw_windows": (C.c_int, [C.c_int64, C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp, vp]),
            "ksw_global2": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 5 + [vp, vp]),
            "ksw_global": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 3 + [vp, vp]),
            "bsw_ref_upload": (C.c_int, [vp, vp, C.c_int64, C.POINTER(vp)]),
            "bsw_ref_free": (None, [vp, vp]),
            "bsw_upload_ref": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(vp)]),
            "bsw_extend_ref": (C.c_int, [vp, vp, vp, vp, sz, vp]),
            "bsw_submit_ref": (C.c_int, [vp, vp, vp, vp, sz, vp]),
            "bsw_plan_batch": (C.c_int64, [vp, vp, sz, C.c_int, C.c_int, vp, vp]),
            "bsw_plan_order_capacity": (sz, [sz]),
            "bsw_pack_bases": (C.c_int, [vp, C.c_int, vp]),
            "bsw_cal_max_gap": (C.c_int, [vp, C.c_int]),
            "bsw_chain_window": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int64, vp]),
            "bsw_seed_scratch_bytes": (sz, [vp, C.c_int64]),
            "bsw_seed_to_task": (C.c_int, [vp, vp, C.c_int, vp, C.c_int64, C.c_int64, vp, vp, sz, C.c_uint32, vp]),
            "bsw_result_to_alnreg": (C.c_int, [vp, vp, vp]),
            "bsw_pac_get_seq": (C.c_int64, [C.c_int64, vp, C.c_int64, C.c_int64, vp]),
            "bsw_synth_generate": (C.c_int64, [vp, sz, vp, vp, sz]),
            "bsw_synth_arena_bound": (sz, [vp, sz]),
            "bsw_synth_ref_generate": (C.c_int64, [vp, vp, C.c_int64, vp, sz, vp, vp, sz]),
            "bsw_set_default_variant": (None, [C.c_int]),
            "ksw_extend2": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 8 + [vp] * 5),
            "ksw_extend": (C.c_int, [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 6 + [vp] * 5),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


EXPORTS = ["bsw_c2a_default_opt", "bsw_chain2aln_plan", "bsw_chain2aln_replay", "bsw_chain2aln_ref_start", "bsw_chain2aln_reads_start",
           "bsw_chain2aln_test", "bsw_chain2aln_finish", "bsw_chain2aln_stats",
           "bsw_c2a_device_register", "bsw_c2a_device_load", "bsw_c2a_device_error", "bsw_set_c2a_device", "bsw_c2a_device",
           "bsw_chain2aln_replay_batch", "bsw_chain2aln_replay_submit_t",
           "bsw_sdp_default_opt", "bsw_sdp_from_cregs", "bsw_sdp_open", "bsw_sdp_needs", "bsw_sdp_feed", "bsw_sdp_collect", "bsw_sdp_close",
           "bsw_sdp_ref_start", "bsw_sdp_reads_start", "bsw_sdp_test", "bsw_sdp_finish", "bsw_sdp_job_stats",
           "bsw_rescue_default_opt", "bsw_rescue_open", "bsw_rescue_needs", "bsw_rescue_feed", "bsw_rescue_collect", "bsw_rescue_out_capacity",
           "bsw_rescue_close", "bsw_rescue_ref_start", "bsw_rescue_reads_start", "bsw_rescue_test", "bsw_rescue_finish", "bsw_rescue_job_stats",
           "bsw_rescue_job_out_capacity",
           "ksw_global2", "ksw_global", "bsw_global_batch", "bsw_cigar_ref_batch", "bsw_infer_bw", "bsw_matesw_ref_batch",
           "bsw_cigar_ref_submit_t", "bsw_matesw_ref_submit_t",
           "bsw_patch_ref_batch", "bsw_patch_ref_submit_t", "bsw_patch_reads_submit_t", "bsw_patch_pretest", "bsw_patch_decide",
           "bsw_reads_upload", "bsw_reads_upload_start", "bsw_reads_upload_enc", "bsw_reads_upload_start_enc", "bsw_reads_test", "bsw_reads_wait", "bsw_reads_image", "bsw_reads_free", "bsw_reads_info", "bsw_submit_reads_t", "bsw_matesw_reads_submit_t", "bsw_cigar_reads_submit_t",
           "bsw_infer_dir", "bsw_matesw_windows", "bsw_align_batch", "ksw_align2", "ksw_align", "ksw_extend2", "ksw_extend", "bsw_set_default_variant", "bsw_scalar_stats", "bsw_set_rtl_packed", "bsw_rtl_packed", "bsw_rtl_packed_stats", "bsw_set_align_long", "bsw_align_long", "bsw_align_long_stats", "bsw_host_alloc", "bsw_host_free",
           "bsw_host_register", "bsw_host_unregister", "bsw_batch_order", "bsw_refbatch_submit", "bsw_refbatch_wait", "bsw_default_params", "bsw_default_config",
           "bsw_device_count", "bsw_create", "bsw_create_sized", "bsw_abi_version", "bsw_chain_timeouts", "bsw_device_placement", "bsw_destroy", "bsw_last_error", "bsw_submit", "bsw_wait",
           "bsw_submit_packed", "bsw_upload_packed", "bsw_pack_tasks", "bsw_pack_tasks_bound",
           "bsw_submit_t", "bsw_submit_packed_t", "bsw_submit_ref_t", "bsw_wait_ticket", "bsw_test", "bsw_inflight", "bsw_host_stats",
           "bsw_upload_raw", "bsw_run_staged", "bsw_run_history2", "bsw_effective_timeout_ms",
           "bsw_extend_batch", "bsw_upload", "bsw_run", "bsw_sync", "bsw_download", "bsw_batch_info",
           "bsw_last_run_ms", "bsw_run_history", "bsw_free_batch", "bsw_refbatch_encode", "bsw_refbatch_decode",
           "bsw_refbatch_encode_results", "bsw_refbatch_decode_results", "bsw_refbatch_run",
           "bsw_ref_upload", "bsw_ref_free", "bsw_upload_ref", "bsw_extend_ref", "bsw_submit_ref",
           "bsw_plan_batch", "bsw_plan_order_capacity", "bsw_pack_bases", "bsw_cal_max_gap", "bsw_chain_window", "bsw_seed_scratch_bytes", "bsw_seed_to_task",
           "bsw_result_to_alnreg", "bsw_pac_get_seq", "bsw_synth_generate", "bsw_synth_arena_bound", "bsw_synth_ref_generate"]


def default_params(**over):
    p = np.zeros(1, dtype=PARAMS)
    lib().bsw_default_params(p.ctypes.data)
    for k, v in over.items():
        p[k] = v
    return p


def pack_tasks(tasks, arena=None):
    """Byte-per-base tasks -> (tasks whose pointers address 4-bit packed words, the uint64 arena holding them).  `arena`: a
    uint64 view of registered memory (HostArena.view(np.uint64, ...)) to pack into, or None for a fresh numpy array."""
    need = int(lib().bsw_pack_tasks_bound(tasks.ctypes.data, len(tasks)))
    if arena is None:
        arena = np.zeros(need // 8 + 1, dtype=np.uint64)
    assert arena.dtype == np.uint64 and arena.nbytes >= need
    out = np.zeros(len(tasks), dtype=TASK)
    used = int(lib().bsw_pack_tasks(tasks.ctypes.data, len(tasks), arena.ctypes.data, arena.nbytes, out.ctypes.data))
    if used < 0:
        raise RuntimeError("bsw_pack_tasks failed (%d)" % used)
    return out, arena


def bwa_matrix(a=1, b=4, n=-1):
    m = np.full((5, 5), -b, dtype=np.int8)
    for i in range(4):
        m[i, i] = a
    m[4, :] = n
    m[:, 4] = n
    return m.reshape(25)


def synth_arena_bound(n, **spec):
    s = np.zeros(1, dtype=SYNTH)
    d = dict(seed=1, read_len=150, seed_len_min=19, seed_len_max=19, seed_at_start=1, sub_rate=0.01,
             indel_rate=0.001, n_rate=0.0, junk_frac=0.0, a=1, w=100, o=6, e=1)
    d.update(spec)
    for k, v in d.items():
        s[k] = v
    return int(lib().bsw_synth_arena_bound(s.ctypes.data, n))


def synth_tasks(n, arena=None, **spec):
    """Generate n synthetic seeds.  Returns (tasks, arena); keep arena alive.
    arena: optional uint8 buffer to generate into (e.g. HostArena(...).u8 for DMA-direct submits)."""
    s = np.zeros(1, dtype=SYNTH)
    d = dict(seed=1, read_len=150, seed_len_min=19, seed_len_max=19, seed_at_start=1, sub_rate=0.01,
             indel_rate=0.001, n_rate=0.0, junk_frac=0.0, a=1, w=100, o=6, e=1)
    d.update(spec)
    for k, v in d.items():
        s[k] = v
    L = lib()
    bound = L.bsw_synth_arena_bound(s.ctypes.data, n)
    if arena is None:
        arena = np.zeros(bound, dtype=np.uint8)
    elif arena.size < bound:
        raise ValueError("arena too small: need %d bytes" % bound)
    tasks = np.zeros(n, dtype=TASK)
    used = L.bsw_synth_generate(s.ctypes.data, n, tasks.ctypes.data, arena.ctypes.data, arena.size)
    if used < 0:
        raise BswError(int(used), "bsw_synth_generate")
    return tasks, arena


def synth_ref_tasks(n, l_pac, params, arena=None, **spec):
    """Synthetic genome + reads against it (bsw_synth_ref_generate).  Returns (pac, rtasks, arena)."""
    s = np.zeros(1, dtype=SYNTH)
    d = dict(seed=1, read_len=150, seed_len_min=19, seed_len_max=19, seed_at_start=1, sub_rate=0.01,
             indel_rate=0.001, n_rate=0.0, junk_frac=0.0, a=1, w=100, o=6, e=1)
    d.update(spec)
    for k, v in d.items():
        s[k] = v
    need = int(d["read_len"]) * n
    if arena is None:
        arena = np.zeros(need + 64, dtype=np.uint8)
    elif arena.size < need:
        raise ValueError("arena too small: need %d bytes" % need)
    pac = np.zeros((l_pac + 3) // 4, dtype=np.uint8)
    rt = np.zeros(n, dtype=REF_TASK)
    used = lib().bsw_synth_ref_generate(s.ctypes.data, params.ctypes.data, l_pac, pac.ctypes.data, n, rt.ctypes.data, arena.ctypes.data, arena.size)
    if used < 0:
        raise BswError(int(used), "bsw_synth_ref_generate")
    return pac, rt, arena


def make_tasks(seeds):
    """Build a TASK array from python dicts {lq, lt, rq, rt, h0, [init_score, qbeg, tag]} (sequences =
    iterables of base codes).  Returns (tasks, arena)."""
    total = sum(len(s.get(k, ())) for s in seeds for k in ("lq", "lt", "rq", "rt"))
    arena = np.zeros(total + 8, dtype=np.uint8)
    tasks = np.zeros(len(seeds), dtype=TASK)
    off = 0
    base = arena.ctypes.data
    for i, s in enumerate(seeds):
        for key, pf, lf in (("lq", "lquery", "lqlen"), ("lt", "ltarget", "ltlen"),
                            ("rq", "rquery", "rqlen"), ("rt", "rtarget", "rtlen")):
            a = np.asarray(s.get(key, ()), dtype=np.uint8)
            arena[off:off + len(a)] = a
            tasks[i][pf] = base + off
            tasks[i][lf] = len(a)
            off += len(a)
        tasks[i]["h0"] = s["h0"]
        tasks[i]["init_score"] = s.get("init_score", -1)
        tasks[i]["qbeg"] = s.get("qbeg", len(s.get("lq", ())))
        tasks[i]["tag"] = s.get("tag", i)
    return tasks, arena


class DeviceBatch:
    def __init__(self, ctx, handle, n):
        self.ctx, self.handle, self.n = ctx, handle, n

    def info(self):
        v = [C.c_uint64(0) for _ in range(4)]
        lib().bsw_batch_info(self.handle, *[C.byref(x) for x in v])
        return dict(n_tasks=v[0].value, in_bytes=v[1].value, out_bytes=v[2].value, launches=v[3].value)

    def free(self):
        if self.handle:
            lib().bsw_free_batch(self.ctx.handle, self.handle)
            self.handle = None


class BswContext:
    """One GPU context = one of the reference's PE arrays behind its batch manager."""

    def __init__(self, device=0, kernel=KERNEL_AUTO, streams=4, pack_threads=8, chunk_tasks=0, devices=None,
                 timeout_ms=0, result_format=RESULT_FULL, pin_threads=None):
        cfg = np.zeros(1, dtype=CONFIG)
        lib().bsw_default_config(cfg.ctypes.data)
        cfg["device"], cfg["kernel"], cfg["streams"] = device, kernel, streams
        cfg["pack_threads"], cfg["chunk_tasks"] = pack_threads, chunk_tasks
        if devices is not None:                 # one context over several GPUs: chunk k -> devices[k % len(devices)]
            cfg["n_devices"] = len(devices)
            cfg["devices"][0, :len(devices)] = devices
        if timeout_ms:
            cfg["timeout_ms"] = timeout_ms
        cfg["result_format"] = result_format
        if pin_threads is not None:
            cfg["pin_threads"] = 1 if pin_threads else -1
        self.out_dtype = PAIR if result_format == RESULT_PAIR else RESULT      # what the submit calls hand back
        h = C.c_void_p()
        rc = lib().bsw_create(cfg.ctypes.data, C.byref(h))
        if rc:
            raise BswError(rc, "bsw_create")
        self.handle = h
        self._keep = None
        self.last_ticket = 0

    def _chk(self, rc, what):
        if rc:
            raise BswError(rc, "%s: %s" % (what, lib().bsw_last_error(self.handle).decode()))

    def placement(self, k=0):
        """Where device k of the context sits and whether its slot threads are pinned next to it."""
        buf = C.create_string_buffer(64)
        node, ncpu = C.c_int(-1), C.c_int(0)
        self._chk(lib().bsw_device_placement(self.handle, k, buf, 64, C.byref(node), C.byref(ncpu)), "bsw_device_placement")
        return dict(bdf=buf.value.decode(), numa_node=node.value, pinned_cpus=ncpu.value)

    def chain_timeouts(self):
        """Waits of the launch chain that ended at their deadline (0 unless kernels are being run one at a time)."""
        v = C.c_uint64(0)
        self._chk(lib().bsw_chain_timeouts(self.handle, C.byref(v)), "bsw_chain_timeouts")
        return v.value

    def close(self):
        if self.handle:
            for job in list(getattr(self, "_jobs", ())):       # jobs never finished: their ticket and pinned arrays go first
                job.release()
            lib().bsw_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # streaming path: host buffers in, host buffers out.  Up to MAX_INFLIGHT submits per context; every submit has a ticket.
    def _submit(self, fn, what, params, tasks, out, *front):
        if out is None:
            out = np.zeros(len(tasks), dtype=self.out_dtype)
        assert out.dtype == self.out_dtype and len(out) >= len(tasks)
        t = C.c_uint64(0)
        self._chk(fn(self.handle, params.ctypes.data, *front, tasks.ctypes.data, len(tasks), out.ctypes.data, C.byref(t)), what)
        if self._keep is None:
            self._keep = {}
        self._keep[t.value] = (params, tasks, out)          # the arrays must outlive the submit
        self.last_ticket = t.value
        return out

    def submit(self, params, tasks, out=None):
        return self._submit(lib().bsw_submit_t, "bsw_submit", params, tasks, out)

    def wait(self):
        """every submit in flight; raises the first failure in submit order"""
        try:
            self._chk(lib().bsw_wait(self.handle), "bsw_wait")
        finally:
            self._keep = None

    def wait_ticket(self, ticket):
        try:
            self._chk(lib().bsw_wait_ticket(self.handle, ticket), "bsw_wait_ticket")
        finally:
            if self._keep:
                self._keep.pop(ticket, None)

    def test(self, ticket):
        """non-blocking: True once the submit is complete (collect it with wait_ticket / wait)"""
        rc = lib().bsw_test(self.handle, ticket)
        if rc < 0:
            self._chk(rc, "bsw_test")
        return bool(rc)

    def inflight(self):
        return int(lib().bsw_inflight(self.handle))

    def host_stats(self):
        """bsw_host_stats as a dict: CPU ns of the slot / gather threads, seeds, chunks, submits, bytes moved"""
        s = np.zeros(1, dtype=STATS)
        self._chk(lib().bsw_host_stats(self.handle, s.ctypes.data, STATS.itemsize), "bsw_host_stats")
        return {k: int(s[k][0]) for k in STATS.names}

    def submit_packed(self, params, ptasks, out=None):
        """bsw_submit_packed: `ptasks` from pack_tasks() (sequence pointers address 4-bit packed words)."""
        return self._submit(lib().bsw_submit_packed_t, "bsw_submit_packed", params, ptasks, out)

    def extend_pairs_packed(self, params, ptasks, out=None):
        out = self.submit_packed(params, ptasks, out)
        self.wait()
        return out[:len(ptasks)]

    def upload_packed(self, params, ptasks):
        h = C.c_void_p()
        self._chk(lib().bsw_upload_packed(self.handle, params.ctypes.data, ptasks.ctypes.data, len(ptasks), C.byref(h)), "bsw_upload_packed")
        return DeviceBatch(self, h, len(ptasks))

    def extend_pairs(self, params, tasks, out=None):
        """Streaming path, synchronous.  Pass a reused `out` array to keep page faults of a fresh one out of timings."""
        out = self.submit(params, tasks, out)
        self.wait()
        return out[:len(tasks)]

    def extend_batch(self, params, etasks):
        out = np.zeros(len(etasks), dtype=EXT)
        self._chk(lib().bsw_extend_batch(self.handle, params.ctypes.data, etasks.ctypes.data, len(etasks), out.ctypes.data), "bsw_extend_batch")
        return out

    # device-resident path
    def upload(self, params, tasks):
        h = C.c_void_p()
        self._chk(lib().bsw_upload(self.handle, params.ctypes.data, tasks.ctypes.data, len(tasks), C.byref(h)), "bsw_upload")
        return DeviceBatch(self, h, len(tasks))

    def upload_raw(self, params, tasks):
        """bsw_upload_raw: the byte-per-base sequences stay in HBM beside the packed form (for run_staged)."""
        h = C.c_void_p()
        self._chk(lib().bsw_upload_raw(self.handle, params.ctypes.data, tasks.ctypes.data, len(tasks), C.byref(h)), "bsw_upload_raw")
        return DeviceBatch(self, h, len(tasks))

    def run(self, batch):
        self._chk(lib().bsw_run(self.handle, batch.handle), "bsw_run")

    def run_staged(self, batch):
        """pack + bin + DP kernels of a batch from upload_raw (the device side of one bsw_submit chunk)."""
        self._chk(lib().bsw_run_staged(self.handle, batch.handle), "bsw_run_staged")

    def run_history2(self, cap=4096):
        """[(total_ms, staging_ms)] of every run since the last call."""
        a, b = (C.c_float * cap)(), (C.c_float * cap)()
        n = lib().bsw_run_history2(self.handle, a, b, cap)
        if n < 0:
            self._chk(n, "bsw_run_history2")
        return [(a[i], b[i]) for i in range(n)]

    def sync(self):
        self._chk(lib().bsw_sync(self.handle), "bsw_sync")

    def last_run_ms(self):
        ms = C.c_float(0)
        self._chk(lib().bsw_last_run_ms(self.handle, C.byref(ms)), "bsw_last_run_ms")
        return ms.value

    def run_history(self, cap=4096):
        buf = (C.c_float * cap)()
        n = lib().bsw_run_history(self.handle, buf, cap)
        if n < 0:
            self._chk(n, "bsw_run_history")
        return [buf[i] for i in range(n)]

    def download(self, batch):
        out = np.zeros(batch.n, dtype=RESULT)
        self._chk(lib().bsw_download(self.handle, batch.handle, out.ctypes.data), "bsw_download")
        return out

    def global_batch(self, params, gtasks, max_cigar=64, want_cigar=True):
        """Batched ksw_global2.  Returns (GRESULT array, cigars uint32[n, max_cigar] or None)."""
        res = np.zeros(len(gtasks), dtype=GRESULT)
        cig = np.zeros((len(gtasks), max_cigar), dtype=np.uint32) if want_cigar else None
        self._chk(lib().bsw_global_batch(self.handle, params.ctypes.data, gtasks.ctypes.data, len(gtasks), max_cigar,
                                         res.ctypes.data, cig.ctypes.data if want_cigar else None), "bsw_global_batch")
        return res, cig

    def cigar_ref_batch(self, params, ref, ctasks, max_cigar=64, max_md=256, want_cigar=True, want_md=True):
        """bwa_gen_cigar2 (+ mem_reg2aln's retries) against a reference from ref_upload.  Returns (CRESULT array,
        cigars uint32[n, max_cigar] or None, list of MD strings or None)."""
        n = len(ctasks)
        res = np.zeros(n, dtype=CRESULT)
        cig = np.zeros((n, max_cigar), dtype=np.uint32) if want_cigar else None
        md = np.zeros((n, max_md), dtype=np.uint8) if want_md else None
        self._chk(lib().bsw_cigar_ref_batch(self.handle, params.ctypes.data, ref, ctasks.ctypes.data, n, max_cigar,
                                            cig.ctypes.data if want_cigar else None, max_md,
                                            md.ctypes.data if want_md else None, res.ctypes.data), "bsw_cigar_ref_batch")
        strings = None
        if want_md:
            strings = [bytes(md[i, :max(int(res["md_len"][i]), 0)]).decode("ascii") for i in range(n)]
        return res, cig, strings

    def matesw_ref_batch(self, params, ref, mtasks):
        """mem_matesw's ksw_align2 against a reference from ref_upload: the windows are fetched and the mates
        reverse-complemented (is_rev) on the GPU.  Returns an MRESULT array."""
        res = np.zeros(len(mtasks), dtype=MRESULT)
        self._chk(lib().bsw_matesw_ref_batch(self.handle, params.ctypes.data, ref, mtasks.ctypes.data, len(mtasks), res.ctypes.data),
                  "bsw_matesw_ref_batch")
        return res

    def patch_ref_batch(self, params, ref, ptasks):
        """mem_patch_reg against a reference from ref_upload (PTASK records: the whole read and two of its regions; params["w"]
        is opt->w).  Returns a PRESULT array."""
        res = np.zeros(len(ptasks), dtype=PRESULT)
        self._chk(lib().bsw_patch_ref_batch(self.handle, params.ctypes.data, ref, ptasks.ctypes.data, len(ptasks), res.ctypes.data),
                  "bsw_patch_ref_batch")
        return res

    def submit_patch_ref(self, params, ref, ptasks):
        """patch_ref_batch as a ticket of the streaming pipeline (bsw_patch_ref_submit_t).  Returns (ticket, PRESULT array); the
        array is filled once the ticket is complete.  The reads that `ptasks` points to must stay alive until then."""
        res = np.zeros(len(ptasks), dtype=PRESULT)
        t = C.c_uint64(0)
        self._chk(lib().bsw_patch_ref_submit_t(self.handle, params.ctypes.data, ref, ptasks.ctypes.data, len(ptasks), res.ctypes.data,
                                               C.byref(t)), "bsw_patch_ref_submit")
        self._keep_alive(t.value, params, ptasks, res)
        return t.value, res

    def submit_patch_reads(self, params, ref, rd, rdptasks):
        """submit_patch_ref against a resident read block (RD_PTASK records).  Returns (ticket, PRESULT array)."""
        res = np.zeros(len(rdptasks), dtype=PRESULT)
        t = C.c_uint64(0)
        self._chk(lib().bsw_patch_reads_submit_t(self.handle, params.ctypes.data, ref, rd, rdptasks.ctypes.data, len(rdptasks),
                                                 res.ctypes.data, C.byref(t)), "bsw_patch_reads_submit")
        self._keep_alive(t.value, params, rdptasks, res)
        return t.value, res

    def _keep_alive(self, ticket, *arrays):
        if self._keep is None:
            self._keep = {}
        self._keep[ticket] = arrays                         # the arrays must outlive the submit
        self.last_ticket = ticket

    def submit_cigar_ref(self, params, ref, ctasks, max_cigar=64, max_md=256, want_cigar=True, want_md=True):
        """cigar_ref_batch as a ticket of the streaming pipeline (bsw_cigar_ref_submit_t): runs on every device of the context,
        beside extension submits.  Returns (ticket, CRESULT array, cigars uint32[n, max_cigar] or None, MD slots
        uint8[n, max_md] or None); the arrays are filled once test(ticket) is true / wait_ticket(ticket) has returned
        (md_strings() decodes the MD slots then).  The reads that `ctasks` points to must stay alive until then."""
        n = len(ctasks)
        res = np.zeros(n, dtype=CRESULT)
        cig = np.zeros((n, max_cigar), dtype=np.uint32) if want_cigar else None
        md = np.zeros((n, max_md), dtype=np.uint8) if want_md else None
        t = C.c_uint64(0)
        self._chk(lib().bsw_cigar_ref_submit_t(self.handle, params.ctypes.data, ref, ctasks.ctypes.data, n, max_cigar,
                                               cig.ctypes.data if want_cigar else None, max_md,
                                               md.ctypes.data if want_md else None, res.ctypes.data, C.byref(t)), "bsw_cigar_ref_submit")
        self._keep_alive(t.value, params, ctasks, res, cig, md)
        return t.value, res, cig, md

    @staticmethod
    def md_strings(res, md):
        """the MD strings of a collected submit_cigar_ref, as cigar_ref_batch returns them"""
        return [bytes(md[i, :max(int(res["md_len"][i]), 0)]).decode("ascii") for i in range(len(res))]

    def submit_matesw_ref(self, params, ref, mtasks):
        """matesw_ref_batch as a ticket of the streaming pipeline (bsw_matesw_ref_submit_t).  Returns (ticket, MRESULT array);
        the array is filled once the ticket is complete.  The mates that `mtasks` points to must stay alive until then."""
        res = np.zeros(len(mtasks), dtype=MRESULT)
        t = C.c_uint64(0)
        self._chk(lib().bsw_matesw_ref_submit_t(self.handle, params.ctypes.data, ref, mtasks.ctypes.data, len(mtasks), res.ctypes.data,
                                                C.byref(t)), "bsw_matesw_ref_submit")
        self._keep_alive(t.value, params, mtasks, res)
        return t.value, res

    # resident read blocks: upload once, then the three stages name a read by index
    @staticmethod
    def _reads_table(reads, encoding):
        """(arrays kept alive, pointers, lengths in bases) of a block: uint8 arrays (codes or letters; bytes objects too), or for
        READS_PACKED (words, n_bases) pairs, words a uint64 array of at least ceil(n_bases / 16) entries"""
        if encoding == READS_PACKED:
            arrs = [np.ascontiguousarray(w, dtype=np.uint64) for w, _ in reads]
            lens = np.array([n for _, n in reads], dtype=np.int32)
            for a, n in zip(arrs, lens):
                if len(a) < (int(n) + 15) // 16:
                    raise ValueError("a packed read of %d bases needs %d words, got %d" % (n, (int(n) + 15) // 16, len(a)))
        else:
            arrs = [np.frombuffer(r, dtype=np.uint8) if isinstance(r, (bytes, bytearray)) else np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
            lens = np.array([len(r) for r in arrs], dtype=np.int32)
        ptrs = np.array([r.ctypes.data if n else 0 for r, n in zip(arrs, lens)], dtype=np.uint64)
        return arrs, ptrs, lens

    def reads_upload(self, reads, encoding=0):
        """bsw_reads_upload / bsw_reads_upload_enc: `reads` is a sequence of uint8 arrays — codes 0..4 (READS_CODES) or FASTQ letters
        (READS_ASCII) — or of (uint64 words, n_bases) pairs (READS_PACKED).  Returns the block's handle; synchronous."""
        arrs, ptrs, lens = self._reads_table(reads, encoding)
        h = C.c_void_p()
        if encoding == READS_CODES:
            self._chk(lib().bsw_reads_upload(self.handle, ptrs.ctypes.data, lens.ctypes.data, len(arrs), C.byref(h)), "bsw_reads_upload")
        else:
            self._chk(lib().bsw_reads_upload_enc(self.handle, ptrs.ctypes.data, lens.ctypes.data, len(arrs), int(encoding), C.byref(h)), "bsw_reads_upload_enc")
        return h

    def reads_upload_start(self, reads, encoding=0):
        """bsw_reads_upload_start / bsw_reads_upload_start_enc: returns the block's handle at once; it may be handed to the
        *_reads_* submits at once.  `reads` as for reads_upload; the arrays are kept alive here until the block is freed (their
        bases belong to the upload until it is ready)."""
        arrs, ptrs, lens = self._reads_table(reads, encoding)
        h = C.c_void_p()
        if encoding == READS_CODES:
            self._chk(lib().bsw_reads_upload_start(self.handle, ptrs.ctypes.data, lens.ctypes.data, len(arrs), C.byref(h)), "bsw_reads_upload_start")
        else:
            self._chk(lib().bsw_reads_upload_start_enc(self.handle, ptrs.ctypes.data, lens.ctypes.data, len(arrs), int(encoding), C.byref(h)), "bsw_reads_upload_start_enc")
        if not hasattr(self, "_reads_alive"):
            self._reads_alive = {}
        self._reads_alive[h.value] = arrs
        return h

    def reads_test(self, rd):
        """bsw_reads_test: True once the block is ready, False while its upload is in flight; raises for a failed upload"""
        rc = lib().bsw_reads_test(self.handle, rd)
        if rc < 0:
            self._chk(rc, "bsw_reads_test")
        return rc == 1

    def reads_wait(self, rd):
        self._chk(lib().bsw_reads_wait(self.handle, rd), "bsw_reads_wait")

    def reads_image(self, rd, k=0):
        """bsw_reads_image: device k's copy of a ready block as uint64 words, slack included"""
        out = np.zeros(self.reads_info(rd)["device_bytes"] // 8, dtype=np.uint64)
        self._chk(lib().bsw_reads_image(self.handle, rd, k, out.ctypes.data, len(out)), "bsw_reads_image")
        return out

    def reads_free(self, rd):
        """bsw_reads_free; raises BswError(BSW_E_BUSY) while a ticket that uses the block has not been collected"""
        self._chk(lib().bsw_reads_free(self.handle, rd), "bsw_reads_free")
        getattr(self, "_reads_alive", {}).pop(getattr(rd, "value", rd), None)

    @staticmethod
    def reads_info(rd):
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().bsw_reads_info(rd, C.byref(a), C.byref(b), C.byref(c))
        if rc:
            raise BswError(rc, "bsw_reads_info")
        return {"n_reads": a.value, "bases": b.value, "device_bytes": c.value}

    def submit_reads(self, params, ref, rd, rdtasks, out=None):
        """submit_ref against a resident read block (bsw_submit_reads_t; RD_TASK records).  Returns the result array, filled
        once the ticket (self.last_ticket) is collected."""
        return self._submit(lib().bsw_submit_reads_t, "bsw_submit_reads", params, rdtasks, out, ref, rd)

    def submit_matesw_reads(self, params, ref, rd, rdmtasks):
        """submit_matesw_ref against a resident read block (RD_MTASK records).  Returns (ticket, MRESULT array)."""
        res = np.zeros(len(rdmtasks), dtype=MRESULT)
        t = C.c_uint64(0)
        self._chk(lib().bsw_matesw_reads_submit_t(self.handle, params.ctypes.data, ref, rd, rdmtasks.ctypes.data, len(rdmtasks),
                                                  res.ctypes.data, C.byref(t)), "bsw_matesw_reads_submit")
        self._keep_alive(t.value, params, rdmtasks, res)
        return t.value, res

    def submit_cigar_reads(self, params, ref, rd, rdctasks, max_cigar=64, max_md=256, want_cigar=True, want_md=True):
        """submit_cigar_ref against a resident read block (RD_CTASK records).  Returns (ticket, CRESULT array, cigars, MD slots)."""
        n = len(rdctasks)
        res = np.zeros(n, dtype=CRESULT)
        cig = np.zeros((n, max_cigar), dtype=np.uint32) if want_cigar else None
        md = np.zeros((n, max_md), dtype=np.uint8) if want_md else None
        t = C.c_uint64(0)
        self._chk(lib().bsw_cigar_reads_submit_t(self.handle, params.ctypes.data, ref, rd, rdctasks.ctypes.data, n, max_cigar,
                                                 cig.ctypes.data if want_cigar else None, max_md,
                                                 md.ctypes.data if want_md else None, res.ctypes.data, C.byref(t)), "bsw_cigar_reads_submit")
        self._keep_alive(t.value, params, rdctasks, res, cig, md)
        return t.value, res, cig, md

    # mem_chain2aln as one job of the pipeline: every seed is extended, bwa's loop is replayed over the results
    def chain2aln_start(self, params, ref, chains, seeds, rd=None, reads=None, opt=None):
        """bsw_chain2aln_reads_start (rd: a resident block) or bsw_chain2aln_ref_start (reads: a list of uint8 code arrays).
        chains: CHAIN array, seeds: CSEED array.  Returns a Chain2alnJob; it takes the place of the extension ticket."""
        chains, seeds = np.ascontiguousarray(chains, dtype=CHAIN), np.ascontiguousarray(seeds, dtype=CSEED)
        o = c2a_opt(**(opt or {}))
        h = C.c_void_p()
        keep = [params, chains, seeds, o]
        if rd is not None:
            rc = lib().bsw_chain2aln_reads_start(self.handle, params.ctypes.data, o.ctypes.data, ref, rd, chains.ctypes.data, len(chains),
                                                 seeds.ctypes.data, len(seeds), C.byref(h))
            n_reads = self.reads_info(rd)["n_reads"]
        else:
            arrs = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
            ptrs = np.array([r.ctypes.data if len(r) else 0 for r in arrs], dtype=np.uint64)
            lens = np.array([len(r) for r in arrs], dtype=np.int32)
            keep += [arrs, ptrs, lens]
            rc = lib().bsw_chain2aln_ref_start(self.handle, params.ctypes.data, o.ctypes.data, ref, ptrs.ctypes.data, lens.ctypes.data, len(arrs),
                                               chains.ctypes.data, len(chains), seeds.ctypes.data, len(seeds), C.byref(h))
            n_reads = len(arrs)
        self._chk(rc, "bsw_chain2aln_start")
        job = Chain2alnJob(self, h, len(seeds), n_reads, keep)
        if not hasattr(self, "_jobs"):
            self._jobs = weakref.WeakSet()
        self._jobs.add(job)
        return job

    def submit_chain2aln_replay(self, params, chains, seeds, lens, results, opt=None, want_extended=True):
        """chain2aln_replay_batch as a ticket (bsw_chain2aln_replay_submit_t).  Returns (ticket, C2aReplay); once the ticket is
        collected, C2aReplay.result() gives (CREG array, extended or None, reg_start, stats dict)."""
        r = C2aReplay(params, chains, seeds, lens, results, opt, want_extended)
        t = C.c_uint64(0)
        self._chk(lib().bsw_chain2aln_replay_submit_t(self.handle, *r.args(), C.byref(t)), "bsw_chain2aln_replay_submit")
        self._keep_alive(t.value, r)
        return t.value, r

    # mem_sort_dedup_patch as a job around the patch tickets
    def sdp_start(self, params, ref, regs, reg_start, rd=None, reads=None, opt=None):
        """bsw_sdp_reads_start (rd: a resident block) or bsw_sdp_ref_start (reads: a list of uint8 code arrays).  regs: SREG array
        sorted by read, reg_start: uint64[n_reads + 1] (what Chain2alnJob.finish and sdp_from_cregs give).  Returns an SdpJob."""
        regs, reg_start = np.ascontiguousarray(regs, dtype=SREG), np.ascontiguousarray(reg_start, dtype=np.uint64)
        o = sdp_opt(**(opt or {}))
        h = C.c_void_p()
        keep = [params, regs, reg_start, o]
        if rd is not None:
            n_reads = self.reads_info(rd)["n_reads"]
            assert len(reg_start) == n_reads + 1
            rc = lib().bsw_sdp_reads_start(self.handle, params.ctypes.data, o.ctypes.data, ref, rd, regs.ctypes.data, len(regs),
                                           reg_start.ctypes.data, C.byref(h))
        else:
            arrs = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
            ptrs = np.array([r.ctypes.data if len(r) else 0 for r in arrs], dtype=np.uint64)
            lens = np.array([len(r) for r in arrs], dtype=np.int32)
            assert len(reg_start) == len(arrs) + 1
            keep += [arrs, ptrs, lens]
            rc = lib().bsw_sdp_ref_start(self.handle, params.ctypes.data, o.ctypes.data, ref, ptrs.ctypes.data, lens.ctypes.data, len(arrs),
                                         regs.ctypes.data, len(regs), reg_start.ctypes.data, C.byref(h))
            n_reads = len(arrs)
        self._chk(rc, "bsw_sdp_start")
        job = SdpJob(self, h, len(regs), n_reads, keep)
        if not hasattr(self, "_jobs"):
            self._jobs = weakref.WeakSet()
        self._jobs.add(job)
        return job

    # mem_sam_pe's mate-rescue loop as a job around the rescue tickets
    def rescue_start(self, params, ref, regs, reg_start, rd=None, reads=None, contigs=None, opt=None):
        """bsw_rescue_reads_start (rd: a resident block) or bsw_rescue_ref_start (reads: a list of uint8 code arrays); reads 2k and
        2k + 1 are mates.  regs: SREG array sorted by read (what SdpJob.finish gives), reg_start: uint64[n_reads + 1], contigs: a
        CONTIG array or (offset, len) pairs (None: no table), opt: fields of RESCUE_OPT (low / high / failed: four values each).
        Returns a RescueJob."""
        regs, reg_start = np.ascontiguousarray(regs, dtype=SREG), np.ascontiguousarray(reg_start, dtype=np.uint64)
        o, ct = rescue_opt(**(opt or {})), contig_table(contigs)
        h = C.c_void_p()
        keep = [params, regs, reg_start, o, ct]
        if rd is not None:
            n_reads = self.reads_info(rd)["n_reads"]
            assert len(reg_start) == n_reads + 1
            rc = lib().bsw_rescue_reads_start(self.handle, params.ctypes.data, o.ctypes.data, ref, rd, ct.ctypes.data, len(ct), regs.ctypes.data,
                                              len(regs), reg_start.ctypes.data, C.byref(h))
        else:
            arrs = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
            ptrs = np.array([r.ctypes.data if len(r) else 0 for r in arrs], dtype=np.uint64)
            lens = np.array([len(r) for r in arrs], dtype=np.int32)
            assert len(reg_start) == len(arrs) + 1
            keep += [arrs, ptrs, lens]
            rc = lib().bsw_rescue_ref_start(self.handle, params.ctypes.data, o.ctypes.data, ref, ptrs.ctypes.data, lens.ctypes.data, len(arrs),
                                            ct.ctypes.data, len(ct), regs.ctypes.data, len(regs), reg_start.ctypes.data, C.byref(h))
            n_reads = len(arrs)
        self._chk(rc, "bsw_rescue_start")
        job = RescueJob(self, h, n_reads, keep)
        if not hasattr(self, "_jobs"):
            self._jobs = weakref.WeakSet()
        self._jobs.add(job)
        return job

    def align_batch(self, params, atasks):
        """Batched ksw_align2 (bwa's local alignment of mate rescue).  Returns a KSWR array."""
        res = np.zeros(len(atasks), dtype=KSWR)
        self._chk(lib().bsw_align_batch(self.handle, params.ctypes.data, atasks.ctypes.data, len(atasks), res.ctypes.data), "bsw_align_batch")
        return res

    def batch_order(self, batch):
        """Launch order the device-side binning produced (order, seg) — same layout as plan_batch."""
        order = np.zeros(int(lib().bsw_plan_order_capacity(batch.n)), dtype=np.uint32)
        seg = np.zeros(PLAN_SEGS + 1, dtype=np.uint32)
        self._chk(lib().bsw_batch_order(self.handle, batch.handle, order.ctypes.data, seg.ctypes.data), "bsw_batch_order")
        return order, seg

    def refbatch_submit(self, in_words, out_words):
        """Queue one 256 KiB task batch; both arrays must stay alive until refbatch_wait()."""
        assert in_words.dtype == np.uint32 and in_words.size == REFBATCH_IN_WORDS and in_words.flags.c_contiguous
        assert out_words.dtype == np.uint32 and out_words.size == REFBATCH_OUT_WORDS and out_words.flags.c_contiguous
        self._chk(lib().bsw_refbatch_submit(self.handle, in_words.ctypes.data, out_words.ctypes.data), "bsw_refbatch_submit")

    def refbatch_wait(self, variant=VARIANT_H, zdrop=0):
        rc = lib().bsw_refbatch_wait(self.handle, variant, zdrop)
        if rc < 0:
            self._chk(rc, "bsw_refbatch_wait")
        return rc

    # seeds against a device-resident 2-bit reference (F3)
    def ref_upload(self, pac, l_pac):
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        h = C.c_void_p()
        self._chk(lib().bsw_ref_upload(self.handle, pac.ctypes.data, l_pac, C.byref(h)), "bsw_ref_upload")
        return h

    def ref_free(self, ref):
        lib().bsw_ref_free(self.handle, ref)

    def extend_ref(self, params, ref, rtasks):
        out = np.zeros(len(rtasks), dtype=RESULT)
        self._chk(lib().bsw_extend_ref(self.handle, params.ctypes.data, ref, rtasks.ctypes.data, len(rtasks), out.ctypes.data), "bsw_extend_ref")
        return out

    def submit_ref(self, params, ref, rtasks, out=None):
        """Streaming form of extend_ref (finish with wait()): only the reads cross PCIe."""
        return self._submit(lib().bsw_submit_ref_t, "bsw_submit_ref", params, rtasks, out, ref)

    def refbatch_run(self, in_words, variant=VARIANT_H, zdrop=0):
        in_words = np.ascontiguousarray(in_words, dtype=np.uint32)
        assert in_words.size == REFBATCH_IN_WORDS
        out = np.zeros(REFBATCH_OUT_WORDS, dtype=np.uint32)
        rc = lib().bsw_refbatch_run(self.handle, in_words.ctypes.data, out.ctypes.data, variant, zdrop)
        if rc < 0:
            self._chk(rc, "bsw_refbatch_run")
        return out, rc


class Chain2alnJob:
    """One bsw_c2a_job: test() polls, finish() collects the ticket, replays mem_chain2aln and frees the job.  A job that is dropped
    without finish() — an exception between start and finish, a `with` block left early — is released (waited for, its results
    thrown away): by release(), at the end of a `with job:` block, by the context's close(), or when the object is collected."""

    def __init__(self, ctx, handle, n_seeds, n_reads, keep):
        self.ctx, self.handle, self.n_seeds, self.n_reads, self._keep = ctx, handle, n_seeds, n_reads, keep

    def release(self):
        """give up a job that was not finished: its place among the submits in flight and its pinned arrays are freed"""
        h, self.handle = self.handle, None
        if h and self.ctx.handle:                           # (a context that is closed has released its jobs itself)
            n = C.c_size_t(0)
            # waits; frees the job whatever it returns but BSW_E_BUSY (a device replay in flight that found no place: the job is intact)
            if lib().bsw_chain2aln_finish(h, None, C.byref(n), None, None, None) == -6:
                self.handle = h
                return
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def test(self):
        rc = lib().bsw_chain2aln_test(self.handle)
        if rc < 0:
            self.ctx._chk(rc, "bsw_chain2aln_test")
        return bool(rc)

    def stats(self):
        s = np.zeros(1, dtype=C2A_STATS)
        rc = lib().bsw_chain2aln_stats(self.handle, s.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_chain2aln_stats")
        return {k: int(s[k][0]) for k in C2A_STATS.names}

    def finish(self):
        """-> (CREG array in bwa's push order, extended uint8[n_seeds], reg_start uint64[n_reads + 1], stats dict)"""
        regs = np.zeros(max(self.n_seeds, 1), dtype=CREG)
        ext = np.zeros(max(self.n_seeds, 1), dtype=np.uint8)
        start = np.zeros(self.n_reads + 1, dtype=np.uint64)
        st = np.zeros(1, dtype=C2A_STATS)
        n = C.c_size_t(0)
        h, self.handle = self.handle, None                  # finish frees the job whatever it returns ...
        try:
            self.ctx._chk(lib().bsw_chain2aln_finish(h, regs.ctypes.data, C.byref(n), ext.ctypes.data, start.ctypes.data, st.ctypes.data),
                          "bsw_chain2aln_finish")
        except BswError as err:
            if err.code == -6:                              # ... but BSW_E_BUSY (the device replay found no place): call again
                self.handle = h
            raise
        finally:
            if self.handle is None:
                self._keep = None
        return regs[:n.value], ext[:self.n_seeds], start, {k: int(st[k][0]) for k in C2A_STATS.names}


def c2a_opt(**over):
    """bsw_c2a_default_opt, with fields replaced (seedlen0_frac < 0: the bwa-0.7.8 behaviour)"""
    o = np.zeros(1, dtype=C2A_OPT)
    lib().bsw_c2a_default_opt(o.ctypes.data)
    for k, v in over.items():
        o[k] = v
    return o


def chain2aln_plan(params, l_pac, chains, seeds, lens, reads=None):
    """bsw_chain2aln_plan: -> (RD_TASK array, REF_TASK array or None when reads is None).  reads: list of uint8 arrays whose
    addresses the REF_TASK records store (keep them alive).  Raises BswError with the plan's text."""
    chains, seeds = np.ascontiguousarray(chains, dtype=CHAIN), np.ascontiguousarray(seeds, dtype=CSEED)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    rdt = np.zeros(len(seeds), dtype=RD_TASK)
    rft = np.zeros(len(seeds), dtype=REF_TASK) if reads is not None else None
    ptrs = np.array([r.ctypes.data if len(r) else 0 for r in reads], dtype=np.uint64) if reads is not None else None
    err = C.create_string_buffer(400)
    rc = lib().bsw_chain2aln_plan(params.ctypes.data, l_pac, chains.ctypes.data, len(chains), seeds.ctypes.data, len(seeds), lens.ctypes.data,
                                  len(lens), ptrs.ctypes.data if reads is not None else None, rdt.ctypes.data,
                                  rft.ctypes.data if reads is not None else None, err, 400)
    if rc:
        raise BswError(rc, err.value.decode())
    return rdt, rft


def chain2aln_replay(params, chains, seeds, lens, results, opt=None):
    """bsw_chain2aln_replay over a RESULT or a PAIR array (one record per seed, in seed order) -> (CREG array, extended, reg_start)"""
    chains, seeds = np.ascontiguousarray(chains, dtype=CHAIN), np.ascontiguousarray(seeds, dtype=CSEED)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    results = np.ascontiguousarray(results)
    assert results.dtype in (RESULT, PAIR) and len(results) == len(seeds)
    o = c2a_opt(**(opt or {}))
    regs = np.zeros(max(len(seeds), 1), dtype=CREG)
    ext = np.zeros(max(len(seeds), 1), dtype=np.uint8)
    start = np.zeros(len(lens) + 1, dtype=np.uint64)
    n = C.c_size_t(0)
    rc = lib().bsw_chain2aln_replay(params.ctypes.data, o.ctypes.data, chains.ctypes.data, len(chains), seeds.ctypes.data, len(seeds),
                                    lens.ctypes.data, len(lens), results.ctypes.data, RESULT_PAIR if results.dtype == PAIR else RESULT_FULL,
                                    regs.ctypes.data, C.byref(n), ext.ctypes.data, start.ctypes.data)
    if rc:
        raise BswError(rc, "bsw_chain2aln_replay")
    return regs[:n.value], ext[:len(seeds)], start


class C2aReplay:
    """the arrays of one device replay: they stay alive, and where they are, until the call has returned or the ticket is collected"""

    def __init__(self, params, chains, seeds, lens, results, opt, want_extended):
        self.params = params
        self.chains, self.seeds = np.ascontiguousarray(chains, dtype=CHAIN), np.ascontiguousarray(seeds, dtype=CSEED)
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.results = np.ascontiguousarray(results)
        assert self.results.dtype in (RESULT, PAIR) and len(self.results) == len(self.seeds)
        self.o = c2a_opt(**(opt or {}))
        self.regs = np.zeros(max(len(self.seeds), 1), dtype=CREG)
        self.ext = np.zeros(max(len(self.seeds), 1), dtype=np.uint8) if want_extended else None
        self.start = np.zeros(len(self.lens) + 1, dtype=np.uint64)
        self.n = C.c_size_t(0)
        self.st = np.zeros(1, dtype=C2A_DEV_STATS)

    def args(self):
        return (self.params.ctypes.data, self.o.ctypes.data, self.chains.ctypes.data, len(self.chains), self.seeds.ctypes.data, len(self.seeds),
                self.lens.ctypes.data, len(self.lens), self.results.ctypes.data, RESULT_PAIR if self.results.dtype == PAIR else RESULT_FULL,
                self.regs.ctypes.data, C.byref(self.n), self.ext.ctypes.data if self.ext is not None else None, self.start.ctypes.data,
                self.st.ctypes.data)

    def result(self):
        return (self.regs[:self.n.value], self.ext[:len(self.seeds)] if self.ext is not None else None, self.start,
                {k: int(self.st[k][0]) for k in C2A_DEV_STATS.names})


def chain2aln_replay_batch(ctx, params, chains, seeds, lens, results, opt=None, want_extended=True):
    """bsw_chain2aln_replay_batch: chain2aln_replay on the GPU, on the context's own lane (needs c2a_device_load) ->
    (CREG array, extended or None, reg_start, stats dict of C2A_DEV_STATS)"""
    r = C2aReplay(params, chains, seeds, lens, results, opt, want_extended)
    ctx._chk(lib().bsw_chain2aln_replay_batch(ctx.handle, *r.args()), "bsw_chain2aln_replay_batch")
    return r.result()


def c2a_device_load(path=None):
    """bsw_c2a_device_load: the companion library with the replay kernel (None: libbwasw_c2a.so next to the main library)"""
    rc = lib().bsw_c2a_device_load(path.encode() if path else None)
    if rc:
        raise BswError(rc, (lib().bsw_c2a_device_error() or b"").decode())


def set_c2a_device(on):
    """bsw_set_c2a_device: chain2aln jobs started from now on replay on the GPU (refused without a loaded companion)"""
    rc = lib().bsw_set_c2a_device(1 if on else 0)
    if rc:
        raise BswError(rc, (lib().bsw_c2a_device_error() or b"").decode())


def c2a_device():
    return int(lib().bsw_c2a_device())


def sdp_opt(**over):
    """bsw_sdp_default_opt, with fields replaced (patch=0: the call after mate rescue; presorted=1: keep the caller's tie order)"""
    o = np.zeros(1, dtype=SDP_OPT)
    lib().bsw_sdp_default_opt(o.ctypes.data)
    for k, v in over.items():
        o[k] = v
    return o


def sdp_from_cregs(cregs):
    """bsw_sdp_from_cregs: a CREG array (Chain2alnJob.finish) as an SREG array"""
    cregs = np.ascontiguousarray(cregs, dtype=CREG)
    s = np.zeros(len(cregs), dtype=SREG)
    rc = lib().bsw_sdp_from_cregs(cregs.ctypes.data, len(cregs), s.ctypes.data)
    if rc:
        raise BswError(rc, "bsw_sdp_from_cregs")
    return s


def _sdp_stats(st):
    return {k: int(st[k][0]) for k in SDP_STATS.names}


class SdpEngine:
    """One bsw_sdp_eng (pure host): needs() -> RD_PTASK array (a copy; empty: every read is finished), feed(PRESULT array of exactly
    those tasks), collect() -> (SREG array, out_start, stats dict).  Raises BswError with open's text."""

    def __init__(self, params, l_pac, regs, reg_start, lens, opt=None):
        regs, reg_start = np.ascontiguousarray(regs, dtype=SREG), np.ascontiguousarray(reg_start, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        assert len(reg_start) == len(lens) + 1
        o = sdp_opt(**(opt or {}))
        self.handle, self.n_regs, self.n_reads = C.c_void_p(), len(regs), len(lens)
        err = C.create_string_buffer(400)
        rc = lib().bsw_sdp_open(params.ctypes.data, o.ctypes.data, l_pac, regs.ctypes.data, len(regs), reg_start.ctypes.data, lens.ctypes.data,
                                len(lens), C.byref(self.handle), err, 400)
        if rc:
            self.handle = None
            raise BswError(rc, err.value.decode())

    def needs(self):
        t, n = C.c_void_p(), C.c_size_t(0)
        rc = lib().bsw_sdp_needs(self.handle, C.byref(t), C.byref(n))
        if rc:
            raise BswError(rc, "bsw_sdp_needs")
        if not n.value:
            return np.zeros(0, dtype=RD_PTASK)
        return np.frombuffer(C.string_at(t.value, n.value * RD_PTASK.itemsize), dtype=RD_PTASK).copy()

    def feed(self, results):
        results = np.ascontiguousarray(results, dtype=PRESULT)
        rc = lib().bsw_sdp_feed(self.handle, results.ctypes.data, len(results))
        if rc:
            raise BswError(rc, "bsw_sdp_feed")

    def collect(self):
        out = np.zeros(max(self.n_regs, 1), dtype=SREG)
        start = np.zeros(self.n_reads + 1, dtype=np.uint64)
        st = np.zeros(1, dtype=SDP_STATS)
        n = C.c_size_t(0)
        rc = lib().bsw_sdp_collect(self.handle, out.ctypes.data, C.byref(n), start.ctypes.data, st.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_sdp_collect")
        return out[:n.value], start, _sdp_stats(st)

    def close(self):
        h, self.handle = self.handle, None
        if h:
            lib().bsw_sdp_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SdpJob:
    """One bsw_sdp_job: test() polls and moves the job on a round, finish() waits for the remaining rounds, returns the regions and
    frees the job.  A job dropped without finish() is released as a Chain2alnJob is."""

    def __init__(self, ctx, handle, n_regs, n_reads, keep):
        self.ctx, self.handle, self.n_regs, self.n_reads, self._keep = ctx, handle, n_regs, n_reads, keep

    def release(self):
        h, self.handle = self.handle, None
        if h and self.ctx.handle:
            n = C.c_size_t(0)
            if lib().bsw_sdp_finish(h, None, C.byref(n), None, None) == -6:     # BSW_E_BUSY: the job is intact, the places are others'
                self.handle = h
                return
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def test(self):
        rc = lib().bsw_sdp_test(self.handle)
        if rc < 0:
            self.ctx._chk(rc, "bsw_sdp_test")
        return bool(rc)

    def stats(self):
        s = np.zeros(1, dtype=SDP_STATS)
        rc = lib().bsw_sdp_job_stats(self.handle, s.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_sdp_job_stats")
        return _sdp_stats(s)

    def finish(self):
        """-> (SREG array, out_start uint64[n_reads + 1], stats dict).  BswError BSW_E_BUSY leaves the job intact: collect a ticket, call again."""
        out = np.zeros(max(self.n_regs, 1), dtype=SREG)
        start = np.zeros(self.n_reads + 1, dtype=np.uint64)
        st = np.zeros(1, dtype=SDP_STATS)
        n = C.c_size_t(0)
        rc = lib().bsw_sdp_finish(self.handle, out.ctypes.data, C.byref(n), start.ctypes.data, st.ctypes.data)
        if rc != -6:                                        # finish has freed the job
            self.handle, self._keep = None, None
        self.ctx._chk(rc, "bsw_sdp_finish")
        return out[:n.value], start, _sdp_stats(st)


def rescue_opt(**over):
    """bsw_rescue_default_opt (every orientation failed, bwa's other defaults), with fields replaced: low / high / failed take
    four values each"""
    o = np.zeros(1, dtype=RESCUE_OPT)
    lib().bsw_rescue_default_opt(o.ctypes.data)
    for k, v in over.items():
        o[k] = v
    return o


def contig_table(contigs):
    """-> a CONTIG array from None, a CONTIG array or (offset, len) pairs"""
    if contigs is None:
        return np.zeros(0, dtype=CONTIG)
    if isinstance(contigs, np.ndarray) and contigs.dtype == CONTIG:
        return np.ascontiguousarray(contigs)
    return np.array([(int(o), int(n)) for o, n in contigs], dtype=CONTIG)


def _rescue_stats(st):
    return {k: int(st[k][0]) for k in RESCUE_STATS.names}


class RescueEngine:
    """One bsw_rescue_eng (pure host): needs() -> RD_MTASK array (a copy; empty: every direction is finished), feed(MRESULT array of
    exactly those tasks), collect() -> (SREG array, out_start, n_sw int32[n_reads / 2], stats dict).  Raises BswError with open's text."""

    def __init__(self, params, l_pac, regs, reg_start, lens, contigs=None, opt=None):
        regs, reg_start = np.ascontiguousarray(regs, dtype=SREG), np.ascontiguousarray(reg_start, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        o, ct = rescue_opt(**(opt or {})), contig_table(contigs)
        self.handle, self.n_reads = C.c_void_p(), len(lens)
        err = C.create_string_buffer(400)
        rc = lib().bsw_rescue_open(params.ctypes.data, o.ctypes.data, l_pac, ct.ctypes.data, len(ct), regs.ctypes.data, len(regs),
                                   reg_start.ctypes.data, lens.ctypes.data, len(lens), C.byref(self.handle), err, 400)
        if rc:
            self.handle = None
            raise BswError(rc, err.value.decode())

    def out_capacity(self):
        return int(lib().bsw_rescue_out_capacity(self.handle))

    def needs(self):
        t, n = C.c_void_p(), C.c_size_t(0)
        rc = lib().bsw_rescue_needs(self.handle, C.byref(t), C.byref(n))
        if rc:
            raise BswError(rc, "bsw_rescue_needs")
        if not n.value:
            return np.zeros(0, dtype=RD_MTASK)
        return np.frombuffer(C.string_at(t.value, n.value * RD_MTASK.itemsize), dtype=RD_MTASK).copy()

    def feed(self, results):
        results = np.ascontiguousarray(results, dtype=MRESULT)
        rc = lib().bsw_rescue_feed(self.handle, results.ctypes.data, len(results))
        if rc:
            raise BswError(rc, "bsw_rescue_feed")

    def collect(self):
        out = np.zeros(max(self.out_capacity(), 1), dtype=SREG)
        start = np.zeros(self.n_reads + 1, dtype=np.uint64)
        n_sw = np.zeros(self.n_reads // 2, dtype=np.int32)
        st = np.zeros(1, dtype=RESCUE_STATS)
        n = C.c_size_t(0)
        rc = lib().bsw_rescue_collect(self.handle, out.ctypes.data, C.byref(n), start.ctypes.data, n_sw.ctypes.data, st.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_rescue_collect")
        return out[:n.value].copy(), start, n_sw, _rescue_stats(st)

    def close(self):
        h, self.handle = self.handle, None
        if h:
            lib().bsw_rescue_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RescueJob:
    """One bsw_rescue_job: test() polls and moves the job on a round, finish() waits for the remaining rounds, returns the regions
    and frees the job.  A job dropped without finish() is released as an SdpJob is."""

    def __init__(self, ctx, handle, n_reads, keep):
        self.ctx, self.handle, self.n_reads, self._keep = ctx, handle, n_reads, keep

    def release(self):
        h, self.handle = self.handle, None
        if h and self.ctx.handle:
            n = C.c_size_t(0)
            if lib().bsw_rescue_finish(h, None, 0, C.byref(n), None, None, None) == -6:     # BSW_E_BUSY: the job is intact, the places are others'
                self.handle = h
                return
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def test(self):
        rc = lib().bsw_rescue_test(self.handle)
        if rc < 0:
            self.ctx._chk(rc, "bsw_rescue_test")
        return bool(rc)

    def stats(self):
        s = np.zeros(1, dtype=RESCUE_STATS)
        rc = lib().bsw_rescue_job_stats(self.handle, s.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_rescue_job_stats")
        return _rescue_stats(s)

    def out_capacity(self):
        return int(lib().bsw_rescue_job_out_capacity(self.handle))

    def finish(self):
        """-> (SREG array, out_start uint64[n_reads + 1], n_sw int32[n_reads / 2], stats dict).  BswError BSW_E_BUSY leaves the job
        intact: collect a ticket, call again."""
        out = np.zeros(max(self.out_capacity(), 1), dtype=SREG)
        start = np.zeros(self.n_reads + 1, dtype=np.uint64)
        n_sw = np.zeros(self.n_reads // 2, dtype=np.int32)
        st = np.zeros(1, dtype=RESCUE_STATS)
        n = C.c_size_t(0)
        rc = lib().bsw_rescue_finish(self.handle, out.ctypes.data, len(out), C.byref(n), start.ctypes.data, n_sw.ctypes.data, st.ctypes.data)
        if rc != -6:                                        # finish has freed the job
            self.handle, self._keep = None, None
        self.ctx._chk(rc, "bsw_rescue_finish")
        return out[:n.value].copy(), start, n_sw, _rescue_stats(st)


class HostArena:
    """Pinned (DMA-able) host memory from bsw_host_alloc, viewed as a numpy array.  Sequences and result
    arrays kept in such memory cross PCIe without a host copy (bsw_submit's direct path)."""

    def __init__(self, nbytes):
        self.ptr = lib().bsw_host_alloc(nbytes)
        if not self.ptr:
            raise BswError(-5, "bsw_host_alloc(%d)" % nbytes)
        self.nbytes = nbytes
        self.u8 = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def view(self, dtype, count, offset=0):
        return self.u8[offset:offset + count * np.dtype(dtype).itemsize].view(dtype)

    def free(self):
        if self.ptr:
            self.u8 = None
            lib().bsw_host_free(self.ptr)
            self.ptr = None


def host_register(arr):
    """Pin an existing numpy array for DMA (bsw_host_register); returns the rc."""
    return lib().bsw_host_register(arr.ctypes.data, arr.nbytes)


def host_unregister(arr):
    return lib().bsw_host_unregister(arr.ctypes.data)


def scalar_stats():
    a, b = C.c_uint64(0), C.c_uint64(0)
    lib().bsw_scalar_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def set_rtl_packed(on):
    """Process-wide opt-in: variant RTL's 72- and 136-column 8-bit lane classes on the packed two-seeds-per-lane kernel
    (bsw_set_rtl_packed; initially BSW_RTL_PACKED=1).  Applies to launches enqueued afterwards."""
    lib().bsw_set_rtl_packed(1 if on else 0)


def rtl_packed():
    return bool(lib().bsw_rtl_packed())


def rtl_packed_stats():
    """Launches of the packed RTL kernel so far: (72 columns shared penalties, 72 separate, 136 shared, 136 separate)."""
    a = np.zeros(4, dtype=np.uint64)
    assert lib().bsw_rtl_packed_stats(a.ctypes.data, 4) == 4
    return tuple(int(x) for x in a)


ALIGN_LONG_MAX_QLEN = 8191


def set_align_long(mode):
    """Process-wide opt-in: ksw_align2 and everything built on it accept queries of 1 025 to 8 191 bases and run them on
    bsw_align_long_kernel (1); every alignment runs on that kernel (2); 0: off (bsw_set_align_long; initially BSW_ALIGN_LONG).
    Applies to the calls that enter the library afterwards."""
    lib().bsw_set_align_long(int(mode))


def align_long():
    return int(lib().bsw_align_long())


def align_long_stats():
    """Launches of bsw_align_long_kernel so far, per class: 8-bit mode slen bound 16 .. 512, then 16-bit mode 32 .. 1 024."""
    n = lib().bsw_align_long_stats(None, 0)
    a = np.zeros(n, dtype=np.uint64)
    assert lib().bsw_align_long_stats(a.ctypes.data, n) == n
    return tuple(int(x) for x in a)


def refbatch_encode(params, tasks):
    words = np.zeros(REFBATCH_IN_WORDS, dtype=np.uint32)
    n = lib().bsw_refbatch_encode(params.ctypes.data, tasks.ctypes.data, len(tasks), words.ctypes.data)
    if n < 0:
        raise BswError(n, "bsw_refbatch_encode")
    return words, n


def refbatch_decode(words):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    p = np.zeros(1, dtype=PARAMS)
    tasks = np.zeros(REFBATCH_MAX_TASKS, dtype=TASK)
    seqbuf = np.zeros(REFBATCH_IN_WORDS * 8 + 64, dtype=np.uint8)
    n = lib().bsw_refbatch_decode(words.ctypes.data, p.ctypes.data, tasks.ctypes.data, len(tasks), seqbuf.ctypes.data, seqbuf.size)
    if n < 0:
        raise BswError(n, "bsw_refbatch_decode")
    return p, tasks[:n], seqbuf


def refbatch_encode_results(res):
    words = np.zeros(REFBATCH_OUT_WORDS, dtype=np.uint32)
    n = lib().bsw_refbatch_encode_results(res.ctypes.data, len(res), words.ctypes.data)
    if n < 0:
        raise BswError(n, "bsw_refbatch_encode_results")
    return words


def refbatch_decode_results(words, n):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    res = np.zeros(n, dtype=RESULT)
    rc = lib().bsw_refbatch_decode_results(words.ctypes.data, n, res.ctypes.data)
    if rc < 0:
        raise BswError(rc, "bsw_refbatch_decode_results")
    return res


PLAN_SEGS = 26


def plan_batch(params, tasks, kernel=KERNEL_AUTO, pack_threads=1):
    """Batch manager's launch plan for a task batch (host only; the order is the host replay of the device's
    binning rules).  Returns (order, seg, seq_words)."""
    order = np.zeros(int(lib().bsw_plan_order_capacity(len(tasks))), dtype=np.uint32)
    seg = np.zeros(PLAN_SEGS + 1, dtype=np.uint32)
    w = lib().bsw_plan_batch(params.ctypes.data, tasks.ctypes.data, len(tasks), kernel, pack_threads, order.ctypes.data, seg.ctypes.data)
    if w < 0:
        raise BswError(int(w), "bsw_plan_batch")
    return order, seg, int(w)


def pack_bases(bases):
    """Device sequence format of one sequence (see bsw_pack_bases).  Returns (uint64 words, has_N)."""
    b = np.ascontiguousarray(bases, dtype=np.uint8)
    words = np.zeros((len(b) + 15) // 16, dtype=np.uint64)
    rc = lib().bsw_pack_bases(b.ctypes.data if len(b) else None, len(b), words.ctypes.data if len(words) else None)
    if rc < 0:
        raise BswError(rc, "bsw_pack_bases")
    return words, bool(rc)


def pac_get_seq(pac, l_pac, beg, end):
    """bns_get_seq on a 2-bit packed reference (numpy uint8 array)."""
    dst = np.zeros(max(abs(end - beg), 1), dtype=np.uint8)
    n = lib().bsw_pac_get_seq(l_pac, pac.ctypes.data, beg, end, dst.ctypes.data)
    if n < 0:
        raise BswError(int(n), "bsw_pac_get_seq")
    return dst[:n]


def infer_bw(l1, l2, score, a, q, r):
    """mem_reg2aln's infer_bw (bsw_infer_bw)."""
    return int(lib().bsw_infer_bw(l1, l2, score, a, q, r))


def patch_pretest(params, l_pac, a, b):
    """mem_patch_reg up to bwa_gen_cigar2 (bsw_patch_pretest; a, b: PREG records): (1, w_) when the alignment runs, else (0, 0)."""
    a, b = np.ascontiguousarray(a, dtype=PREG), np.ascontiguousarray(b, dtype=PREG)
    w = C.c_int(0)
    r = lib().bsw_patch_pretest(params.ctypes.data, l_pac, a.ctypes.data, b.ctypes.data, C.byref(w))
    return int(r), int(w.value)


def patch_decide(a, b, gscore):
    """mem_patch_reg behind bwa_gen_cigar2 (bsw_patch_decide): its return value for the alignment's score."""
    a, b = np.ascontiguousarray(a, dtype=PREG), np.ascontiguousarray(b, dtype=PREG)
    return int(lib().bsw_patch_decide(a.ctypes.data, b.ctypes.data, int(gscore)))


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir (bsw_infer_dir): (orientation 0..3, distance)."""
    d = C.c_int64(0)
    r = lib().bsw_infer_dir(l_pac, b1, b2, C.byref(d))
    return int(r), int(d.value)


def matesw_windows(anchor_rb, l_ms, l_pac, low, high, failed):
    """mem_matesw's windows for the four orientations (bsw_matesw_windows).  low / high / failed: four values each.
    Returns dict of int arrays rb, re, is_rev, skip (index = orientation)."""
    lo, hi, fa = (np.ascontiguousarray(x, dtype=np.int32) for x in (low, high, failed))
    assert lo.size == hi.size == fa.size == 4
    rb, re = np.zeros(4, np.int64), np.zeros(4, np.int64)
    is_rev, skip = np.zeros(4, np.int32), np.zeros(4, np.int32)
    rc = lib().bsw_matesw_windows(anchor_rb, l_ms, l_pac, lo.ctypes.data, hi.ctypes.data, fa.ctypes.data, rb.ctypes.data,
                                  re.ctypes.data, is_rev.ctypes.data, skip.ctypes.data)
    if rc:
        raise BswError(rc, "bsw_matesw_windows")
    return {"rb": rb, "re": re, "is_rev": is_rev, "skip": skip}


def pack_pac(bases):
    """ACGT codes -> bwa .pac layout (4 bases per byte, first base in the top two bits)."""
    b = np.asarray(bases, dtype=np.uint8)
    pad = (-len(b)) % 4
    b4 = np.concatenate([b, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    return (b4[:, 0] << 6 | b4[:, 1] << 4 | b4[:, 2] << 2 | b4[:, 3]).astype(np.uint8)


def seeds_to_tasks(params, pac, l_pac, reads, seeds):
    """mem_chain2aln glue for single-seed chains: reads = list of base arrays, seeds = SEED array (one per read).
    Returns (tasks, keepalive) with the sequences laid out by bsw_seed_to_task."""
    L = lib()
    n = len(reads)
    tasks = np.zeros(n, dtype=TASK)
    keep = []
    for i in range(n):
        q = np.ascontiguousarray(reads[i], dtype=np.uint8)
        rmax = np.zeros(2, dtype=np.int64)
        rc = L.bsw_chain_window(params.ctypes.data, seeds[i:i + 1].ctypes.data, 1, len(q), l_pac, rmax.ctypes.data)
        if rc:
            raise BswError(rc, "bsw_chain_window")
        rseq = pac_get_seq(pac, l_pac, int(rmax[0]), int(rmax[1]))
        rseq = np.ascontiguousarray(rseq)
        scratch = np.zeros(L.bsw_seed_scratch_bytes(seeds[i:i + 1].ctypes.data, int(rmax[0])) + 8, dtype=np.uint8)
        rc = L.bsw_seed_to_task(params.ctypes.data, seeds[i:i + 1].ctypes.data, len(q), q.ctypes.data, int(rmax[0]), int(rmax[1]),
                                rseq.ctypes.data, scratch.ctypes.data, scratch.size, i, tasks[i:i + 1].ctypes.data)
        if rc:
            raise BswError(rc, "bsw_seed_to_task")
        keep.append((q, rseq, scratch))
    return tasks, keep


def results_to_alnregs(seeds, results):
    out = np.zeros(len(seeds), dtype=ALNREG)
    for i in range(len(seeds)):
        lib().bsw_result_to_alnreg(seeds[i:i + 1].ctypes.data, results[i:i + 1].ctypes.data, out[i:i + 1].ctypes.data)
    return out


def shard_indices(n, world, rank, chunk=65536):
    """Per-read task shard of rank `rank`: task k -> rank (k // chunk) % world.
    Tasks are independent, so there is no exchange step and no data-path collective."""
    idx = np.arange(n, dtype=np.int64)
    return idx[(idx // chunk) % world == rank]


def task_seq(tasks, i, field, lenfield):
    """Read one sequence of task i back as a numpy array (for tests / fixtures)."""
    n = int(tasks[i][lenfield])
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.ctypeslib.as_array(C.cast(int(tasks[i][field]), C.POINTER(C.c_uint8)), shape=(n,)).copy()
