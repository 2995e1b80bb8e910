"""The kernel ledger: for every kernel compiled into libbwasw_mi355.so, a small workload that dispatches it and the reference it
must match.

tests/test_kernel_ledger_cpu.py checks that the ledger covers the build (the .kd symbols of the gfx950 code objects, demangled)
and that every workload is non-vacuous at the edge of its class; tests/test_gpu_kernel_ledger.py runs the cases group by group
(a group = one set of routing switches, read once per process) under a kernel trace, proves that each group dispatched the
kernels its cases name and compares every result with the reference (tests/_kernel_ledger_run.py).

A case:
  name     unique
  targets  normalised kernel names (demangled, without `void ` and the argument list) the case must dispatch
  env      routing switches the case needs ({} for product routes)
  ctx      BswContext settings (kernel, streams, chunk_tasks, result_format)
  entry    extend_pairs | upload_run (upload / run / download) | packed_registered (extend_pairs_packed from registered memory)
           | wire (bsw_refbatch_run) | global_batch | align_batch | cigar_ref_batch
           | reads_upload_async (bsw_reads_upload_start / bsw_reads_wait / bsw_reads_image)
  params   overrides of default_params, and the matrix (a, b, n) in `mat`
  gen      seeded generator: gen(rng) -> the workload of the entry point
  ref      what the results are compared with, bit for bit
  seed     the generator's seed
"""
import numpy as np

H, M, RTL = 0, 1, 2
AUTO, WAVE, LANE = 0, 1, 2             # host.KERNEL_*
PAIR = 1                               # host.RESULT_PAIR
NS = "bsw::"


def wave(c, v):
    return NS + "bsw_wave_kernel<%d, %d>" % (c, v)


def quad(s, v):
    return NS + "bsw_quad_kernel<%d, %d>" % (s, v)


def long_(v, wpb):
    return NS + "bsw_long_kernel<%d, %d>" % (v, wpb)


def lane(qb, v, sym, b8, wps):
    return NS + "bsw_lane_kernel<%d, %d, %s, %s, %d>" % (qb, v, _b(sym), _b(b8), wps)


def lane2(qb, wps, vm, sym, fused):
    return NS + "bsw_lane2_kernel<%d, %d, %s, %s, %s>" % (qb, wps, _b(vm), _b(sym), _b(fused))


def lane2_rtl(qb, wps, sym):
    return NS + "bsw_lane2_rtl_kernel<%d, %d, %s>" % (qb, wps, _b(sym))


def align_long(byte):
    return NS + "bsw_align_long_kernel<%s>" % _b(byte)


def reads_pack():
    return NS + "bsw_reads_pack_kernel"


def lane2l(qb, vm, sym):
    return NS + "bsw_lane2l_kernel<%d, 1, %s, %s>" % (qb, _b(vm), _b(sym))


def lane2g(ns, wps, vm, sym, fused):
    return NS + "bsw_lane2g_kernel<%d, %d, %s, %s, %s>" % (ns, wps, _b(vm), _b(sym), _b(fused))


def _b(x):
    return "true" if x else "false"


def normalise(name):
    """a demangled kernel name as the trace and c++filt print it -> `bsw::kernel<args>`"""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    return name.split("(", 1)[0].strip()


# Compiled kernels no product path or switch can dispatch: {name: reason}.  Empty: every compiled kernel has a case.
UNREACHED = {}

# ---- extension workloads (seeds of make_tasks) ------------------------------------------------------------------------------

WAVE_COLS = (64, 128, 192, 256, 512, 1024)        # bsw_wave_kernel<C>: C * 64 columns (bsw_long_kernel: 2 048 and 8 192)
L16_COLS = 136                                    # the 16-bit lane class (the 8-bit ones: 72, 136, 232 columns)


def _target(rng, q_len, tfac=1.3):
    return rng.integers(0, 4, max(0, int(q_len * tfac) + int(rng.integers(0, 12)))).astype(np.uint8)


def _query(rng, t, ql, sub, indel, junk, perfect):
    """ql bases read off target t (substitutions, short indels, a junk tail or a wholly junk query)"""
    if perfect:
        return t[:ql].copy() if len(t) >= ql else np.concatenate([t, rng.integers(0, 4, ql - len(t))]).astype(np.uint8)
    r = rng.random()
    if r < junk:
        return rng.integers(0, 4, ql).astype(np.uint8)
    q = np.concatenate([t[:ql], rng.integers(0, 4, max(0, ql - len(t)))]).astype(np.uint8)
    q = np.where(rng.random(ql) < sub, (q + rng.integers(1, 4, ql)) & 3, q).astype(np.uint8)
    for _ in range(int(rng.poisson(indel * ql))):
        at, k = int(rng.integers(0, ql)), int(rng.integers(1, 8))
        if rng.random() < 0.5:
            q = np.concatenate([q[:at], rng.integers(0, 4, k).astype(np.uint8), q[at:]])[:ql]
        else:
            q = np.concatenate([q[:at], q[at + k:], rng.integers(0, 4, k).astype(np.uint8)])[:ql]
    if r < junk * 2 and ql > 20:                       # a junk tail: where z-drop ends the extension
        cut = int(rng.integers(ql // 2, ql))
        q[cut:] = rng.integers(0, 4, ql - cut)
    return q.astype(np.uint8)


def seeds(rng, n, bands, a=1, b=4, bits=0, nrate=0.01, sub=0.03, indel=0.02, junk=0.15, share16=0.0, big_h0=300):
    """n seeds whose longer side falls in one of `bands` [(lo, hi)], a third of them at hi (hi + 1 = the class's columns).
    bits = 8: h0 + (lq + rq) a + b <= 255 (half exactly 255, some of those a perfect match to the end); bits = 16: the top
    h0 + (lq + rq) a in 256 .. 64 999 (half within 64 of 65 000); bits = 0: h0 in 1 .. 60 and now and then big_h0.  share16: that
    share of an 8-bit workload's seeds is made 16-bit instead.  Ns in queries and targets at nrate."""
    out = []
    for k in range(n):
        lo, hi = bands[k % len(bands)]
        r = rng.random()
        sides = "lr" if r < 0.7 else "l" if r < 0.85 else "r"
        long_side = sides[int(rng.integers(0, len(sides)))]
        big = hi if (k // len(bands)) % 3 == 0 else int(rng.integers(lo, hi + 1))
        lens = {long_side: big}
        sb = bits
        if bits == 8 and rng.random() < share16:
            sb = 16
        for sd in sides:
            if sd == long_side:
                continue
            room = big
            if sb == 8:
                room = min(big, (254 - b) // a - big - 1)
            lens[sd] = int(rng.integers(1, max(1, room) + 1)) if room >= 1 else 0
        lens = {sd: ln for sd, ln in lens.items() if ln > 0}
        tot = sum(lens.values()) * a
        perfect = False
        if sb == 8:
            assert tot + b + 1 <= 255, (lens, a, b)
            if rng.random() < 0.5:
                h0 = 255 - b - tot
                perfect = rng.random() < 0.3
            else:
                h0 = int(rng.integers(1, 255 - b - tot + 1))
        elif sb == 16:
            h0 = 64999 - tot - int(rng.integers(0, 64)) if rng.random() < 0.5 else int(rng.integers(max(1, 256 - tot), 3000))
        else:
            h0 = big_h0 if rng.random() < 0.03 else int(rng.integers(1, 61))
        s = {"h0": h0, "init_score": -1 if rng.random() < 0.8 else int(rng.integers(-1, 50)), "tag": int(rng.integers(0, 2 ** 32))}
        for sd, ln in lens.items():
            t = _target(rng, ln)
            q = _query(rng, t, ln, sub, indel, junk, perfect)
            if nrate > 0 and not perfect:
                q[rng.random(ln) < nrate] = 4
                t[rng.random(len(t)) < nrate] = 4
            s[sd + "q"], s[sd + "t"] = q, t
        out.append(s)
    return out


def _ext(name, targets, n, bands, kw, params, env=None, ctx=None, entry="upload_run", seed=0, edges=None, ref=None):
    """an extension case: n seeds of seeds(rng, n, bands, **kw); `edges`: what the CPU test requires of the workload"""
    p = dict(params)
    kw = dict(kw or {})
    if "mat" in p:
        kw.update(a=p["mat"][0], b=p["mat"][1])
    variant = p.get("variant", H)
    if edges is None:
        edges = ("last_col", "retry", "zdrop", "qn", "tn") + (("bound8",) if kw.get("bits") == 8 else ()) + \
                (("bound16",) if kw.get("share16") else ())
    return dict(name=name, targets=tuple(targets), env=dict(env or {}), ctx=dict(ctx or dict(kernel=LANE)), entry=entry, params=p,
                gen=lambda rng: seeds(rng, n, bands, **kw), bands=tuple(bands), kw=kw,
                ref=ref or ("rtl_ref.pair_batch" if variant == RTL else "oracle.pair_batch"), seed=seed, edges=edges)


SYM = dict(o_del=6, e_del=1, o_ins=6, e_ins=1)
ASYM = dict(o_del=5, e_del=2, o_ins=7, e_ins=1)
EXTP = dict(w=10, max_band_try=3, zdrop=40)       # a narrow first band (retries) and a z-drop that stops junk tails


def _pen(vm, sym):
    return dict(SYM if sym else ASYM, variant=M if vm else H)


CASES = []
_seed = [9100]


def add(case):
    _seed[0] += 1
    if not case["seed"]:
        case["seed"] = _seed[0]
    CASES.append(case)


# general kernels (bsw_wave_kernel): every class up to its last column, one case per variant
_wbands = [(c0, c1 - 1) for c0, c1 in zip((1,) + WAVE_COLS[:-1], WAVE_COLS)]
for v in (H, M, RTL):
    add(_ext("general_v%d" % v, [wave(c // 64, v) for c in WAVE_COLS] + ([NS + "bsw_pack_kernel", NS + "bsw_bin_count", NS + "bsw_bin_scan",
                                                                              NS + "bsw_bin_scatter"] if v == H else []),
             360, _wbands, dict(nrate=0.01), dict(EXTP, variant=v, **(SYM if v != M else ASYM)),
             ctx=dict(kernel=WAVE), entry="extend_pairs"))
# the LDS-row kernel: 2 048 columns (four waves per block) and 8 192 (one)
for v in (H, M, RTL):
    add(_ext("long_v%d" % v, [long_(v, 4), long_(v, 1)], 12, [(1024, 2047), (2048, 8191)], dict(nrate=0.002),
             dict(w=40, max_band_try=2, zdrop=100, variant=v, **ASYM), ctx=dict(kernel=WAVE), entry="extend_pairs"))
# the four-seeds-per-wavefront kernel on every class up to 256 columns (BSW_QUAD=1: by default only from 8 192 seeds)
for v in (H, M, RTL):
    add(_ext("quad_v%d" % v, [quad(s, v) for s in (2, 4, 6, 8)], 400, _wbands[:4], {}, dict(EXTP, variant=v, **ASYM),
             env=dict(BSW_QUAD="1"), ctx=dict(kernel=WAVE), entry="extend_pairs"))

# the one-seed-per-lane kernel (bsw_lane_kernel): every trigger of lane2_params_ok failing, each on the 136- and 232-column
# 8-bit classes and with 16-bit seeds (the 16-bit class always runs this kernel).  a + b >= 256 cannot be built: the matrix is
# int8, so a <= 127 and b <= 128.
_fb = [  # name, params, matrix (a, b, n)
    ("fallback_n_score_positive", dict(SYM, variant=H), (1, 4, 1)),
    ("fallback_n_penalty_above_b", dict(ASYM, variant=M), (1, 4, -6)),
    ("fallback_del_gap_256", dict(o_del=250, e_del=6, o_ins=5, e_ins=2, variant=H), (1, 4, -1)),
    ("fallback_gap_256_sym", dict(o_del=200, e_del=60, o_ins=200, e_ins=60, variant=M), (1, 4, -1)),
    ("fallback_rtl_sym", dict(SYM, variant=RTL), (1, 4, -1)),
    ("fallback_rtl_asym", dict(ASYM, variant=RTL), (1, 4, -1)),
]
for name, pen, mat in _fb:
    v, sym = pen["variant"], pen["o_del"] == pen["o_ins"] and pen["e_del"] == pen["e_ins"]
    tg = [lane(17, v, sym, True, 4), lane(29, v, sym, True, 3), lane(17, v, sym, False, 2)]
    if name == "fallback_rtl_sym":
        tg.append(NS + "bsw_pair_finalize")
    c = _ext(name, tg, 600, [(1, 135), (136, 231)], dict(a=mat[0], b=mat[1], bits=8, share16=0.25), dict(EXTP, mat=mat, **pen))
    if "gap_256" in name:                               # (a gap that costs >= 256 never pays: no band ever needs a retry)
        c["edges"] = tuple(e for e in c["edges"] if e != "retry")
    add(c)
# BSW_NO_LANE2L=1: the 232-column class on the one-seed-per-lane kernel under product parameters
for vm, sym in ((False, True), (True, False)):
    add(_ext("no_lane2l_%s_%s" % ("m" if vm else "h", "sym" if sym else "asym"), [lane(29, M if vm else H, sym, True, 3)],
             400, [(136, 231)], dict(bits=8), dict(EXTP, **_pen(vm, sym)), env=dict(BSW_NO_LANE2L="1")))

# the two-seeds-per-lane kernels: 72 columns (a chunk of short sides only), 136 columns unrolled and 232 looped in one chunk
# (their lane launches form a chain: bsw_wait_count in front of every follower)
for vm in (False, True):
    for sym in (True, False):
        tag = "%s_%s" % ("m" if vm else "h", "sym" if sym else "asym")
        add(_ext("lane2_72_" + tag, [lane2(9, 3, vm, sym, False)], 800, [(1, 71)], dict(a=2, b=5, bits=8),
                 dict(EXTP, mat=(2, 5, -1), **_pen(vm, sym))))
        add(_ext("lane2_136_232_" + tag, [lane2(17, 2, vm, sym, False), lane2l(29, vm, sym)] + ([NS + "bsw_wait_count"] if not vm and sym else []),
                 800, [(72, 135), (136, 231)], dict(bits=8), dict(EXTP, **_pen(vm, sym))))
        # BSW_LANE2L_NARROW=1: the 136-column class through the looped kernel
        add(_ext("lane2l_narrow_" + tag, [lane2l(17, vm, sym)], 600, [(72, 135)], dict(bits=8), dict(EXTP, **_pen(vm, sym)),
                 env=dict(BSW_LANE2L_NARROW="1")))
        # the lane kernels' fused launch: left then right sides of a seed (sides <= 135)
        add(_ext("lane_fused_" + tag, [lane2(17, 2, vm, sym, True)], 800, [(1, 71), (72, 135)], dict(a=1, b=3, bits=8),
                 dict(EXTP, mat=(1, 3, -1), **_pen(vm, sym)), env=dict(BSW_GROUP="0", BSW_LANE_FUSE="1")))
        # the group kernel (eight lanes per seed pair): a launch per side and class (three stripes <= 192 columns, four for 232)
        add(_ext("group_" + tag, [lane2g(3, 3, vm, sym, False), lane2g(4, 2, vm, sym, False)],
                 600, [(1, 135), (136, 231)], dict(bits=8), dict(EXTP, **_pen(vm, sym)),
                 env=dict(BSW_GROUP="1", BSW_GROUP_FUSE="0")))
        # ... and fused: the chunk's widest class picks the stripes, so a chunk of sides <= 135 and one with wider sides
        add(_ext("group_fused_narrow_" + tag, [lane2g(3, 3, vm, sym, True)], 600, [(1, 71), (72, 135)], dict(bits=8),
                 dict(EXTP, **_pen(vm, sym)), env=dict(BSW_GROUP="1", BSW_GROUP_FUSE="1")))
        add(_ext("group_fused_wide_" + tag, [lane2g(4, 2, vm, sym, True)], 600, [(1, 135), (136, 231)], dict(bits=8),
                 dict(EXTP, **_pen(vm, sym)), env=dict(BSW_GROUP="1", BSW_GROUP_FUSE="1")))

# BSW_RTL_PACKED=1: variant RTL on the two-seeds-per-lane kernels, shared and separate gap penalties.  As for lane2_72_* above
# the 72-column class is launched only for a chunk whose 8-bit sides are all short (a mixed chunk folds it into the 136-column
# class), so each penalty set takes a chunk of short sides and a mixed one.  Every default edge is kept: the RTL reference
# produces each of them on these workloads.
for sym in (True, False):
    tag = "sym" if sym else "asym"
    pen = dict(EXTP, mat=(1, 4, -1), variant=RTL, **(SYM if sym else ASYM))
    add(_ext("rtl_packed_72_" + tag, [lane2_rtl(9, 3, sym)], 300, [(1, 71)], dict(bits=8), pen, env=dict(BSW_RTL_PACKED="1")))
    add(_ext("rtl_packed_136_" + tag, [lane2_rtl(17, 2, sym)], 600, [(1, 71), (72, 135)], dict(bits=8), pen, env=dict(BSW_RTL_PACKED="1")))

# BSW_NSPLIT=1: lane seeds with an N in a query go to the general kernel's N list (bsw_nlist_count sizes its launch)
add(_ext("nsplit", [NS + "bsw_nlist_count"], 800, [(1, 135)], dict(bits=8, nrate=0.02), dict(EXTP, **ASYM),
         env=dict(BSW_NSPLIT="1")))
# the pair format: the general kernels' seeds copied into the dense pair records
add(_ext("pair_format", [NS + "bsw_pairs_from_results"], 400, _wbands[:3], {}, dict(EXTP, **SYM),
         ctx=dict(kernel=WAVE, result_format=PAIR), entry="extend_pairs"))
# packed input in registered memory: DMA'd as it lies, the task records rebased on the device
add(_ext("packed_registered", [NS + "bsw_rebase_kernel"], 600, [(1, 71), (72, 135)], dict(bits=8, share16=0.2),
         dict(EXTP, **SYM), ctx=dict(kernel=AUTO, chunk_tasks=8192, streams=3), entry="packed_registered"))
# the reference's wire format (256 KiB task batch in, 16 KiB result batch out)
add(_ext("wire", [NS + "bsw_wire_pack_kernel", NS + "bsw_wire_results_kernel"], 500, [(1, 60), (61, 131)],
         dict(big_h0=127),                                 # (the wire format's h0 is 1 .. 127: the reference's int8 datapath)
         dict(variant=H, zdrop=0), ctx=dict(kernel=AUTO), entry="wire", edges=("last_col", "qn", "tn"), ref="oracle.pair_batch (pair fields)"))

# ---- global alignment, local alignment, CIGAR against the resident reference ------------------------------------------------

GLOBAL_COLS = (64, 128, 256, 512, 1024)


def _mutated(rng, t, ql, sub=0.04, indel=0.02):
    import _gen
    return _gen.mutate(rng, t, ql, sub, indel)


def global_pairs(rng, qlens, nper, nrate=0.02):
    pairs, ws = [], []
    for ql in qlens:
        for k in range(nper):
            t = rng.integers(0, 4, max(1, ql + int(rng.integers(-ql // 20 - 1, ql // 20 + 2)))).astype(np.uint8)
            q = _mutated(rng, t, ql)
            q[rng.random(len(q)) < nrate] = 4
            pairs.append((q, t))
            ws.append(int(rng.choice([0, 3, 20, 100, 600, 2100, ql + 5])))
    return pairs, ws


def _glob(name, targets, gen, params, env=None, seed=0):
    return dict(name=name, targets=tuple(targets), env=dict(env or {}), ctx=dict(kernel=AUTO), entry="global_batch", params=dict(params),
                gen=gen, ref="oracle.global2 (score; CIGAR where the band holds a path)", seed=seed, edges=())


add(_glob("global", [NS + "bsw_global_kernel<%d>" % (c // 64) for c in GLOBAL_COLS],
          lambda rng: global_pairs(rng, [1, 2] + [c - 1 for c in GLOBAL_COLS] + [c for c in GLOBAL_COLS[:-1]] + [100, 700], 6), ASYM))
add(_glob("global_long", [NS + "bsw_global_long_kernel<4>", NS + "bsw_global_long_kernel<1>"],
          lambda rng: global_pairs(rng, [1024, 2047, 4096, 8191], 4), SYM))

ALIGN_CLASSES = [(1, 8), (1, 10), (1, 16), (1, 32), (1, 64), (0, 16), (0, 20), (0, 32), (0, 64), (0, 128)]   # (byte, slen)
XB, XSTOP, XSUBO, XSTART = 0x10000, 0x20000, 0x40000, 0x80000


def align_pairs(rng):
    """for every class of both modes: queries of its last length and one more than the class before, with random flags"""
    pairs, xt = [], []
    for byte, slen in ALIGN_CLASSES:
        top = slen * (16 if byte else 8)
        prev = max([s * (16 if byte else 8) for b2, s in ALIGN_CLASSES if b2 == byte and s < slen] or [0])
        for ql in (top, prev + 1, int(rng.integers(prev + 1, top + 1))):
            for k in range(3):
                t = rng.integers(0, 4, int(rng.integers(ql, 2 * ql + 40))).astype(np.uint8)
                a0 = int(rng.integers(0, len(t) - ql + 1))
                q = _mutated(rng, t[a0:a0 + ql], ql, 0.05 if k else 0.3, 0.02)
                if k == 2:
                    q[rng.integers(0, ql)] = 4
                x = (XB if byte else 0) | int(rng.choice([0, XSTART, XSUBO | 19, XSUBO | XSTART | 19, XSTOP | 25]))
                pairs.append((q, t))
                xt.append(x)
    return pairs, xt


add(dict(name="align", targets=tuple(NS + "bsw_align_kernel<%d, %s>" % (s, _b(b)) for b, s in ALIGN_CLASSES), env={}, ctx=dict(kernel=AUTO),
         entry="align_batch", params=dict(SYM), gen=align_pairs, ref="oracle.align2_batch (every field)", seed=0, edges=()))


ALIGN_LONG_QLENS = (1025, 2048, 2049, 4097, 8191)     # the first long query, and both sides of the class edges above it


def align_long_pairs(rng):
    """per length and mode two queries (the second with an N), flags drawn as in align_pairs; the target is a mutated piece of
    the query between two flanks, a few hundred bases: the rows of the alignment are the query's, its time the target's"""
    pairs, xt = [], []
    for ql in ALIGN_LONG_QLENS:
        for byte in (1, 0):
            for k in range(2):
                q = rng.integers(0, 4, ql).astype(np.uint8)
                a0 = int(rng.integers(0, ql - 300 + 1))
                piece = _mutated(rng, q[a0:a0 + 300], 300, 0.05, 0.02)
                t = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 60))), piece, rng.integers(0, 4, int(rng.integers(0, 60)))]).astype(np.uint8)
                if k == 1:
                    q[rng.integers(0, ql)] = 4
                x = (XB if byte else 0) | int(rng.choice([0, XSTART, XSUBO | 19, XSUBO | XSTART | 19, XSTOP | 25]))
                pairs.append((q, t))
                xt.append(x)
    return pairs, xt


# BSW_ALIGN_LONG=1: queries of more than 1 024 bases on the LDS-row kernel, both modes
add(dict(name="align_long", targets=(align_long(True), align_long(False)), env=dict(BSW_ALIGN_LONG="1"), ctx=dict(kernel=AUTO),
         entry="align_batch", params=dict(SYM), gen=align_long_pairs, ref="oracle.align2_batch (every field)", seed=0, edges=()))

READS_LENS = (1, 15, 16, 17, 31, 32, 33, 150, 250)


def reads_block(rng):
    """(raw, lens, offs): about 300 reads back to back in one raw buffer (read i = raw[offs[i]:offs[i] + lens[i]]), Ns at 2 %.
    Sixteen reads of 17 bases in a row put a read's first byte at every offset modulo 16 of the raw buffer, whether the upload
    sends the buffer as it lies or gathers the reads (both keep them back to back)."""
    lens = [int(n) for n in READS_LENS] * 28 + [int(n) for n in rng.integers(1, 401, 32)]
    rng.shuffle(lens)
    lens = np.array(lens[:150] + [17] * 16 + lens[150:], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    raw = rng.integers(0, 4, int(lens.sum())).astype(np.uint8)
    raw[rng.random(len(raw)) < 0.02] = 4
    return raw, lens, offs


def reads_image(raw, lens, offs, slack):
    """the block's device image in numpy: 16 bases per uint64, base k in bits [4k, 4k+3], codes above 4 stored as 4, every read
    on a word boundary, the nibbles behind a read's last base zero, `slack` zero words in front and behind"""
    words = [np.zeros(slack, np.uint64)]
    for n, o in zip(lens, offs):
        b = np.zeros((int(n) + 15) // 16 * 16, dtype=np.uint64)
        b[:n] = np.minimum(raw[o:o + n], 4)
        words.append((b.reshape(-1, 16) << (4 * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64))
    return np.concatenate(words + [np.zeros(slack, np.uint64)])


# the asynchronous read-block upload: the raw bytes packed on the device.  (Every block with a base launches the kernel, from
# any kind of host memory; the reads here lie in pageable memory.)
add(dict(name="reads_upload_async", targets=(reads_pack(),), env={}, ctx=dict(kernel=AUTO), entry="reads_upload_async", params=dict(),
         gen=reads_block, ref="the image of bsw_reads_upload and a numpy packing of the bases (byte for byte)", seed=0, edges=()))


def cigar_specs(rng):
    """reads of both strands against a resident reference: retries, the no-gap shortcut, Ns, a long read"""
    import test_gpu_cigar_ref as T
    specs = []
    pac = cigar_genome()
    for lq in (1, 60, 150, 250, 1100):
        for strand in (0, 1):
            for k in range(3):
                rlen = max(1, lq + int(rng.integers(-lq // 20 - 1, lq // 20 + 2)))
                rb, re = T.interval(rng, rlen, strand)
                q = T.read_of(rng, pac, rb, re, lq, 0.03, 0.01, 0.02 if k else 0.0)
                specs.append(T.spec(q, rb, re, w=int(rng.choice([0, 5, 40, 100]))))
    for strand in (0, 1):
        rb, _ = T.interval(rng, 150, strand)
        specs.append(T.spec(T.retry_read(rng, pac, rb, [6, 6, -12]), rb, rb + 150, w=4, w_cap=64, min_score=1000, max_tries=3))
        rb, re = T.interval(rng, 150, strand)
        specs.append(T.spec(T.read_of(rng, pac, rb, re, 150, 0.05, 0.0), rb, re, w=0))
    return specs


_genome = {}


def cigar_genome():
    """the 2-bit reference the cigar case aligns against (the same for every call)"""
    if "pac" not in _genome:
        import _gencigar_ref as gc
        import test_gpu_cigar_ref as T
        _genome["pac"] = gc.pack_pac(np.random.default_rng(2025).integers(0, 4, T.L_PAC).astype(np.uint8))
    return _genome["pac"]


add(dict(name="cigar_ref", targets=(NS + "bsw_cigar_md_kernel", NS + "bsw_global_kernel<4>"), env={}, ctx=dict(kernel=AUTO),
         entry="cigar_ref_batch", params=dict(), gen=cigar_specs, ref="_gencigar_ref.reg2aln (score, CIGAR, NM, MD, w, tries, status)",
         seed=0, edges=()))


def targets():
    return set(t for c in CASES for t in c["targets"])


def groups():
    """{group name: [cases]}: the cases of one switch set run in one process"""
    out = {}
    for c in CASES:
        key = "product" if not c["env"] else "_".join("%s=%s" % (k[4:].lower(), v) for k, v in sorted(c["env"].items()))
        out.setdefault(key, []).append(c)
    return out


def make_params(host, case):
    over = dict(case["params"])
    mat = over.pop("mat", None)
    p = host.default_params(**over)
    if mat is not None:
        p["mat"][0] = host.bwa_matrix(a=mat[0], b=mat[1], n=mat[2])
    return p


def workload(case):
    return case["gen"](np.random.default_rng(case["seed"]))
