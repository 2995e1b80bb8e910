"""BSW_VARIANT_RTL on the CPU: known answers where RTL and H part, tests/ksw_extend_rtl_ref.c against a literal Python
transcription of the row loop, the reference's H / M against the oracle, the measured RTL / H cell ratio, and the host's
acceptance of variant 2."""
import numpy as np
import pytest

import _rtl_ref as R

MIX150 = dict(read_len=150, seed_len_min=19, seed_len_max=60, seed_at_start=0, sub_rate=0.01, indel_rate=0.001,
              junk_frac=0.05, n_rate=0.0005, w=100)
BP250 = dict(read_len=250, seed_len_min=19, seed_len_max=40, seed_at_start=0, sub_rate=0.04, indel_rate=0.01,
             junk_frac=0.05, n_rate=0.0005, w=500)


def bwa_mat(a=1, b=4, n=-1):
    m = np.full((5, 5), -b, np.int8)
    np.fill_diagonal(m, a)
    m[4, :] = n
    m[:, 4] = n
    return m


def ext(q, t, h0, w, o_del, e_del, o_ins, e_ins, variant, end_bonus=5, zdrop=0):
    return R.extend2(np.array(q), np.array(t), bwa_mat(), o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, variant)


A_, C_, G_, T_ = 0, 1, 2, 3


# ---- known answers (a = 1, b = 4; every value derived by hand below) ----

def test_kat_column0_at_beg_gt0_reaches_the_row_tail():
    """KAT 1 and 4: column 0 at beg > 0, on a junk side whose gtle / gscore then differ.
    q = T, t = C T, h0 = 8, w = 0, o_del = 1, e_del = 1, o_ins = 2, e_ins = 1 (oe_ins = 3).
    First row: eh[0].h = 8, eh[1].h = 8 - 3 = 5.
    Row 0: beg 0, end min(1, 0+0+1) = 1; h1 = 8 - (1 + 1) = 6 (beg == 0: both variants).
      j = 0: h = 8 + s(C,T) = 8 - 4 = 4; eh[0] = {6, e' = max(4 - 2, 0) = 2}.  mrow 4 at mj 0.
      K7: eh[1].h = 4; j == qlen -> gscore 4, max_ie 0.  4 < max 8.
      K8 H: eh[0] is non-zero -> beg 0; end = min(1 + 2, 1) = 1.  RTL: eh[0].h = 6 -> beg 0; mj + 2 = 2 > end -> end 2.
    Row 1: K3 beg = max(0, 1 - 0) = 1, end = min(end, 2, qlen 1) = 1: no cells.
      H: beg != 0 -> h1 = 0.  RTL: h1 = 8 - (1 + 1*2) = 5 — column 0 at beg = 1.
      K7: eh[1].h = h1; j == qlen: H 0 < 4 keeps gscore 4, gtle 1; RTL 5 >= 4 -> gscore 5, max_ie 1 -> gtle 2.
      mrow 0 -> stop.  Score 8 = h0, qle = tle = 0 in both."""
    args = ([T_], [C_, T_], 8, 0, 1, 1, 2, 1)
    h = ext(*args, variant=0)
    r = ext(*args, variant=2)
    assert h == dict(score=8, qle=0, tle=0, gtle=1, gscore=4, max_off=0, cells=1)
    assert r == dict(score=8, qle=0, tle=0, gtle=2, gscore=5, max_off=0, cells=1)


def test_kat_interior_zero_drops_the_run_without_mj():
    """KAT 2: q = G A G, t = G C, h0 = 1, o_del = e_del = o_ins = e_ins = 1 (oe = 2), w = 100.
    First row: eh[0].h = 1, eh[1].h = max(1 - 2, 0) = 0, the rest 0.
    Row 0 (t = G): beg 0, end 3, h1 = max(1 - 2, 0) = 0.
      j0: 1 + 1 = 2 -> eh[0] = {0, e 0}, f 0; mrow 2 at mj 0.  j1: 0 - 4 -> 0 -> eh[1].h = 2.  j2: 0 + 1 = 1 -> eh[2].h = 0.
      K7 eh[3].h = 1; j == qlen -> gscore 1, max_ie 0; 2 > max 1 -> max 2 at (0, 0).
      eh[].h = 0 2 0 1, every e 0: an interior zero (eh[2]) splits the run {1} holding mj + 1 from the run {3}.
      K8 H: beg 1 (first non-zero), end min(3 + 2, 3) = 3.  RTL: eh[0].h = 0 -> beg 1; eh[2].h = 0 -> end 2.
    Row 1 (t = C): H walks columns 1, 2 (cells 3 + 2 = 5), RTL column 1 only (3 + 1 = 4); every h is 0 -> stop.
    Everything but `cells` agrees."""
    args = ([G_, A_, G_], [G_, C_], 1, 100, 1, 1, 1, 1)
    assert ext(*args, variant=0) == dict(score=2, qle=1, tle=1, gtle=1, gscore=1, max_off=0, cells=5)
    assert ext(*args, variant=2) == dict(score=2, qle=1, tle=1, gtle=1, gscore=1, max_off=0, cells=4)


def test_kat_nonzero_e_with_zero_h_is_ignored():
    """KAT 3: a non-zero e next to a zero h — H keeps the entry in range, RTL, which never looks at e, trims it.
    q = T, t = T A, h0 = 2, w = 2, o_del = 1, e_del = 1 (oe_del 2), o_ins = 3, e_ins = 1 (oe_ins 4).
    First row: eh[0].h = 2, eh[1].h = max(2 - 4, 0) = 0.
    Row 0 (t = T): beg 0, end 1; h1 = 2 - 2 = 0.  j0: 2 + 1 = 3 -> eh[0] = {0, e max(3 - 2, 0) = 1}; mrow 3 at mj 0.
      K7 eh[1].h = 3; gscore 3 at i 0; max 3 at (0, 0).
      K8 H: eh[0] = {0, 1} is non-zero -> beg 0; end min(1 + 2, 1) = 1.  RTL: eh[0].h = 0 -> beg 1; end 2 (clamped to 1).
    Row 1 (t = A): H walks column 0 (h = max(0 - 4, e 1, 0) = 1, cells 2); RTL's range [1, 1) is empty (cells 1) and
      stops.  H: mrow 1 < 3, gscore stays 3 (j == qlen, h1 1 < 3).  Everything but `cells` agrees."""
    args = ([T_], [T_, A_], 2, 2, 1, 1, 3, 1)
    assert ext(*args, variant=0) == dict(score=3, qle=1, tle=1, gtle=1, gscore=3, max_off=0, cells=2)
    assert ext(*args, variant=2) == dict(score=3, qle=1, tle=1, gtle=1, gscore=3, max_off=0, cells=1)


# ---- the C reference against a literal transcription of the row loop ----

def extend2_py(q, t, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0, variant, wlim=0):
    qlen, tlen = len(q), len(t)
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    H = [0] * (qlen + 2)
    E = [0] * (qlen + 2)
    H[0] = h0
    if qlen >= 1:
        H[1] = h0 - oe_ins if h0 > oe_ins else 0
    j = 2
    while j <= qlen and H[j - 1] > e_ins:
        H[j] = H[j - 1] - e_ins
        j += 1
    mx = int(np.max(mat))
    max_ins = max(int((qlen * mx + end_bonus - o_ins) / e_ins + 1.), 1)
    max_del = max(int((qlen * mx + end_bonus - o_del) / e_del + 1.), 1)
    if wlim > 0:
        max_ins = max_del = wlim
    w = min(w, max_ins, max_del)
    best, max_i, max_j, max_ie, gscore, max_off = h0, -1, -1, -1, -1, 0
    beg, end, cells = 0, qlen, 0
    for i in range(tlen):
        f, mrow, mj = 0, 0, -1
        beg = max(beg, i - w)
        end = min(end, i + w + 1, qlen)
        h1 = max(h0 - (o_del + e_del * (i + 1)), 0) if (beg == 0 or variant == 2) else 0
        if end > beg:
            cells += end - beg
        j = beg
        while j < end:
            h, e, s = H[j], E[j], int(mat[t[i]][q[j]])
            H[j] = h1
            if variant == 1:
                M = h + s if h else 0
                h = max(M, e, f)
                base = M
            else:
                h = max(h + s, e, f)
                base = h
            h1 = h
            if h >= mrow:
                mrow, mj = h, j
            E[j] = max(e - e_del, base - oe_del, 0)
            f = max(f - e_ins, base - oe_ins, 0)
            j += 1
        H[end], E[end] = h1, 0
        if j == qlen:
            if h1 >= gscore:
                max_ie = i
            gscore = max(gscore, h1)
        if mrow == 0:
            break
        if mrow > best:
            best, max_i, max_j = mrow, i, mj
            max_off = max(max_off, abs(mj - i))
        elif zdrop > 0:
            di, dj = i - max_i, mj - max_j
            pen = (di - dj) * e_del if di > dj else (dj - di) * e_ins
            if best - mrow - pen > zdrop:
                break
        if variant == 2:
            j = mj
            while j >= beg and H[j]:
                j -= 1
            beg = j + 1
            j = mj + 2
            while j <= end and H[j]:
                j += 1
            end = j
        else:
            j = beg
            while j < end and H[j] == 0 and E[j] == 0:
                j += 1
            beg = j
            j = end
            while j >= beg and H[j] == 0 and E[j] == 0:
                j -= 1
            end = min(j + 2, qlen)
    return dict(score=best, qle=max_j + 1, tle=max_i + 1, gtle=max_ie + 1, gscore=gscore, max_off=max_off, cells=cells)


def test_reference_matches_the_transcription():
    rng = np.random.default_rng(2026)
    n_sides, n_differ = 0, 0
    for k in range(2200):
        ql = int(rng.integers(1, 33))
        tl = int(rng.integers(0, 48))
        t = rng.integers(0, 4, tl).astype(np.uint8)
        if rng.random() < 0.3 or tl == 0:
            q = rng.integers(0, 4, ql).astype(np.uint8)
        else:
            q = np.resize(t[:ql], ql).copy()
            q[rng.random(ql) < 0.1] = rng.integers(0, 4)
        if rng.random() < 0.2:
            q[rng.random(ql) < 0.1] = 4
            t[rng.random(tl) < 0.1] = 4
        a, b = int(rng.integers(1, 4)), int(rng.integers(1, 6))
        mat = bwa_mat(a, b, -int(rng.integers(0, 3)))
        o_del, e_del = int(rng.integers(0, 8)), int(rng.integers(1, 4))
        o_ins, e_ins = int(rng.integers(0, 8)), int(rng.integers(1, 4))
        w = int(rng.integers(0, 40))
        zdrop = int(rng.choice([0, 5, 20]))
        h0 = int(rng.integers(1, 40))
        wlim = int(rng.choice([0, 0, 3, 10]))
        tries = int(rng.integers(1, 4))
        got = {}
        for variant in (0, 2):
            for k2 in range(tries):                      # the band retry's widths: each pass starts from fresh state
                aw = w << k2
                want = extend2_py(q, t, mat, o_del, e_del, o_ins, e_ins, aw, 5, zdrop, h0, variant, wlim)
                have = R.extend2(q, t, mat, o_del, e_del, o_ins, e_ins, aw, 5, zdrop, h0, variant, wlim)
                assert have == want, (k, variant, aw, have, want)
            got[variant] = have
        n_sides += 1
        n_differ += got[0] != got[2]
    assert n_differ > n_sides // 50, (n_differ, n_sides)     # the cases exercise RTL's own blocks


# ---- H / M of the new reference are the oracle's ----

@pytest.mark.parametrize("variant", [0, 1])
def test_reference_h_m_equal_the_oracle(host, oracle, variant):
    for spec, n in ((MIX150, 3000), (BP250, 600)):
        p = host.default_params(variant=variant, w=spec["w"])
        tasks, arena = host.synth_tasks(n, seed=91 + variant, **spec)
        assert R.pair_batch(p, tasks).tobytes() == oracle.pair_batch(p, tasks, nthreads=4).tobytes()
    rng = np.random.default_rng(7 + variant)
    import _gen
    tasks, arena = host.make_tasks(_gen.random_seeds(rng, 1500, qmax=100, nrate=0.02))
    for over in (dict(), dict(zdrop=0), dict(o_del=3, e_del=2, o_ins=5, e_ins=1), dict(max_band_try=3, w=5)):
        p = host.default_params(variant=variant, **over)
        assert R.pair_batch(p, tasks).tobytes() == oracle.pair_batch(p, tasks, nthreads=4).tobytes(), over


# ---- how much RTL differs from H, and how many cells it walks (recorded in DESIGN.md §4.4) ----

def rtl_vs_h(host, spec, n, seed):
    p = host.default_params(w=spec["w"])
    tasks, arena = host.synth_tasks(n, seed=seed, **spec)
    h = R.pair_batch(R.with_variant(p, 0), tasks)
    r = R.pair_batch(R.with_variant(p, 2), tasks)
    has = np.concatenate([tasks["lqlen"] > 0, tasks["rqlen"] > 0])
    diff = R.sides_differ(h, r, ("gscore", "gtle"))[has]
    cells_h = int(h["left"]["cells"].sum() + h["right"]["cells"].sum())
    cells_r = int(r["left"]["cells"].sum() + r["right"]["cells"].sum())
    pair_fields = ["qb", "qe", "rb", "re", "score", "truesc", "w"]
    pair_diff = np.any(np.stack([h[f] != r[f] for f in pair_fields]), axis=0)
    return cells_r / cells_h, float(diff.mean()), float(pair_diff.mean())


def test_rtl_walks_fewer_cells_than_h(host):
    ratio150, d150, p150 = rtl_vs_h(host, MIX150, 20000, 1)
    ratio250, d250, p250 = rtl_vs_h(host, BP250, 4000, 2)
    print("150 bp mix: RTL/H cells %.3f, sides with gscore/gtle differing %.2f %%, pairs differing %.2f %%" % (ratio150, 100 * d150, 100 * p150))
    print("250 bp w500: RTL/H cells %.3f, sides with gscore/gtle differing %.2f %%, pairs differing %.2f %%" % (ratio250, 100 * d250, 100 * p250))
    # measured: 150 bp 0.667x of H's cells, 2.09 % of sides differ; 250 bp / w500 0.462x, 3.33 %
    assert ratio150 < 0.75 and ratio250 < 0.55
    assert 0.01 < d150 < 0.04 and 0.015 < d250 < 0.06


# ---- the host accepts variant 2 and nothing above it ----

def test_plan_batch_accepts_rtl_and_rejects_3(host):
    tasks, arena = host.synth_tasks(64, seed=3)
    host.plan_batch(host.default_params(variant=host.VARIANT_RTL), tasks)
    with pytest.raises(host.BswError) as ei:
        host.plan_batch(host.default_params(variant=3), tasks)
    assert ei.value.code == -2
